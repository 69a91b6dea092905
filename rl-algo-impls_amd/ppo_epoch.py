"""PPO updates that are n_epochs launches of ONE whole-epoch kernel: which policies and options they
cover, the driver all four share (_run_epochs) and the four launches.  A base class of PPO (ppo.py).

    _update_fused           rai_mlp_ppo_epoch           CartPole-class MLP, single process
    _update_fused_dp        rai_mlp_ppo_epoch_xdp / rai_mlp_ppo_epoch_dp / the rai_mlp_ppo_grads loop
    _update_wide_epoch      rai_mlp_wide_epoch          wide MLP (HalfCheetah class), single process
    _update_wide_epoch_xdp  rai_mlp_wide_epoch_xdp      the same over the in-kernel cross-GPU exchange
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib


class PPOEpochKernels:
    _we_ws: Optional[torch.Tensor] = None  # rai_mlp_wide_epoch's workspace (_mlp_ws: rai_mlp_ppo_epoch's)
    _grad_alt: Optional[torch.Tensor] = None
    _prep_stream: Optional[torch.cuda.Stream] = None

    # -- which update a whole-epoch kernel covers --------------------------------------------
    def _plain_options(self) -> bool:
        """The loss options every whole-epoch kernel is written for: an optimizer step per minibatch, no
        kl_cutoff, one advantage and value column with a scalar vf_coef, normalisation before scaling."""
        return not (self.gradient_accumulation or self.kl_cutoff is not None or self.multi_reward_weights is not None
                    or self.vf_weights is not None or self.normalize_advantages_after_scaling
                    or np.ndim(self.vf_coef) > 0)

    def _fused_kernels_off(self, r=None) -> bool:
        """No fused MLP kernel for this update (of rollout r): force_generic, a teacher term (the fused
        kernels carry none: the network + rai_ppo_loss_teacher run), a freeze_* flag or parameters at
        different optimizer steps after one (the whole-epoch kernels and WideStep carry ONE Adam step
        count and would apply wrong bias corrections: rai_clip_optim_step_runs runs per minibatch) or
        action masks (no mask input: the per-minibatch policy forward receives Batch.action_masks)."""
        return (self.force_generic or self._teacher_on() or self._freeze_on() or not self.optimizer.uniform()
                or (r is not None and getattr(r, "action_masks", None) is not None))

    def fused_mlp_spec(self) -> Optional[dict]:
        """Shape descriptor if the policy/options fit rai_mlp_ppo_epoch (CartPole-class MLP
        actor-critic: Flatten encoder, [in -> 64 -> 64 -> out] actor and critic, Categorical
        head); None otherwise (the generic per-minibatch path then runs)."""
        from .policy import mlp_actor_critic_spec

        if self._fused_kernels_off():
            return None
        spec = mlp_actor_critic_spec(self.policy)
        if spec is None or self.batch_size < 2:
            return None
        # > 256 rows per minibatch (SURVEY 8(d) batch policy (b)): the all-CU large-minibatch kernels of
        # rai_mlp_ppo_epoch / rai_mlp_ppo_grads (csrc/mlp_large.hip) cover in_dim <= 4, two actions
        if self.batch_size > _lib.RAI_MLP_EPOCH_MAX_B and not (spec["in_dim"] <= 4 and spec["n_act"] == 2):
            return None
        return spec if self._plain_options() else None

    def _wide_epoch_options_ok(self) -> bool:
        """The options rai_mlp_wide_epoch covers: K = 1, Adam, minibatches of 2..64 rows (per rank), no
        gradient accumulation / kl_cutoff / multi-reward weights / vf_weights."""
        if os.environ.get("RAI_WIDE_EPOCH", "1") == "0":
            return False
        if not self._plain_options() or self.optimizer.kind != self.optimizer.ADAM:
            return False
        return 2 <= self.batch_size <= 64

    def _wide_epoch_step(self, r):
        """The WideStep (descriptor) when the whole epoch can run as ONE persistent launch
        (rai_mlp_wide_epoch): a wide-MLP policy within _wide_epoch_options_ok, single process or data
        parallel over the in-kernel cross-GPU exchange (rai_mlp_wide_epoch_xdp).
        RAI_WIDE_EPOCH=0 keeps the graph-replayed per-minibatch path."""
        if not hasattr(r, "epoch_batch") or (self.dp_enabled and self._xdp is None):
            return None
        if self._fused_kernels_off(r) or not self._wide_epoch_options_ok():
            return None
        if r.total_steps < 2 or (not self.dp_enabled and r.total_steps % self.batch_size == 1):
            return None
        return self._wide_step()

    def _wide_step(self):
        """The wide-MLP fused step for this policy, or None (structure / options not covered)."""
        if self._fused_kernels_off() or not self.use_wide or not self.flat.flat.is_cuda:
            return None
        if self._wide is None:
            from .mlp_wide import WideStep, wide_mlp_spec

            if wide_mlp_spec(self.policy) is None or not (1 <= self.batch_size <= _lib.RAI_WIDE_MAX_B):
                self._wide = False
            else:
                self._wide = WideStep(self.policy, self.device, accumulate=self.gradient_accumulation)
        if self._wide is False:
            return None
        self._wide.check_pointers()
        return self._wide

    # -- the driver --------------------------------------------------------------------------
    def _run_epochs(self, r, launch, what: str) -> Tuple[np.ndarray, np.ndarray, int]:
        """n_epochs launches of a whole-epoch kernel over rollout r and the update's one read-back.
        launch(rows, tables, moments) makes the C call; the tuples hold arguments every entry point takes
        in this order: rows = the epoch's permuted copy (f32 contiguous obs, actions, logprobs, values,
        advantages, returns, row count, batch_size), tables = (hparams, optimizer hparams, train state,
        stats, stats rows, norms, norms rows); moments = the global minibatches' advantage (mean, den)
        under data parallel, else None.  `what` names the launch in the error of a kernel whose
        device-side wait expired."""
        nmb = r.num_minibatches(self.batch_size)
        n_steps = self.n_epochs * nmb
        blocks, opt = self.blocks, self.optimizer
        blocks.ensure_tables(n_steps, n_steps)
        blocks.upload(self._hparams(1, nmb), opt.step_count)
        tables = (blocks.hp.data_ptr(), opt.hp_dev.data_ptr(), blocks.state.data_ptr(), blocks.stats.data_ptr(),
                  int(blocks.stats.shape[0]), blocks.norms.data_ptr(), int(blocks.norms.shape[0]))
        xdp = self._xdp if self.dp_enabled else None  # the sums over the ranks happen inside the kernel
        timed = self.kernel_events is not None and (xdp is not None or not self.dp_enabled)
        epochs = self._dp_epochs(r, nmb) if self.dp_enabled else self._overlapped_epochs(r)
        for b, obs, moments in epochs:
            actions = b.actions.contiguous()
            rows = (obs.data_ptr(), actions.data_ptr(), b.logprobs.data_ptr(), b.values.data_ptr(),
                    b.advantages.data_ptr(), b.returns.data_ptr(), r.total_steps, self.batch_size)
            if timed:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            launch(rows, tables, moments)
            if timed:
                ev[1].record()
                self.kernel_events.append(ev)
            if xdp is not None:
                xdp["step"] += nmb
            opt.step_count += nmb
        return self._read_tables(n_steps, n_steps, what=what, agree=xdp is not None)

    def _overlapped_epochs(self, r):
        """Single process: yields each epoch's (batch, f32 contiguous obs, None); the caller launches the
        epoch's kernel on the current stream before it asks for the next.  Epoch k + 1's permutation and
        gather (rai_feistel_permutation + one gather) run on a side stream into the other of two permuted
        copies while epoch k's kernel runs, so the launches follow each other without them.  Same
        permutations: the shuffle keys are drawn on the host in the same order.  A rollout without the
        two slots (only DeviceRollout has them) is prepared in order on the current stream."""
        cur = torch.cuda.current_stream(self.device)
        two_slots = hasattr(r, "alloc_epoch_buffers")
        side = self._epoch_prep_stream() if two_slots else cur
        if two_slots:
            for slot in (0, 1):
                r.alloc_epoch_buffers(slot)
            side.wait_stream(cur)  # the rollout, its GAE and the parameters are ready

        def prep(k):
            with torch.cuda.stream(side):
                bk = r.epoch_batch(shuffle=True, slot=k % 2) if two_slots else r.epoch_batch(shuffle=True)
                assert bk.logprobs is not None, "PPO needs rollout logprobs (include_logp=True)"
                obs_k = bk.obs if bk.obs.dtype == torch.float32 else bk.obs.float()
                obs_k = obs_k.contiguous()
                if obs_k.data_ptr() != bk.obs.data_ptr():
                    obs_k.record_stream(cur)
                ready = torch.cuda.Event()
                ready.record(side)
            return bk, obs_k, ready

        nxt = prep(0)
        done: List[torch.cuda.Event] = []
        for k in range(self.n_epochs):
            b, obs, ready = nxt
            cur.wait_event(ready)
            yield b, obs, None
            done.append(torch.cuda.Event())
            done[-1].record(cur)
            if k + 1 < self.n_epochs:
                if k >= 1 and two_slots:
                    side.wait_event(done[k - 1])  # slot (k + 1) % 2 was read by epoch k - 1
                nxt = prep(k + 1)
        cur.wait_stream(side)

    def _dp_epochs(self, r, nmb: int):
        """Data parallel: yields each epoch's (batch, f32 contiguous obs, moments), prepared in order on
        the current stream; the global minibatches' advantage moments take one small all-reduce."""
        for _ in range(self.n_epochs):
            b = r.epoch_batch(shuffle=True)
            assert b.logprobs is not None, "PPO needs rollout logprobs (include_logp=True)"
            moments = self._global_adv_moments(b.advantages, nmb).view(nmb, 2)
            # the kernels apply A = (A - mean) / den as given: encode the reference's rule
            if not self.normalize_advantage:
                moments[:, 0] = 0.0
                if not self.standardize_advantage:
                    moments[:, 1] = 1.0
            yield b, (b.obs if b.obs.dtype == torch.float32 else b.obs.float()).contiguous(), moments

    def _epoch_prep_stream(self) -> torch.cuda.Stream:
        if self._prep_stream is None:
            self._prep_stream = torch.cuda.Stream(self.device)
        return self._prep_stream

    # -- workspaces --------------------------------------------------------------------------
    def _ensure_mlp_workspace(self, n_rows: int) -> torch.Tensor:
        need = int(_lib.lib().rai_mlp_ppo_workspace_bytes(n_rows, self.batch_size))
        if self._mlp_ws is None or self._mlp_ws.numel() < need:
            self._mlp_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._mlp_ws

    def _ensure_wide_epoch_workspace(self, wide, n_rows: int) -> torch.Tensor:
        need = int(_lib.lib().rai_mlp_wide_epoch_workspace_bytes(wide.spec["hidden"], wide.desc.in_dim, n_rows))
        if self._we_ws is None or self._we_ws.numel() < need:
            self._we_ws = torch.zeros(need, dtype=torch.uint8, device=self.device)
        return self._we_ws

    # -- the four launches -------------------------------------------------------------------
    def _update_fused(self, r, spec) -> Tuple[np.ndarray, np.ndarray, int]:
        if r.total_steps % self.batch_size == 1:
            raise ValueError("a 1-row minibatch has no unbiased std (reference would produce NaN)")
        L, st, f, opt = _lib.lib(), _lib.stream_handle(self.device), self.flat, self.optimizer
        ws = self._ensure_mlp_workspace(r.total_steps)

        def launch(rows, tables, _):
            _lib.check(L.rai_mlp_ppo_epoch(
                f.flat.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr(), *rows, spec["in_dim"], 64,
                spec["n_act"], spec["activation"], *tables, ws.data_ptr(), ws.numel(), st), "rai_mlp_ppo_epoch")

        return self._run_epochs(r, launch, "rai_mlp_ppo_epoch: device-side exchange")

    def _update_fused_dp(self, r, spec) -> Tuple[np.ndarray, np.ndarray, int]:
        """Data-parallel CartPole-class epochs: one launch with the cross-GPU sums inside the kernel, else
        the natively driven loop (grads -> RCCL all-reduce -> clip+Adam), else that loop from Python."""
        L, st, f, opt, x = _lib.lib(), _lib.stream_handle(self.device), self.flat, self.optimizer, self._xdp
        ws = self._ensure_mlp_workspace(r.total_steps)
        shape = (spec["in_dim"], 64, spec["n_act"], spec["activation"])
        if x is not None:
            def launch(rows, tables, moments):
                _lib.check(L.rai_mlp_ppo_epoch_xdp(
                    f.flat.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr(), *rows, moments.data_ptr(),
                    self.world, x["rank"], x["peers"].data_ptr(), x["step"], *shape, *tables, ws.data_ptr(),
                    ws.numel(), st), "rai_mlp_ppo_epoch_xdp")
        elif self._dp_comm is not None:
            if self._grad_alt is None or self._grad_alt.numel() != f.P:
                self._grad_alt = torch.zeros_like(f.grad)

            def launch(rows, tables, moments):
                _lib.check(L.rai_mlp_ppo_epoch_dp(
                    f.flat.data_ptr(), f.grad.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr(), f.P, *rows,
                    moments.data_ptr(), self.world, *shape, *tables, self._dp_comm, self._grad_alt.data_ptr(),
                    ws.data_ptr(), ws.numel(), opt.workspace.data_ptr(), opt.workspace.numel(), st),
                    "rai_mlp_ppo_epoch_dp")
        else:
            def launch(rows, tables, moments):
                for i in range(r.num_minibatches(self.batch_size)):
                    _lib.check(L.rai_mlp_ppo_grads(
                        f.flat.data_ptr(), *rows, i, 1, moments.data_ptr(), self.world, *shape, *tables[:3],
                        f.grad.data_ptr(), *tables[3:5], ws.data_ptr(), ws.numel(), st), "rai_mlp_ppo_grads")
                    self._all_reduce(f.grad)
                    opt.step(self.blocks.state, self.blocks.norms, count=False)  # _run_epochs counts the epoch's

        return self._run_epochs(r, launch, "fused data-parallel update: a device-side exchange")

    def _update_wide_epoch(self, r, wide) -> Tuple[np.ndarray, np.ndarray, int]:
        L, st, f, opt = _lib.lib(), _lib.stream_handle(self.device), self.flat, self.optimizer
        ws = self._ensure_wide_epoch_workspace(wide, r.total_steps)

        def launch(rows, tables, _):
            _lib.check(L.rai_mlp_wide_epoch(
                C.byref(wide.desc), f.flat.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr(), f.P, *rows,
                *tables, ws.data_ptr(), ws.numel(), st), "rai_mlp_wide_epoch")

        return self._run_epochs(r, launch, "rai_mlp_wide_epoch: a device-side hand-off")

    def _update_wide_epoch_xdp(self, r, wide) -> Tuple[np.ndarray, np.ndarray, int]:
        """The data-parallel form: the launch's workgroups sum their owned gradients over the ranks
        inside the kernel; the stats rows are summed over the ranks after."""
        L, st, f, opt, x = _lib.lib(), _lib.stream_handle(self.device), self.flat, self.optimizer, self._xdp
        ws = self._ensure_wide_epoch_workspace(wide, r.total_steps)

        def launch(rows, tables, moments):
            _lib.check(L.rai_mlp_wide_epoch_xdp(
                C.byref(wide.desc), f.flat.data_ptr(), opt.state1.data_ptr(), opt.state2.data_ptr(), f.P, *rows,
                moments.data_ptr(), self.world, x["rank"], x["peers"].data_ptr(), x["step"], *tables, ws.data_ptr(),
                ws.numel(), st), "rai_mlp_wide_epoch_xdp")

        return self._run_epochs(r, launch, "rai_mlp_wide_epoch_xdp: a device-side hand-off")
