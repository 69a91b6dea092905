"""PPO on MI355X — drop-in for rl_algo_impls/ppo/ppo.py:106-447.

Same constructor kwargs, same mutable attributes (learning_rate, clip_range,
ent_coef, gamma, gae_lambda, vf_coef, ... — what HyperparamTransitions and
LearningRateByKLDivergence set), same learn()/learn_epoch() contract, same
TrainStats and tensorboard tags, same `train/steps_per_second` definition
(wall time of learn_epoch before callbacks, ppo.py:221,422-427).

PPO.update picks one of five paths; none synchronises with the host until the update ends:

  here          per minibatch: PyTorch-ROCm forward of the policy on a contiguous slice of the permuted
                HBM rollout (or the fused wide-MLP forward/backward kernels) -> ONE fused HIP loss kernel
                (advantage normalisation, clipped surrogate, value/entropy/teacher-KL loss, gradients
                w.r.t. the network outputs, stats row) -> PyTorch-ROCm backward seeded with those
                gradients -> ONE fused clip_grad_norm_ + Adam step (two HIP launches) over the flat
                parameter buffer; replayed from a hipGraph (_update_graphed) or as an eager loop
  ppo_epoch.py  one kernel launch per epoch, four forms on one driver: CartPole-class MLPs
                (_update_fused; data parallel _update_fused_dp) and wide MLPs (_update_wide_epoch; over
                the in-kernel cross-GPU exchange _update_wide_epoch_xdp), and the tests of which
                policies and options they cover
  ppo_dp.py     the data-parallel set-up those paths run over (enable_data_parallel)
"""
from __future__ import annotations

import gc
import logging
import os
from time import perf_counter
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .optim import FlatOptimizer, FlatParams
from .pg_common import (DeviceBlocks, TrainStats, launch_loss, load_optimizer, log_scalars, make_hparams,
                        num_or_array, save_optimizer, unsupported, value_columns)
from .ppo_dp import PPODataParallel
from .ppo_epoch import PPOEpochKernels


class PPO(PPOEpochKernels, PPODataParallel):
    def __init__(self, policy, device: torch.device, tb_writer, learning_rate: float = 3e-4,
                 batch_size: int = 64, n_epochs: int = 10, gamma=0.99, gae_lambda=0.95, clip_range: float = 0.2,
                 clip_range_vf: Optional[float] = None, normalize_advantage: bool = True,
                 standardize_advantage: bool = False, ent_coef: float = 0.0, vf_coef=0.5,
                 ppo2_vf_coef_halving: bool = False, max_grad_norm: float = 0.5,
                 multi_reward_weights: Optional[List[float]] = None, gradient_accumulation: bool = False,
                 kl_cutoff: Optional[float] = None, freeze_policy_head: bool = False,
                 freeze_value_head: bool = False, freeze_backbone: bool = False, switch_range=None,
                 guide_probability=None, normalize_advantages_after_scaling: bool = False,
                 autocast_loss: bool = False, vf_loss_fn: str = "mse_loss", vf_weights=None,
                 teacher_kl_loss_coef=None, teacher_kl_loss_fn=None, teacher_loss_importance_sampling=True):
        unsupported(switch_range=switch_range is not None, guide_probability=guide_probability is not None,
                    autocast_loss=autocast_loss)
        # ppo.py:280-285,412-413: policy.freeze(...) around the update; HyperparamTransitions sets these
        self.freeze_policy_head = freeze_policy_head
        self.freeze_value_head = freeze_value_head
        self.freeze_backbone = freeze_backbone
        assert not (normalize_advantage and standardize_advantage), "Cannot both normalize and standardize advantage"
        # the teacher-KL term (ppo.py:188-190,363-371): on when the coefficient is truthy; the loss fn's
        # add_to_batch runs after every rollout whenever the fn is set
        assert not teacher_kl_loss_coef or teacher_kl_loss_fn is not None, \
            "teacher_kl_loss_coef needs a teacher_kl_loss_fn (TeacherKLLoss)"
        self.teacher_kl_loss_coef = teacher_kl_loss_coef
        self.teacher_kl_loss_fn = teacher_kl_loss_fn
        self.teacher_loss_importance_sampling = teacher_loss_importance_sampling
        self._teacher_stats: Optional[np.ndarray] = None
        self.policy = policy
        self.device = torch.device(device)
        self.tb_writer = tb_writer
        self.learning_rate = learning_rate
        cl = policy.channels_last_params() if self.device.type == "cuda" and hasattr(policy, "channels_last_params") else ()
        self.flat = FlatParams(policy, self.device, channels_last=cl)
        self.optimizer = FlatOptimizer(self.flat, FlatOptimizer.ADAM, lr=learning_rate, eps=1e-7,
                                       max_grad_norm=max_grad_norm)
        self.gamma = num_or_array(gamma)
        self.gae_lambda = num_or_array(gae_lambda)
        self.max_grad_norm = max_grad_norm
        self.clip_range = clip_range
        self.clip_range_vf = clip_range_vf
        self.normalize_advantage = normalize_advantage
        self.standardize_advantage = standardize_advantage
        self.ent_coef = ent_coef
        self.vf_coef = num_or_array(vf_coef)
        self.vf_weights = np.array(vf_weights) if vf_weights is not None else None
        self.ppo2_vf_coef_halving = ppo2_vf_coef_halving
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.multi_reward_weights = np.array(multi_reward_weights) if multi_reward_weights else None
        self.gradient_accumulation = gradient_accumulation
        self.kl_cutoff = kl_cutoff
        self.normalize_advantages_after_scaling = normalize_advantages_after_scaling
        self.vf_loss_fn = vf_loss_fn
        self.blocks = DeviceBlocks(self.device)
        self.last_update_seconds: Optional[float] = None
        self.force_generic = False  # True: always use the per-minibatch (PyTorch network) path
        # generic path: capture the minibatch step into a hipGraph and replay it (graphs.py);
        # RAI_GRAPHS=0 keeps the eager loop
        self.use_graphs = os.environ.get("RAI_GRAPHS", "1") != "0"
        self._graphed = None
        # wide MLP actor-critics (HalfCheetah class): fused forward/backward kernels instead of the
        # PyTorch module + autograd (mlp_wide.py); RAI_WIDE=0 keeps the PyTorch network path
        self.use_wide = os.environ.get("RAI_WIDE", "1") != "0"
        self._wide = None
        self._wide_out: dict = {}
        # bench/profiling hook: when a list, (start, end) HIP events bracket every fused epoch launch
        self.kernel_events: Optional[list] = None
        self._mlp_ws: Optional[torch.Tensor] = None
        self.dp_group = None
        self.world = 1
        self._dp_comm = None
        self.dp_enabled = False  # enable_data_parallel() called (any world size, incl. 1-rank rehearsal)
        self.dp_batch = "per-rank"
        self.dp_update_mode = "exchange"  # or "replicated" (enable_data_parallel)
        self.global_batch_size = batch_size
        self._yaml_batch_size = batch_size  # enable_data_parallel derives the per-rank size from it
        self._buckets = None

    # -- reference API -------------------------------------------------------------------
    def learn(self, train_timesteps: int, rollout_generator, callbacks=None, total_timesteps=None,
              start_timesteps: int = 0) -> "PPO":
        if total_timesteps is None:
            total_timesteps = train_timesteps
        assert start_timesteps + train_timesteps <= total_timesteps
        timesteps_elapsed = start_timesteps
        while timesteps_elapsed < start_timesteps + train_timesteps:
            timesteps_elapsed, should_continue = self.learn_epoch(timesteps_elapsed, total_timesteps,
                                                                  rollout_generator, callbacks)
            gc.collect()
            if not should_continue:
                break
        return self

    def _hparams(self, K: int, num_minibatches: int):
        return make_hparams(
            loss_kind=0, K=K, clip_range=self.clip_range, clip_range_vf=self.clip_range_vf,
            ent_coef=self.ent_coef, vf_coef=self.vf_coef, vf_weights=self.vf_weights,
            multi_reward_weights=self.multi_reward_weights, normalize_advantage=self.normalize_advantage,
            standardize_advantage=self.standardize_advantage,
            normalize_after_scaling=self.normalize_advantages_after_scaling,
            ppo2_vf_coef_halving=self.ppo2_vf_coef_halving, kl_cutoff=self.kl_cutoff, vf_loss_fn=self.vf_loss_fn,
            grad_scale=(1.0 / num_minibatches) if self.gradient_accumulation else 1.0)

    def learn_epoch(self, timesteps_elapsed: int, total_timesteps: int, rollout_generator,
                    callbacks=None) -> Tuple[int, bool]:
        start_time = perf_counter()
        self.optimizer.param_groups[0]["lr"] = self.learning_rate  # update_learning_rate (schedule.py:64-66)
        self.optimizer.max_grad_norm = self.max_grad_norm
        self.optimizer.sync_hparams()
        chart = {"learning_rate": self.learning_rate, "ent_coef": self.ent_coef, "pi_clip": self.clip_range,
                 "gamma": self.gamma, "gae_lambda": self.gae_lambda, "vf_coef": self.vf_coef}
        if self.clip_range_vf is not None:
            chart["v_clip"] = self.clip_range_vf
        if self.multi_reward_weights is not None:
            chart["reward_weights"] = self.multi_reward_weights
        if self.vf_weights is not None:
            chart["vf_weights"] = self.vf_weights
        if self.teacher_kl_loss_coef is not None:
            chart["teacher_kl_loss_coef"] = self.teacher_kl_loss_coef
        log_scalars(self.tb_writer, "charts", chart, timesteps_elapsed)

        if self.world > 1 and not getattr(rollout_generator, "data_parallel", True):
            raise NotImplementedError(f"{type(rollout_generator).__name__} under data parallel (world > 1)")
        r = rollout_generator.rollout(gamma=self.gamma, gae_lambda=self.gae_lambda)
        if self.teacher_kl_loss_fn:  # ppo.py:259-262
            r.add_to_batch(self.teacher_kl_loss_fn.add_to_batch, rollout_generator.vec_env.num_envs)
        self.last_rollout_seconds = perf_counter() - start_time  # host env + policy steps (synced per step)
        timesteps_elapsed += r.total_steps
        stats, norms, K = self.update(r)
        ru = getattr(self, "last_update_rollout", None) or r  # the whole env group's under replicated DP
        explained_var = ru.explained_variance()
        train_stats = self._train_stats(stats, norms, K, ru.num_minibatches(self.batch_size), explained_var)
        train_stats.write_to_tensorboard(self.tb_writer)
        end_time = perf_counter()
        self.last_update_seconds = end_time - start_time
        if self.tb_writer is not None:
            self.tb_writer.add_scalar("train/steps_per_second", r.total_steps / (end_time - start_time))
            if hasattr(self.tb_writer, "on_steps"):
                self.tb_writer.on_steps(r.total_steps)
        self.last_train_stats = train_stats
        if callbacks:
            if not all(c.on_step(timesteps_elapsed=r.total_steps, train_stats=train_stats) for c in callbacks):
                logging.info(f"Callback terminated training at {timesteps_elapsed} timesteps")
                return timesteps_elapsed, False
        return timesteps_elapsed, True

    def _teacher_on(self) -> bool:
        """The teacher-KL term is part of the loss (ppo.py:363: a truthy coefficient)."""
        return bool(self.teacher_kl_loss_coef) and self.teacher_kl_loss_fn is not None

    def _teacher_field(self, r, wide) -> Optional[torch.Tensor]:
        """The rollout's flat teacher_logprobs when the per-minibatch path launches rai_ppo_loss_teacher:
        the field is there (add_to_batch ran) and the loss kernel is the standalone one.  A coefficient
        of 0 keeps the launch (the kernel then computes rai_ppo_loss's loss exactly), so a schedule that
        reaches 0 replays the graph it captured."""
        if self.teacher_kl_loss_fn is None or wide is not None:
            return None
        t = getattr(r, "additional", {}).get("teacher_logprobs")
        if t is None and not self._teacher_on():
            return None
        # every update with the term on comes through here (_fused_kernels_off), the replicated one too:
        # its rollout of the whole env group carries no additional fields, and world stays > 1 inside it
        if self.world > 1:
            raise NotImplementedError("the teacher-KL term under data parallel (world > 1)")
        if t is None:
            raise ValueError("teacher_kl_loss_coef is set but the rollout carries no teacher_logprobs "
                             "(Rollout.add_to_batch with TeacherKLLoss.add_to_batch)")
        return t

    def _teacher_block(self) -> _lib.TeacherKL:
        return _lib.TeacherKL(coef=float(self.teacher_kl_loss_coef or 0.0),
                              unbiased=int(bool(self.teacher_kl_loss_fn.unbiased)),
                              importance_sampling=int(bool(self.teacher_loss_importance_sampling)))

    def _minibatch_loss_grads(self, wide, obs, actions, masks, values, adv, ret, logprobs, K_box,
                              obs_prepared: bool = False, teacher_logp=None) -> None:
        """Forward, fused loss and backward of one minibatch into the flat gradient buffer: the
        wide-MLP kernels when available, else the PyTorch network + autograd (NatureCNN layers
        with the cnn_ops epilogues accumulating straight into the flat gradient views).
        teacher_logp: the minibatch's teacher log-probabilities (rai_ppo_loss_teacher)."""
        if wide is not None and masks is None:
            assert teacher_logp is None
            B = int(obs.shape[0])
            outs = self._wide_out.get(B)
            if outs is None:
                outs = self._wide_out[B] = wide.outputs(B)
            logp, ent, v = outs
            K_box[0] = 1
            d_logp, d_ent, d_v = wide.forward_loss(obs, actions, logp, ent, v, self.blocks, logprobs, values, adv,
                                                   ret)
            wide.backward(obs, actions, d_logp, d_ent, d_v)
            return
        from .cnn_ops import direct_grads

        with direct_grads(self.flat.flat.is_cuda):
            if obs_prepared:
                logp, ent, v = self.policy(obs, actions, action_masks=masks, obs_prepared=True)
            else:
                logp, ent, v = self.policy(obs, actions, action_masks=masks)
            if K_box[0] is None:
                K_box[0] = value_columns(v)
            d_logp, d_ent, d_v = launch_loss(self.blocks, logp, ent, v, logprobs, values, adv, ret, K_box[0],
                                             teacher_logp=teacher_logp)
            # (a frozen head under a frozen backbone leaves its outputs without a graph: freeze_*)
            outs = [(o, d) for o, d in ((logp, d_logp), (ent, d_ent), (v, d_v)) if o.requires_grad]
            torch.autograd.backward([o for o, _ in outs], [d for _, d in outs])

    def _freeze_on(self) -> bool:
        return bool(self.freeze_policy_head or self.freeze_value_head or self.freeze_backbone)

    def update(self, r) -> Tuple[np.ndarray, np.ndarray, int]:
        """All epochs x minibatches of one update, enqueued without host syncs;
        returns the per-minibatch stats rows and grad norms (one D2H copy).

        With a freeze_* flag set the update runs between policy.freeze(...) and policy.unfreeze()
        (ppo.py:280-285,412-413).  torch's semantics are per tensor: a frozen tensor has no gradient,
        clip_grad_norm_ sums over the others, Adam skips it (no moment update, no step increment).
        Here the optimizer's frozen mask comes from requires_grad over the flat parameters and the step is
        rai_clip_optim_step_runs; afterwards the frozen parameters' lag grows by the steps taken.  Such an
        update, and every later one of a policy whose parameters' step counts differ, runs on the
        per-minibatch path: the whole-epoch kernels and WideStep carry ONE Adam step count
        (_fused_kernels_off)."""
        opt = self.optimizer
        if not self._freeze_on():
            if self.world > 1 and opt.lag.any():
                raise NotImplementedError("parameters at different optimizer steps (after a freeze_* phase) "
                                          "under data parallel (world > 1)")
            return self._update(r)
        if self.world > 1:
            raise NotImplementedError("freeze_policy_head / freeze_value_head / freeze_backbone under data "
                                      "parallel (world > 1)")
        self.policy.freeze(self.freeze_policy_head, self.freeze_value_head, self.freeze_backbone)
        try:
            mask = [not p.requires_grad for p in self.flat.params]
            if all(mask):
                raise ValueError("every parameter is frozen (freeze_policy_head, freeze_value_head and "
                                 "freeze_backbone): nothing to train")
            opt.set_frozen(mask)
            before = opt.step_count
            try:
                return self._update(r)
            finally:  # also when the update raised part-way: the steps it did take are accounted for
                opt.account(opt.step_count - before)
        finally:
            self.policy.unfreeze()
            opt.set_frozen([False] * len(self.flat.params))

    def _update(self, r) -> Tuple[np.ndarray, np.ndarray, int]:
        self.last_update_rollout = r
        self._teacher_stats = None
        if self.dp_enabled and self.dp_update_mode == "replicated":
            # data parallel by replication: the whole env group's rollout on every rank, then the
            # single-process update (no exchange inside it); the ranks' weights are checked equal after
            g = self._replicated_rollout(r)
            self.last_update_rollout = g
            self.dp_enabled = False
            try:
                out = self._update(g)
            finally:
                self.dp_enabled = True
                self.last_update_rollout = g
            if self.world > 1 and not self._params_agree():
                raise RuntimeError("ranks' parameters diverged under the replicated data-parallel update")
            return out
        # a whole-epoch kernel (ppo_epoch.py) where one covers the policy, the options and the rollout
        spec = self.fused_mlp_spec() if hasattr(r, "epoch_batch") and not self._fused_kernels_off(r) else None
        if spec is not None:
            return self._update_fused_dp(r, spec) if self.dp_enabled else self._update_fused(r, spec)
        wide_epoch = self._wide_epoch_step(r)
        if wide_epoch is not None:
            if self.dp_enabled:
                return self._update_wide_epoch_xdp(r, wide_epoch)
            return self._update_wide_epoch(r, wide_epoch)
        nmb = r.num_minibatches(self.batch_size)
        n_steps = self.n_epochs * nmb
        n_norms = self.n_epochs if self.gradient_accumulation else n_steps
        blocks = self.blocks
        blocks.ensure_tables(n_steps, n_norms)
        K = None
        self.flat.check_views()
        if (self.use_graphs and self.flat.flat.is_cuda and hasattr(r, "_flat_fields")
                and r.logprobs is not None and not (self.dp_enabled and self.world > 1
                                                    and torch.distributed.get_backend(self.dp_group) != "nccl")):
            K = self._update_graphed(r, nmb)
            return self._read_tables(n_steps, n_norms, K, teacher=self._teacher_field(r, self._wide_step()) is not None)
        wide = self._wide_step()
        teacher = self._teacher_field(r, wide) is not None
        shuffle = not self.gradient_accumulation
        ext = None
        for e in range(self.n_epochs):
            if hasattr(r, "epoch_batch"):  # DeviceRollout: the epoch's permuted copy, sliced
                full = r.epoch_batch(shuffle)
                mbs = [r._batch_from([full.obs, full.actions, full.values, full.advantages, full.returns]
                                     + ([full.logprobs] if full.logprobs is not None else [])
                                     + ([full.action_masks] if full.action_masks is not None else [])
                                     + list(full.additional.values()),
                                     slice(i, i + self.batch_size)) for i in range(0, r.total_steps, self.batch_size)]
            else:
                full, mbs = None, r.minibatches(self.batch_size, shuffle=shuffle)
            for mb in mbs:
                if K is None:
                    with torch.no_grad():  # K (value columns) before the device blocks are written
                        K = value_columns(self.policy(mb.obs[:1], mb.actions[:1], action_masks=(
                            mb.action_masks[:1] if mb.action_masks is not None else None))[2])
                    ext = self._dp_moments_table(K, n_steps)
                    hp = self._hparams(K, nmb)
                    hp.ext_moments = ext.data_ptr() if ext is not None else None
                    blocks.upload(hp, self.optimizer.step_count, self._teacher_block() if teacher else None)
                    if ext is not None and full is not None:
                        self._fill_epoch_moments(ext, e, full.advantages, nmb)
                elif ext is not None and mb is mbs[0] and full is not None:
                    self._fill_epoch_moments(ext, e, full.advantages, nmb)
                if mb.logprobs is None:
                    raise ValueError("PPO needs rollout logprobs (include_logp=True)")
                self._minibatch_loss_grads(wide, mb.obs, mb.actions, mb.action_masks, mb.values, mb.advantages,
                                           mb.returns, mb.logprobs, [K],
                                           teacher_logp=mb.additional["teacher_logprobs"] if teacher else None)
                if not self.gradient_accumulation:
                    if self.dp_enabled:
                        self._all_reduce(self.flat.grad, average=True)
                    self.optimizer.step(blocks.state, blocks.norms)
            if self.gradient_accumulation:
                if self.dp_enabled:
                    self._all_reduce(self.flat.grad, average=True)
                self.optimizer.step(blocks.state, blocks.norms)
        return self._read_tables(n_steps, n_norms, K, teacher=teacher)

    def _read_tables(self, n_steps: int, n_norms: int, K: Optional[int] = None, teacher: bool = False,
                     what: Optional[str] = None, agree: bool = False) -> Tuple[np.ndarray, np.ndarray, int]:
        """The update's one D2H copy: the stats rows (under data parallel every rank holds its share:
        averaged over the ranks, summed after a whole-epoch kernel) and the gradient norms.
        teacher: the update launched rai_ppo_loss_teacher; its table comes back in the same copy.
        what: the update ran a whole-epoch kernel (named in the error); the train-state block comes back
        too, a set err flag (word 5) raises, and the value term the kernel left out of the loss column is
        added.  agree: the in-kernel cross-GPU exchange ran; the ranks' weights are checked equal."""
        blocks = self.blocks
        stats_t = blocks.stats[:n_steps]
        if self.dp_enabled:
            stats_t = stats_t.clone()
            self._all_reduce(stats_t, average=what is None)
        parts = [stats_t.reshape(-1), blocks.norms[:n_norms]]
        if teacher:
            parts.append(blocks.teacher_stats[:n_steps])
        if what is not None:
            parts.append(blocks.state.view(torch.float32))
        host = torch.cat(parts).cpu().numpy()
        n_s = n_steps * _lib.RAI_STAT_STRIDE
        stats, norms = host[:n_s].reshape(n_steps, _lib.RAI_STAT_STRIDE), host[n_s:n_s + n_norms]
        rest = host[n_s + n_norms:]  # the teacher table or the train state: no whole-epoch kernel has the term
        if teacher and self._teacher_on():
            self._teacher_stats = rest
        if what is not None:
            if rest.view(np.int32)[5] != 0:
                raise RuntimeError(f"{what} timed out (err flag set)")
            if agree and not self._params_agree():
                raise RuntimeError("ranks' parameters diverged after the in-kernel cross-GPU exchange")
            stats = stats.copy()
            stats[:, 0] += float(self.vf_coef) * stats[:, 5]
        return stats, norms, K or 1

    def _update_graphed(self, r, nmb: int) -> int:
        """The generic update with the minibatch step replayed from a hipGraph (graphs.py).
        Same minibatches, same kernels, same order as the eager loop above."""
        from .graphs import GraphedUpdate

        if self._graphed is None:
            self._graphed = GraphedUpdate(self.device)
        gu = self._graphed
        blocks = self.blocks
        fields = r._flat_fields()
        shuffle = not self.gradient_accumulation
        n = r.total_steps
        B = min(self.batch_size, n)
        n_full, tail = n // B, n % B
        # data parallel over our RCCL communicator: the gradient all-reduce is bucketed, overlapped
        # with the backward on a side stream and captured with the step (dp_buckets.py)
        buckets = self._grad_buckets() if not self.gradient_accumulation else None
        optim_in_step = not self.gradient_accumulation and (not self.dp_enabled or buckets is not None)
        has_masks = r.action_masks is not None
        K_box = [None]

        wide = self._wide_step()
        # the step's fields: the Batch fields and, with a teacher, its log-probabilities as the last one
        teacher = self._teacher_field(r, wide)
        fields = fields[:len(fields) - len(getattr(r, "additional", {}))] + ([teacher] if teacher is not None else [])
        # NatureCNN on uint8 frames: the gather emits obs.float() / range_size in channels_last
        xf = getattr(self.policy, "obs_transform", lambda o: None)(fields[0]) if wide is None else None
        xforms = [xf] + [None] * (len(fields) - 1) if xf is not None else None

        def step(bufs):
            obs, actions, values, adv, ret, logprobs = bufs[:6]
            masks = bufs[6] if has_masks else None
            if buckets is not None:
                buckets.begin()
            self._minibatch_loss_grads(wide, obs, actions, masks, values, adv, ret, logprobs, K_box,
                                       obs_prepared=xforms is not None,
                                       teacher_logp=bufs[-1] if teacher is not None else None)
            if buckets is not None:
                buckets.finish(scale=1.0 / self.world)
            if optim_in_step:
                self.optimizer.step(blocks.state, blocks.norms, count=False)

        # K (value columns) before the device blocks are written: one forward of one row
        with torch.no_grad():
            _, _, v0 = self.policy(fields[0][:1], fields[1][:1],
                                   action_masks=fields[6][:1] if has_masks else None)
        K = value_columns(v0)
        K_box[0] = K
        ext = self._dp_moments_table(K, self.n_epochs * nmb)
        hp = self._hparams(K, nmb)
        hp.ext_moments = ext.data_ptr() if ext is not None else None
        blocks.upload(hp, self.optimizer.step_count, self._teacher_block() if teacher is not None else None)
        # a graph bakes in every device pointer it touches: key it on the ones that can change
        tag = (optim_in_step, wide is not None, buckets is not None, blocks.stats.data_ptr(), blocks.norms.data_ptr(), blocks.hp.data_ptr(),
               blocks.state.data_ptr(), self.flat.flat.data_ptr(), self.flat.grad.data_ptr(),
               self.optimizer.hp_dev.data_ptr(),
               # the captured autograd work differs with requires_grad; the optimizer call bakes in its form,
               # the table's pointer and its length (the host rewrites the entries between updates)
               tuple(bool(f) for f in self.optimizer.frozen), self.optimizer._n_runs,
               self.optimizer.runs_dev.data_ptr())
        if teacher is not None:
            tag += (blocks.teacher.data_ptr(), blocks.teacher_stats.data_ptr())
        g = gu.graph_for(fields, B, tag, xforms)
        cur = torch.cuda.current_stream(self.device)
        gu.stream.wait_stream(cur)
        with torch.cuda.stream(gu.stream):
            gu.set_rollout(fields, B, shuffle)
            for e in range(self.n_epochs):
                perm = r.permutation() if shuffle else None
                if ext is not None:
                    self._fill_epoch_moments(ext, e, fields[3][perm] if perm is not None else fields[3], nmb)
                gu.start_epoch(perm)
                for _ in range(n_full):
                    g.run(gu.desc, gu.stream, step)
                    if not optim_in_step and not self.gradient_accumulation:
                        self._all_reduce(self.flat.grad, average=True)
                        self.optimizer.step(blocks.state, blocks.norms)
                if tail:
                    gu.tail(fields, tail, step, xforms)
                    if not optim_in_step and not self.gradient_accumulation:
                        self._all_reduce(self.flat.grad, average=True)
                        self.optimizer.step(blocks.state, blocks.norms)
                if self.gradient_accumulation:
                    if self.dp_enabled:
                        self._all_reduce(self.flat.grad, average=True)
                    self.optimizer.step(blocks.state, blocks.norms)
        cur.wait_stream(gu.stream)
        if optim_in_step:  # replays stepped the optimizer on device; keep the host count in sync
            self.optimizer.step_count += self.n_epochs * (n_full + (1 if tail else 0))
        return K

    def _train_stats(self, stats: np.ndarray, norms: np.ndarray, K: int, nmb: int, explained_var: float):
        last = stats[-nmb:].astype(np.float64)  # only the last epoch's stats are kept (ppo.py:288-289)
        vl = last[:, 5:5 + K]
        vc = last[:, 5 + _lib.RAI_MAX_K:5 + _lib.RAI_MAX_K + K]
        if self.vf_weights is not None:
            w = np.asarray(self.vf_weights, np.float64)
            v_loss = float(np.mean(vl @ w))
        else:
            v_loss = np.mean(vl, axis=0)
            v_loss = float(v_loss[0]) if K == 1 else v_loss
        val_clipped = np.mean(vc, axis=0)
        last_norms = norms[-1:] if self.gradient_accumulation else norms[-nmb:]
        return TrainStats(
            loss=float(last[:, 0].mean()), pi_loss=float(last[:, 1].mean()), v_loss=v_loss,
            entropy_loss=float(last[:, 2].mean()), approx_kl=float(last[:, 3].mean()),
            clipped_frac=float(last[:, 4].mean()),
            val_clipped_frac=float(val_clipped[0]) if K == 1 else val_clipped,
            additional_losses=({"teacher_kl_loss": float(np.mean(self._teacher_stats[-nmb:].astype(np.float64)))}
                               if self._teacher_stats is not None else {}),
            explained_var=explained_var, grad_norm=float(np.mean(last_norms)))

    def save(self, path: str) -> None:
        save_optimizer(self.optimizer, path)

    def load(self, path: str) -> None:
        load_optimizer(self.optimizer, path, self.device, per_parameter_steps=True)
