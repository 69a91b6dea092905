"""PPO's data-parallel set-up (one process per GPU): the batch rule and update mode, the IPC regions of
the in-kernel cross-GPU exchange, the RCCL communicator of our own, the replicated rollout, the global
advantage moments and the bucketed gradient all-reduce.  A base class of PPO (ppo.py), whose constructor
sets the attributes used here; the updates that run over it are in ppo.py and ppo_epoch.py."""
from __future__ import annotations

import ctypes as C
import logging
import os
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib


class PPODataParallel:
    _xdp: Optional[dict] = None  # the in-kernel exchange's regions (_setup_xdp)

    def enable_data_parallel(self, group=None, native_dp: bool = True, xdp: Optional[bool] = None,
                             dp_batch: str = "global", update_mode: Optional[str] = None) -> None:
        """Data parallelism: every rank owns its own env group and HBM rollout; a global
        minibatch is the union of the ranks' minibatch slices, gradients are summed over ranks
        with one all-reduce per optimizer step (RCCL over xGMI via torch.distributed, or the
        in-kernel exchange), and every rank applies the identical clip+Adam step.  The
        advantage normalisation uses global per-minibatch moments (one small all-reduce per
        epoch), reproducing the reference's normalisation over the whole (global) minibatch:
        on the fused MLP path through the kernels' moments argument, on the per-minibatch path
        through rai_ppo_hparams.ext_moments (per advantage column, or of the weighted advantage
        under normalize_advantages_after_scaling).

        dp_batch: "per-rank" — each rank takes batch_size rows per optimizer step (global
        minibatch batch_size x world); "global" — SURVEY.md 8(e)'s rule: batch_size / world rows
        per rank, so the global minibatch is batch_size (rl_algo_impls/ppo/ppo.py:314,
        rollout/vec_rollout.py:108-111) and the update equals the single-process one over the
        ranks' interleaved rollouts.

        update_mode: "exchange" — every optimizer step sums the ranks' gradients (in-kernel over the
        IPC-mapped regions, native RCCL loop, bucketed all-reduce or the Python loop, in that order of
        preference); "replicated" (dp_batch "global" only) — each rank steps its own env group, ONE
        all-gather per update assembles the rollout of the whole env group (GAE is per env column, so
        the local advantages / returns concatenate), and every rank runs the identical single-process
        update over it: bitwise the single-process update, with no cross-rank traffic inside the
        dependent optimizer-step chain; "auto" (default; RAI_DP_UPDATE overrides) — replicated where
        the update is a dependent chain of one-launch-per-epoch steps (the fused CartPole-class epoch
        kernel at <= 256 rows, the wide whole-epoch kernel), whose per-step cross-GPU hop costs more
        than the rows it spreads, exchange otherwise."""
        self.dp_group = group
        self.dp_enabled = True
        self.world = dist.get_world_size(group)
        if dp_batch not in ("per-rank", "global"):
            raise ValueError(f"dp_batch must be 'per-rank' or 'global', not {dp_batch!r}")
        self.dp_batch = dp_batch
        # idempotent: derived from the YAML batch_size every call, never from a previous division
        yaml_bs = self._yaml_batch_size
        self.batch_size = yaml_bs
        self.global_batch_size = yaml_bs * self.world
        if dp_batch == "global":
            if yaml_bs % self.world:
                raise ValueError(f"dp_batch='global': batch_size {yaml_bs} is not divisible by the "
                                 f"world size {self.world}")
            self.global_batch_size = yaml_bs
            self.batch_size = yaml_bs // self.world
        self._dp_comm = None
        self._xdp = None
        # the bucketed all-reduce closes over the communicator, and the captured minibatch-step
        # graphs over the buckets: both are rebuilt against the new communicator
        self._buckets = None
        self._graphed = None
        if update_mode is None:
            update_mode = os.environ.get("RAI_DP_UPDATE", "auto")
        if update_mode not in ("auto", "exchange", "replicated"):
            raise ValueError(f"update_mode must be 'auto', 'exchange' or 'replicated', not {update_mode!r}")
        if update_mode == "replicated" and dp_batch != "global":
            raise ValueError("update_mode='replicated' runs the single-process update over the whole env "
                             "group: it needs dp_batch='global'")
        self.dp_update_mode = "exchange"
        if update_mode != "exchange" and dp_batch == "global":
            self.batch_size = yaml_bs  # the single-process minibatch, for the path check below
            if update_mode == "replicated" or (self.world > 1 and self.flat.flat.is_cuda
                                               and self._dependent_chain_update()):
                self.dp_update_mode = "replicated"
            else:
                self.batch_size = yaml_bs // self.world
        if self.dp_update_mode == "replicated":
            self._broadcast_params(group)
            return
        if xdp is None:
            xdp = os.environ.get("RAI_XDP", "1") != "0"
        spec = self.fused_mlp_spec()
        # the CartPole-class fused epoch kernel (<= 256 rows per rank) and the large-minibatch steps (batch
        # policy (b): the exchange inside each step's reduce launch, mlp_large.hip)
        c2_xdp = (spec is not None and spec["in_dim"] <= 4
                  and (spec["n_act"] <= 2 if self.batch_size <= _lib.RAI_MLP_EPOCH_MAX_B else spec["n_act"] == 2))
        # the wide whole-epoch kernel (C4) keeps its one launch per epoch under data parallel too
        wide_xdp = spec is None and self._wide_epoch_options_ok() and self._wide_step() is not None
        if xdp and self.flat.flat.is_cuda and self.world > 1 and self.world <= 8 and (c2_xdp or wide_xdp):
            try:
                self._xdp = self._setup_xdp(group)
            except RuntimeError as e:  # e.g. IPC unavailable: fall back to the per-step RCCL loop
                logging.warning(f"in-kernel cross-GPU exchange unavailable ({e}); using the RCCL loop")
                self._xdp = None
        if self._xdp is None and self.flat.flat.is_cuda and dist.get_backend(group) == "nccl" and native_dp:
            self._dp_comm = self._native_comm(group)
        self._broadcast_params(group)

    def _broadcast_params(self, group) -> None:
        """Identical starting weights on every rank (rank 0's)."""
        with torch.no_grad():
            src = dist.get_global_rank(group, 0) if group is not None else 0
            if self.flat.flat.is_cuda and dist.get_backend(group) == "gloo":
                h = self.flat.flat.cpu()
                dist.broadcast(h, src=src, group=group)
                self.flat.flat.copy_(h)
            else:
                dist.broadcast(self.flat.flat, src=src, group=group)

    def _dependent_chain_update(self) -> bool:
        """True when this trainer's single-process update is a chain of one-launch-per-epoch dependent
        optimizer steps (rai_mlp_ppo_epoch's fused kernel at <= 256 rows, rai_mlp_wide_epoch): there a
        per-step cross-GPU exchange adds its hop to every step and shrinks nothing the step waits on."""
        spec = self.fused_mlp_spec()
        if spec is not None:
            return self.batch_size <= _lib.RAI_MLP_EPOCH_MAX_B
        return self._wide_epoch_options_ok() and self._wide_step() is not None

    def _replicated_rollout(self, r):
        """The rollout of the whole env group from every rank's own (T, N/R, ...) rollout: one all-gather
        per field (RCCL over xGMI; gloo through host memory), rank r's envs as columns [r N/R, (r+1) N/R).
        The epoch permutations must agree on every rank: a perm_source the caller injected is used as
        is, otherwise the shuffle keys derive from rank 0's next key (one 8-byte broadcast)."""
        from .rollout import DeviceRollout

        g, W = self.dp_group, self.world
        gloo = dist.get_backend(g) == "gloo"

        def gather(t):
            if t is None:
                return None
            src = t.contiguous()
            if gloo:
                h = src.cpu()
                parts = [torch.empty_like(h) for _ in range(W)]
                dist.all_gather(parts, h, group=g)
                out = torch.stack(parts).to(src.device)
            else:
                out = torch.empty((W,) + tuple(src.shape), dtype=src.dtype, device=src.device)
                dist.all_gather_into_tensor(out, src, group=g)
            return out.transpose(0, 1).reshape((src.shape[0], W * src.shape[1]) + tuple(src.shape[2:]))

        keys = None
        if r._perm_source is None:
            k = torch.tensor([r._perm_keys() if r._perm_keys is not None else 0], dtype=torch.int64)
            if not gloo:
                k = k.to(self.device)
            dist.broadcast(k, src=dist.get_global_rank(g, 0) if g is not None else 0, group=g)
            k0, count = int(k.item()), [0]

            def keys():
                count[0] += 1
                return (k0 * 0x9E3779B97F4A7C15 + count[0]) & (2**63 - 1)

        return DeviceRollout.from_fields(
            self.device, gather(r.obs), gather(r.actions), gather(r.values), gather(r.advantages),
            gather(r.returns), gather(r.logprobs), gather(r.action_masks), gather(r.num_actions),
            perm_keys=keys, perm_source=r._perm_source)

    def _setup_xdp(self, group) -> dict:
        """Exchange regions for the in-kernel cross-GPU all-reduce (rai_mlp_ppo_epoch_xdp): one
        uncached device region per rank, shared by IPC handle over `group`, mapped by every rank."""
        L = _lib.lib()
        rank = dist.get_rank(group)

        def agreed(ok: bool) -> bool:
            # every rank learns whether every rank's local step succeeded, so a failure on one rank
            # turns into the same RuntimeError (and the RCCL-loop fallback) on all of them instead
            # of leaving the others blocked in the next collective
            f = torch.tensor([0 if ok else 1], dtype=torch.int64, device=self.device)
            if dist.get_backend(group) == "gloo":
                f = f.cpu()
            dist.all_reduce(f, op=dist.ReduceOp.MAX, group=group)
            return int(f.item()) == 0

        nbytes = int(L.rai_xdp_region_bytes(self.world))
        region = C.c_void_p()
        torch.cuda.synchronize(self.device)
        hb = int(L.rai_xdp_handle_bytes())
        hbuf = (C.c_uint8 * hb)()
        ok = L.rai_xdp_alloc(nbytes, C.byref(region)) == 0 and L.rai_xdp_handle(region, hbuf, hb) == 0
        handles = [None] * self.world
        dist.all_gather_object(handles, bytes(hbuf) if ok else b"", group=group)

        def release(opened):
            for p in opened:
                L.rai_xdp_close(p)
            if region.value:
                L.rai_xdp_free(region)

        if not all(handles):
            release([])
            raise RuntimeError("cross-GPU exchange: region allocation / IPC export failed on some rank")
        ptrs, opened = [], []
        for r, h in enumerate(handles):
            if r == rank:
                ptrs.append(region.value)
                continue
            peer = C.c_void_p()
            if L.rai_xdp_open(h, C.byref(peer)) != 0:
                ok = False
                break
            opened.append(peer)
            ptrs.append(peer.value)
        if not agreed(ok):
            release(opened)
            raise RuntimeError("cross-GPU exchange: IPC mapping of a peer region failed on some rank")
        peers = torch.tensor(ptrs, dtype=torch.int64, device=self.device)
        torch.cuda.synchronize(self.device)
        dist.barrier(group=group)  # every region zeroed and mapped before any kernel pushes into it
        # canary: the epoch kernel's memory, scopes and flag protocol on a known payload, on every rank
        bad = torch.zeros(2, dtype=torch.int32, device=self.device)
        if os.environ.get("RAI_XDP_INJECT_FAIL_RANK", "") == str(rank):
            rc = -1  # test hook: this rank's canary "fails" without launching (its partners time out)
        else:
            rc = L.rai_xdp_selftest(peers.data_ptr(), self.world, rank, 1, bad.data_ptr(),
                                    _lib.stream_handle(self.device))
        torch.cuda.synchronize(self.device)
        verdict = bad.to(torch.int64)
        if rc != 0:  # a launch failure joins the verdict instead of raising on this rank alone
            verdict[0] += 1
        if dist.get_backend(group) == "gloo":
            verdict = verdict.cpu()
        dist.all_reduce(verdict, op=dist.ReduceOp.MAX, group=group)
        if int(verdict.sum()) != 0:
            release(opened)
            raise RuntimeError(f"cross-GPU exchange self-test failed (wrong values, timeouts) = {verdict.tolist()}")
        return dict(region=region, opened=opened, peers=peers, rank=rank, step=0)

    def _params_agree(self) -> bool:
        """Cheap cross-rank consistency check of the (bitwise-identical by construction) weights."""
        v = self.flat.flat.double()
        t = torch.stack([v.sum(), (v * v).sum(), -v.sum(), -(v * v).sum()])
        if dist.get_backend(self.dp_group) == "gloo":
            t = t.cpu()
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.dp_group)
        return bool((t[0] == -t[2]) and (t[1] == -t[3]))

    def _native_comm(self, group):
        """An RCCL communicator of our own (same ranks as `group`) for the natively driven
        per-minibatch loop (rai_mlp_ppo_epoch_dp); the unique id travels over `group`."""
        L = _lib.lib()
        if not L.rai_dp_available():
            raise RuntimeError("librccl.so.1 is not mapped in this process: native data parallelism unavailable")
        uid = torch.zeros(_lib.RAI_DP_UID_BYTES, dtype=torch.uint8)
        if dist.get_rank(group) == 0:
            buf = (C.c_uint8 * _lib.RAI_DP_UID_BYTES)()
            _lib.check(L.rai_dp_unique_id(buf, _lib.RAI_DP_UID_BYTES), "rai_dp_unique_id")
            uid.copy_(torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8))
        dev_uid = uid.to(self.device)
        dist.broadcast(dev_uid, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = bytes(dev_uid.cpu().numpy().tobytes())
        comm = C.c_void_p()
        torch.cuda.synchronize(self.device)
        _lib.check(L.rai_dp_comm_init(C.byref(comm), raw, self.world, dist.get_rank(group)), "rai_dp_comm_init")
        return comm

    def _all_reduce(self, t: torch.Tensor, average: bool = False) -> None:
        if t.is_cuda and dist.get_backend(self.dp_group) == "gloo":  # test/rehearsal backend
            h = t.cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.dp_group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.dp_group)  # RCCL over xGMI
        if average:
            t.mul_(1.0 / self.world)

    def _global_adv_moments(self, adv: torch.Tensor, nmb: int) -> torch.Tensor:
        """(mean, den) of every global minibatch of this epoch, per advantage column (or of the
        multi_reward_weights-weighted advantage under normalize_advantages_after_scaling):
        local per-minibatch (count, sum, sum of squares) in fp64, one all-reduce, unbiased std
        (ppo.py:307-318).  Returns (nmb, columns, 2) f32; the loss kernel applies the
        normalize / standardize rule itself."""
        B = self.batch_size
        a = adv.double()
        a = a.reshape(a.shape[0], -1)
        if self.normalize_advantages_after_scaling:
            w = self.multi_reward_weights
            if w is not None:
                a = (a.float() * torch.as_tensor(np.asarray(w, np.float32), device=a.device)).sum(1, keepdim=True)
                a = a.double()
            else:
                a = a[:, :1]
        rows, kc = a.shape
        n_full = rows // B
        full = a[:n_full * B].view(n_full, B, kc)
        parts = [torch.stack([torch.full((n_full, kc), float(B), dtype=torch.float64, device=a.device),
                              full.sum(1), (full ** 2).sum(1)], -1)]
        if n_full < nmb:
            tail = a[n_full * B:]
            parts.append(torch.stack([torch.full((kc,), float(tail.shape[0]), dtype=torch.float64, device=a.device),
                                      tail.sum(0), (tail ** 2).sum(0)], -1).view(1, kc, 3))
        m = torch.cat(parts, 0)
        self._all_reduce(m)
        n, s1, s2 = m[..., 0], m[..., 1], m[..., 2]
        mean = s1 / n
        std = torch.sqrt(torch.clamp(s2 - n * mean * mean, min=0.0) / (n - 1)).float()
        out = torch.empty((nmb, kc, 2), dtype=torch.float32, device=a.device)
        out[..., 0] = mean.float()
        out[..., 1] = std + 1e-8
        return out.contiguous()

    def _dp_moments_table(self, K: int, n_steps: int) -> Optional[torch.Tensor]:
        """Data parallel on the per-minibatch path: the global minibatches' advantage (mean, den),
        one row per stats row, for the loss kernel (rai_ppo_hparams.ext_moments); None when the
        minibatch's own moments are the reference's (single rank) or no normalisation is asked for.
        Layout (n_steps, columns, 2): K columns, or one under normalize_advantages_after_scaling."""
        if not self.dp_enabled or self.world == 1:
            return None
        if self.normalize_advantages_after_scaling:
            return torch.zeros((n_steps, 1, 2), dtype=torch.float32, device=self.device)
        if not (self.normalize_advantage or self.standardize_advantage):
            return None
        return torch.zeros((n_steps, K, 2), dtype=torch.float32, device=self.device)

    def _fill_epoch_moments(self, ext: torch.Tensor, epoch: int, adv_epoch: torch.Tensor, nmb: int) -> None:
        """Rows [epoch*nmb, (epoch+1)*nmb) of the table from this rank's permuted advantages (one
        small all-reduce; stream-ordered before the epoch's loss launches)."""
        ext[epoch * nmb:(epoch + 1) * nmb].copy_(self._global_adv_moments(adv_epoch, nmb))

    def _grad_buckets(self):
        """GradBuckets for the bucketed, backward-overlapped all-reduce (dp_buckets.py) when data
        parallel runs over our own RCCL communicator and the policy has a bucket layout (NatureCNN),
        else None (one all-reduce of the whole flat gradient after the step).  RAI_DP_BUCKETS=0: off."""
        if not self.dp_enabled or self._dp_comm is None or os.environ.get("RAI_DP_BUCKETS", "1") == "0":
            return None
        if self._buckets is not None:
            return self._buckets
        from .dp_buckets import GradBuckets, nature_cnn_buckets

        layout = nature_cnn_buckets(self.policy, self.flat)
        if layout is None:
            return None
        bounds, triggers = layout
        L, comm, dev = _lib.lib(), self._dp_comm, self.device

        def allreduce(v: torch.Tensor) -> None:
            _lib.check(L.rai_dp_allreduce_sum_f32(comm, v.data_ptr(), v.numel(), _lib.stream_handle(dev)),
                       "rai_dp_allreduce_sum_f32")

        self._buckets = GradBuckets(self.flat, bounds, triggers, allreduce, dev)
        return self._buckets
