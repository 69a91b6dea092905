"""The reference-AI rollout generator (rollout_type: reference; rl_algo_impls/rollout/reference_ai_rollout.py):
the env's scripted bot plays, and the batch's actions are the BOT's (vec_env.last_action), which is what
ACBC clones.  Every ACBC configuration of the reference (acbc-Microrts.yml, acbc-LuxAI_S2.yml) sets it.

The one new piece of hot path per env step is taking the bot's actions onto the device: the env hands over
int32 (N, cells, planes) arrays, the rollout buffers hold int64, and the update kernels index a row's logits
by these values.  `store` (rai_ref_actions_store, csrc/ref_actions.hip) widens, sanitises and counts in one
launch; `store_host` is the same function in numpy, the CPU path's.

Two stated deviations from the reference:
  * include_logp=True: the reference rebinds self.logprobs to the step's own tensor every step
    (reference_ai_rollout.py:53-58), so its rollout carries the LAST step's log-probs only; here they are
    written into slot s like the sync generator's, and the rollout carries all T.
  * a recorded action outside [0, nvec[g]) is stored as 0 and counted, a recorded action its mask forbids is
    stored as it is and counted (invalid_actions, invalid_action_count, one warning per rollout); the
    reference stores whatever the env hands over.
"""
from __future__ import annotations

import logging
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .envs import is_box
from .md_ops import nvec_array
from .rollout import DeviceRollout, SyncStepRolloutGenerator, _pinned


def store_host(src: np.ndarray, nvec: Sequence[int], mask: Optional[np.ndarray], cells: int
               ) -> Tuple[np.ndarray, np.ndarray]:
    """rai_ref_actions_store in numpy.  src: R * G integers (R = N * cells rows), mask: R * A bools or None.
    Returns (dst int64 (R, G), bad int32 (N,))."""
    nv = np.asarray(nvec, dtype=np.int64)
    G = len(nv)
    a = np.asarray(src).reshape(-1, G)
    assert a.dtype.kind in "iu", f"integer actions expected, got {a.dtype}"
    if a.dtype.kind == "u" and a.dtype.itemsize == 8:
        a = np.where(a > np.uint64(2**63 - 1), -1, a.astype(np.int64))  # beyond int64: out of range
    a = a.astype(np.int64)
    R = a.shape[0]
    assert cells >= 1 and R % cells == 0
    oor = (a < 0) | (a >= nv[None, :])
    dst = np.where(oor, 0, a)
    counted = oor.copy()
    if mask is not None:
        m = np.asarray(mask).reshape(R, int(nv.sum())) != 0
        off = np.concatenate([[0], np.cumsum(nv)])
        for g in range(G):
            mg = m[:, off[g]:off[g + 1]]
            picked = np.take_along_axis(mg, dst[:, g:g + 1], axis=1)[:, 0]
            counted[:, g] |= ~oor[:, g] & mg.any(axis=1) & ~picked
    bad = counted.reshape(R // cells, cells * G).sum(axis=1).astype(np.int32)
    return dst, bad


def store(src: torch.Tensor, nvec: Sequence[int], mask: Optional[torch.Tensor], cells: int, dst: torch.Tensor,
          bad: torch.Tensor) -> None:
    """One launch of rai_ref_actions_store: src (int32 or int64, N * cells * G elements) on the device into
    dst (int64, a slot of the action buffer) and bad (int32 (N,))."""
    _lib.require_device(src, mask, dst, bad)
    assert src.is_contiguous() and dst.is_contiguous() and bad.is_contiguous()
    assert dst.dtype == torch.int64 and bad.dtype == torch.int32 and src.numel() == dst.numel()
    code = {torch.int32: _lib.RAI_REF_ACT_I32, torch.int64: _lib.RAI_REF_ACT_I64}[src.dtype]
    G = len(nvec)
    N = int(bad.shape[0])
    assert src.numel() == N * cells * G
    m = None
    if mask is not None:
        assert mask.is_contiguous() and mask.numel() == N * cells * sum(int(n) for n in nvec)
        m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        assert m.dtype == torch.uint8
    rc = _lib.lib().rai_ref_actions_store(src.data_ptr(), code, nvec_array(nvec), G, _lib.ptr(m), N, cells,
                                          dst.data_ptr(), bad.data_ptr(), _lib.stream_handle(src.device))
    _lib.check(rc, "rai_ref_actions_store")


def _gae_host(rewards, values, episode_starts, next_episode_starts, next_values, gamma, gae_lambda) -> np.ndarray:
    """rl_algo_impls/shared/gae.py:97-124 in numpy (the CPU path; the device path is rai_gae)."""
    adv = np.zeros_like(rewards)
    last = 0
    T = adv.shape[0]
    col = lambda x: x.reshape((1,) * (values.ndim - 1 - x.ndim) + x.shape) if isinstance(x, np.ndarray) else x
    gamma, gae_lambda = col(gamma), col(gae_lambda)
    for t in reversed(range(T)):
        nonterminal = 1.0 - (next_episode_starts if t == T - 1 else episode_starts[t + 1])
        next_value = next_values if t == T - 1 else values[t + 1]
        nonterminal = nonterminal.reshape(nonterminal.shape + (1,) * (next_value.ndim - nonterminal.ndim))
        delta = rewards[t] + gamma * next_value * nonterminal - values[t]
        last = delta + gamma * gae_lambda * nonterminal * last
        adv[t] = last
    return adv


class ReferenceAIRolloutGenerator(SyncStepRolloutGenerator):
    """Device-resident ReferenceAIRolloutGenerator (reference_ai_rollout.py:19-97), same constructor kwargs as
    SyncStepRolloutGenerator.  Per env step:

      include_logp=False (every reference YAML): the policy's work is the value forward alone (network.value,
        graph-replayed like the other rollout forwards); nothing is sampled, no RNG offset is consumed, no
        action leaves the device, and the env receives a zero action of the action space's shape and dtype;
      include_logp=True: the sync generator's policy step unchanged; the sampled action goes to the env and
        log-probs and values into slot s (the reference keeps only the last step's log-probs: see the module
        docstring);
      then vec_env.last_action goes host -> device in its own dtype and ONE rai_ref_actions_store launch writes
      actions[s] and invalid_actions[s], under action_masks[s], the mask the bot acted under.

    After the rollout invalid_action_count (a Python int, one device read) is the sum of invalid_actions
    (T, N) int32; a non-zero count is logged as a warning.  It always takes the generic step loop, for
    CartPole-class policies too.  On the CPU the same class runs with store_host and a numpy GAE.
    Dict actions (Lux pick_position) and Box action spaces are refused, and so is data parallel: PPO raises
    at world > 1 for a generator whose data_parallel is False (the counts are not reduced over ranks).

    Ordering of the host staging buffers.  Every step writes ONE pinned buffer per field on the host (rewards,
    dones, observations, masks, the bot's actions) and queues an asynchronous copy from it.  The sync
    generator may reuse them because its per-step wait for the sampled actions drains the stream first;
    without log-probs there is no such wait, and a forward slower than the env would let the host overwrite
    a buffer that a queued copy has not read yet.  So _staged is recorded after a step's last copy, and the
    next step waits for it after vec_env.step returns and before its first host write: the forward still
    overlaps the env step, and no action leaves the device."""

    data_parallel = False

    def __init__(self, policy, vec_env, **kwargs) -> None:
        act_space = vec_env.single_action_space
        if isinstance(act_space, dict) or hasattr(act_space, "spaces"):
            raise NotImplementedError("dict action spaces (Lux pick_position) are outside the reference-AI "
                                      "generator's scope")
        if is_box(act_space):
            raise NotImplementedError("the reference-AI generator records integer actions: Box action spaces are "
                                      "outside its scope")
        super().__init__(policy, vec_env, **kwargs)
        self._mapped_loop = False
        self._host = self.device.type != "cuda"
        if self._host:
            self.fused_step = None  # the bootstrap values by network.value
        N, dev = self.num_envs, self.device
        if self.gridnet:
            self.ref_nvec = [int(n) for n in self.action_plane_space.nvec]
            self.ref_cells = int(self.act_shape[0])
        elif self.multidiscrete:
            self.ref_nvec, self.ref_cells = [int(n) for n in act_space.nvec], 1
        else:
            self.ref_nvec, self.ref_cells = [int(act_space.n)], 1
        if len(self.ref_nvec) > _lib.RAI_MD_MAX_G or sum(self.ref_nvec) > _lib.RAI_GRID_MAX_A:
            raise NotImplementedError(f"action planes {self.ref_nvec} are beyond rai_ref_actions_store's limits")
        self.invalid_actions = torch.zeros((self.n_steps, N), dtype=torch.int32, device=dev)
        self.invalid_action_count = 0
        self._ref_stage = None  # (pinned host, device) buffers of last_action's dtype, made at first use
        if not self.include_logp:
            dt = torch.from_numpy(np.zeros((), dtype=getattr(act_space, "dtype", np.int64))).dtype
            self._zero_action = _pinned(torch.zeros((N,) + self.act_shape, dtype=dt), dev)
        self._staged = None
        if not self._host:  # recorded after each step's last host -> device copy (the constructor's staging first)
            self._staged = torch.cuda.Event()
            self._staged.record()

    # -- the step's phases ---------------------------------------------------------------------
    def _value_step(self, s: int) -> None:
        v = self._policy_forward(self.policy.network.value)
        self.values[s].copy_(v.float().reshape(self.values[s].shape))

    def _policy_step(self, s: int) -> None:
        if not self._host:
            return super()._policy_step(s)
        # the CPU path: the policy's own numpy step (no sampler kernels there)
        masks = self.next_masks_dev.numpy() if self.action_masks is not None else None
        st = self.policy.step(self.next_obs_dev.numpy(), action_masks=masks)
        self.actions[s].copy_(torch.as_tensor(st.a).view(self.actions[s].shape))
        self.logprobs[s].copy_(torch.as_tensor(st.logp_a))
        self.values[s].copy_(torch.as_tensor(st.v).view(self.values[s].shape))

    def _last_action(self) -> np.ndarray:
        if not hasattr(self.vec_env, "last_action"):
            raise AttributeError(f"{type(self.vec_env).__name__} has no last_action: the reference-AI generator "
                                 "records the actions of the env's own scripted bot")
        a = self.vec_env.last_action
        if isinstance(a, dict) or (isinstance(a, np.ndarray) and a.dtype == object):
            raise NotImplementedError("dict last_action (Lux pick_position) is outside the reference-AI "
                                      "generator's scope")
        a = np.asarray(a)
        if a.dtype.kind not in "iu":
            raise NotImplementedError(f"last_action of dtype {a.dtype}: integer actions expected")
        if a.dtype not in (np.int32, np.int64):  # the narrower of the two that holds it (uint64 beyond int64
            a = a.astype(np.int32 if a.dtype.itemsize < 4 else np.int64)  # wraps negative: out of range)
        if a.size != self.actions[0].numel():
            raise ValueError(f"last_action {a.shape} does not match the action shape {tuple(self.actions[0].shape)}")
        return a

    def _record_bot_actions(self, s: int) -> None:
        """vec_env.last_action -> actions[s], invalid_actions[s] (reference_ai_rollout.py:69-70)."""
        a = self._last_action()
        mask = self.action_masks[s] if self.action_masks is not None else None
        if self._host:
            dst, bad = store_host(a, self.ref_nvec, None if mask is None else mask.numpy(), self.ref_cells)
            self.actions[s].copy_(torch.from_numpy(dst).view(self.actions[s].shape))
            self.invalid_actions[s].copy_(torch.from_numpy(bad))
            return
        dt = torch.from_numpy(a[:0]).dtype
        if self._ref_stage is None or self._ref_stage[0].dtype != dt:
            shape = tuple(self.actions[0].shape)
            self._ref_stage = (_pinned(torch.zeros(shape, dtype=dt), self.device),
                               torch.zeros(shape, dtype=dt, device=self.device))
        host, dev = self._ref_stage
        np.copyto(host.numpy(), a.reshape(host.shape))
        dev.copy_(host, non_blocking=True)
        store(dev, self.ref_nvec, mask, self.ref_cells, self.actions[s], self.invalid_actions[s])

    @torch.no_grad()
    def _rollout(self, output_next_values: bool) -> Optional[torch.Tensor]:
        self.policy.eval()
        h_rew, h_done = self.h_rew.numpy(), self.h_done.numpy()
        for s in range(self.n_steps):
            self._slot_copies(s)
            if self.include_logp:
                self._policy_step(s)
                step_actions = self._actions_to_host(s)
            else:
                self._value_step(s)
                step_actions = self._zero_action.numpy()
            obs, rew, term, trunc, info = self.vec_env.step(step_actions)
            if self._staged is not None:  # the copies queued from the staging buffers have read them
                self._staged.synchronize()
            self._take_env_results(rew, term, trunc, info, h_rew, h_done)
            self._results_to_device(s)
            self._record_bot_actions(s)
            self._stage_next(obs)
            if self._staged is not None:
                self._staged.record()
        next_values = self._finish_rollout(output_next_values)
        self.invalid_action_count = int(self.invalid_actions.sum().item())
        if self.invalid_action_count:
            logging.warning("reference-AI rollout: %d recorded action components were out of range or masked out",
                            self.invalid_action_count)
        return next_values

    def _actions_to_host(self, s: int) -> np.ndarray:
        if not self._host:
            return super()._actions_to_host(s)
        self.h_act.copy_(self._act_src[s])
        return self.h_act.numpy()

    def rollout(self, gamma, gae_lambda) -> DeviceRollout:
        if not self._host:
            return super().rollout(gamma, gae_lambda)
        if self.scale_advantage_by_values_accuracy:
            raise NotImplementedError("scale_advantage_by_values_accuracy on the CPU path")
        next_values = self._rollout(output_next_values=True)
        nes = self.next_episode_starts.clone()
        adv = torch.from_numpy(_gae_host(self.rewards.numpy(), self.values.numpy(), self.episode_starts.numpy(),
                                         nes.numpy(), next_values.numpy(), gamma, gae_lambda))
        r = DeviceRollout.from_fields(self.device, self.obs, self.actions, self.values, adv, adv + self.values,
                                      self.logprobs if self.include_logp else None, self.action_masks,
                                      perm_keys=self._perm_key, perm_source=self.perm_source)
        r.rewards, r.episode_starts, r.next_episode_starts, r.next_values = (self.rewards, self.episode_starts, nes,
                                                                             next_values)
        return r
