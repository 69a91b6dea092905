"""Replay buffer for DQN: a ring in HBM filled and sampled by HIP kernels (csrc/dqn.hip).

Drop-in for rl_algo_impls/rollout/replay_buffer_rollout_generator.py:29-84.  The reference keeps a
`deque(maxlen=buffer_size)` of per-transition tuples filled in a per-env Python loop and rebuilds every
batch with `random.sample` + `torch.as_tensor` over lists of arrays.  Here the five fields live in device
memory in the env's dtype, one env step is one pinned H2D (rai_copy_h2d_multi) + one rai_replay_push, and a
batch is one rai_replay_sample launch (keyed draw without replacement + gather into static buffers).  The
ring's head / len / draws live on the device, so both launches replay from a hipGraph unchanged.

On the CPU the same ring is torch tensors and the sampler is the same keyed bijection computed with numpy
(`feistel_positions`), so the logic is covered without a GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _lib

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


class Batch(NamedTuple):  # replay_buffer_rollout_generator.py:13-18
    obs: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    dones: torch.Tensor
    next_obs: torch.Tensor


def _mix32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def sample_key(seed: int, draws: int) -> int:
    """The 64-bit key of draw number `draws` (rai_replay_sample)."""
    return (seed + _GOLDEN * draws) & _M64


def feistel_positions(n: int, key: int, count: Optional[int] = None) -> np.ndarray:
    """The first `count` outputs of rai_feistel_permutation(n, key) (csrc/rollout.hip), on the host:
    distinct positions in [0, n)."""
    count = n if count is None else count
    assert 0 <= count <= n
    bits = max(2, int(n - 1).bit_length()) if n > 1 else 2
    h1 = bits // 2
    h2 = bits - h1
    m1, m2 = np.uint32((1 << h1) - 1), np.uint32((1 << h2) - 1)
    lo_k, hi_k = np.uint32(key & 0xFFFFFFFF), np.uint32((key >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        ks = [_mix32(np.array([lo_k]) ^ _mix32(np.array([hi_k]) + np.uint32(0x9E3779B9) * np.uint32(r + 1)))[0]
              for r in range(6)]
        x = np.arange(count, dtype=np.uint64)
        todo = np.ones(count, dtype=bool)
        while todo.any():
            xs = x[todo]
            hi = (xs >> np.uint64(h2)).astype(np.uint32)
            lo = xs.astype(np.uint32) & m2
            for r in range(0, 6, 2):
                t = hi ^ (_mix32(lo ^ ks[r]) & m1)
                hi, lo = lo, t
                u = hi ^ (_mix32(lo ^ ks[r + 1]) & m2)
                hi, lo = lo, u
            x[todo] = (hi.astype(np.uint64) << np.uint64(h2)) | lo.astype(np.uint64)
            todo = x >= np.uint64(n)
    return x.astype(np.int64)


class ReplayRing:
    """The five-field ring.  `len(ring)` is the number of live transitions (host mirror of the device's
    `len`); positions are in deque order (0 = oldest), slots are ring rows."""

    def __init__(self, capacity: int, obs_shape, obs_dtype, device, seed: int = 0):
        self.capacity = int(capacity)
        assert self.capacity >= 1
        self.device = torch.device(device)
        self.on_device = self.device.type == "cuda"
        self.obs_shape = tuple(int(d) for d in obs_shape)
        self.obs_dtype = torch.from_numpy(np.empty(0, dtype=obs_dtype)).dtype
        self.row_bytes = int(np.prod(self.obs_shape, dtype=np.int64)) * np.dtype(obs_dtype).itemsize
        self.seed = int(seed) & _M64
        dev = self.device
        self.obs = torch.zeros((self.capacity,) + self.obs_shape, dtype=self.obs_dtype, device=dev)
        self.next_obs = torch.zeros_like(self.obs)
        self.actions = torch.zeros(self.capacity, dtype=torch.int64, device=dev)
        self.rewards = torch.zeros(self.capacity, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(self.capacity, dtype=torch.uint8, device=dev)
        # host mirror of the device state block (exact: every update is a launch this object issued)
        self.head = 0
        self.len = 0
        self.draws = 0
        self._staging: Dict[int, tuple] = {}
        self._batches: Dict[int, tuple] = {}
        if self.on_device:
            self.state = torch.zeros(C.sizeof(_lib.ReplayState), dtype=torch.uint8, device=dev)
            self.c_ring = _lib.ReplayRing(obs=self.obs.data_ptr(), next_obs=self.next_obs.data_ptr(),
                                          actions=self.actions.data_ptr(), rewards=self.rewards.data_ptr(),
                                          dones=self.dones.data_ptr(), capacity=self.capacity,
                                          row_bytes=self.row_bytes, state=self.state.data_ptr())
            self._staged = torch.cuda.Event()
            self._staged.record(torch.cuda.current_stream(dev))

    def __len__(self) -> int:
        return self.len

    def device_state(self) -> dict:
        """The device's state block (synchronises; tests and diagnostics)."""
        if not self.on_device:
            return dict(head=self.head, len=self.len, draws=self.draws, err=0)
        s = _lib.ReplayState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return dict(head=s.head, len=s.len, draws=s.draws, err=s.err)

    def position_to_slot(self, positions) -> np.ndarray:
        return (self.head - self.len + np.asarray(positions, dtype=np.int64)) % self.capacity

    # -- push ---------------------------------------------------------------------------------------------
    def _stage(self, n: int) -> tuple:
        st = self._staging.get(n)
        if st is None:
            like = ((self.obs, self.obs_shape), (self.next_obs, self.obs_shape), (self.actions, ()),
                    (self.rewards, ()), (self.dones, ()))
            host = [torch.empty((n,) + shp, dtype=t.dtype).pin_memory() for t, shp in like]
            dev = [torch.empty((n,) + shp, dtype=t.dtype, device=self.device) for t, shp in like]
            nbytes = (C.c_int64 * 5)(*[h.numel() * h.element_size() for h in host])
            src = (C.c_void_p * 5)(*[h.data_ptr() for h in host])
            dst = (C.c_void_p * 5)(*[d.data_ptr() for d in dev])
            st = self._staging[n] = (host, [h.numpy() for h in host], dev, src, dst, nbytes)
        return st

    def push(self, obs, next_obs, actions, rewards, dones) -> None:
        """Append N transitions (row i of every array), evicting the oldest: deque(maxlen) order."""
        n = int(np.shape(actions)[0])
        if n > self.capacity:
            raise ValueError(f"push of {n} transitions into a ring of {self.capacity}")
        if n == 0:
            return
        if self.on_device:
            host, host_np, dev, src, dst, nbytes = self._stage(n)
            self._staged.synchronize()  # the previous step's H2D has read the pinned buffers
            for h, a in zip(host_np, (obs, next_obs, actions, rewards, dones)):
                np.copyto(h, np.asarray(a).reshape(h.shape), casting="same_kind")
            L, st = _lib.lib(), _lib.stream_handle(self.device)
            _lib.check(L.rai_copy_h2d_multi(5, dst, src, nbytes, st), "rai_copy_h2d_multi")
            self._staged.record(torch.cuda.current_stream(self.device))
            _lib.check(L.rai_replay_push(C.byref(self.c_ring), *[d.data_ptr() for d in dev], n, st),
                       "rai_replay_push")
        else:
            slots = torch.from_numpy((self.head + np.arange(n)) % self.capacity)
            self.obs[slots] = torch.as_tensor(np.asarray(obs), dtype=self.obs_dtype).reshape((n,) + self.obs_shape)
            self.next_obs[slots] = torch.as_tensor(np.asarray(next_obs),
                                                   dtype=self.obs_dtype).reshape((n,) + self.obs_shape)
            self.actions[slots] = torch.as_tensor(np.asarray(actions), dtype=torch.int64)
            self.rewards[slots] = torch.as_tensor(np.asarray(rewards), dtype=torch.float32)
            self.dones[slots] = torch.as_tensor(np.asarray(dones).astype(np.uint8))
        self.head = (self.head + n) % self.capacity
        self.len = min(self.len + n, self.capacity)

    # -- sample -------------------------------------------------------------------------------------------
    def batch_buffers(self, B: int) -> tuple:
        """The static destination buffers of batch size B: (obs, next_obs, actions, rewards, dones u8, slots)."""
        bufs = self._batches.get(B)
        if bufs is None:
            dev = self.device
            bufs = self._batches[B] = (
                torch.zeros((B,) + self.obs_shape, dtype=self.obs_dtype, device=dev),
                torch.zeros((B,) + self.obs_shape, dtype=self.obs_dtype, device=dev),
                torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.float32, device=dev),
                torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int64, device=dev))
        return bufs

    def launch_sample(self, B: int, inject: Optional[torch.Tensor] = None, count: bool = True) -> None:
        """rai_replay_sample into batch_buffers(B) (device only; capturable: no host state is read by the
        launch).  count=False for a launch recorded into a graph (the caller calls count_draws per replay)."""
        obs, nobs, act, rew, done, slots = self.batch_buffers(B)
        _lib.check(_lib.lib().rai_replay_sample(
            C.byref(self.c_ring), self.seed, B, None if inject is None else inject.data_ptr(), slots.data_ptr(),
            obs.data_ptr(), nobs.data_ptr(), act.data_ptr(), rew.data_ptr(), done.data_ptr(),
            _lib.stream_handle(self.device)), "rai_replay_sample")
        if inject is None and count:
            self.draws += 1

    def count_draws(self, n: int) -> None:
        self.draws += n

    def as_batch(self, B: int) -> Batch:
        obs, nobs, act, rew, done, _ = self.batch_buffers(B)
        return Batch(obs, act, rew, done.view(torch.bool), nobs)

    def sample(self, B: int, positions=None) -> Batch:
        """B distinct transitions drawn uniformly (keyed by (seed, draws)), or the given deque positions
        (0 = oldest; e.g. the reference's own draws).  The returned tensors are the ring's static batch
        buffers: the next sample of the same size overwrites them."""
        B = int(B)
        if B > self.len:
            raise ValueError("Sample larger than population")  # random.sample's error
        if positions is not None:
            positions = np.asarray(positions, dtype=np.int64)
            if positions.shape != (B,) or positions.min() < 0 or positions.max() >= self.len:
                raise ValueError("injected positions outside [0, len)")
        if self.on_device:
            inj = None if positions is None else torch.from_numpy(positions).to(self.device)
            self.launch_sample(B, inj)
            return self.as_batch(B)
        if positions is None:
            positions = feistel_positions(self.len, sample_key(self.seed, self.draws), B)
            self.draws += 1
        slots = torch.from_numpy(self.position_to_slot(positions))
        obs, nobs, act, rew, done, sl = self.batch_buffers(B)
        sl.copy_(slots)
        for dst, src in ((obs, self.obs), (nobs, self.next_obs), (act, self.actions), (rew, self.rewards),
                         (done, self.dones)):
            torch.index_select(src, 0, slots, out=dst)
        return self.as_batch(B)


class ReplayBufferRolloutGenerator:
    """replay_buffer_rollout_generator.py:29-84 over the device ring."""

    def __init__(self, policy, vec_env, buffer_size: int = 1_000_000, learning_starts: int = 50_000,
                 train_freq: int = 4, seed: int = 0) -> None:
        self.policy = policy
        self.vec_env = vec_env
        if vec_env.num_envs > buffer_size:
            raise ValueError(f"num_envs ({vec_env.num_envs}) exceeds buffer_size ({buffer_size})")
        self.next_obs, _ = vec_env.reset()
        assert isinstance(self.next_obs, np.ndarray)
        self.learning_starts = learning_starts
        self.train_freq = train_freq
        self.buffer = ReplayRing(buffer_size, self.next_obs.shape[1:], self.next_obs.dtype, policy.device, seed=seed)
        if self.learning_starts > 0:
            self._collect_transitions(int(np.ceil(self.learning_starts / self.vec_env.num_envs)), eps=1)

    def prepare(self) -> None:
        pass

    def rollout(self, **kwargs) -> int:
        return self._collect_transitions(self.train_freq, **kwargs)

    def _collect_transitions(self, n_steps: int, **kwargs) -> int:
        self.policy.train(False)
        for _ in range(n_steps):
            actions = self.policy.act(self.next_obs, deterministic=False, **kwargs)
            next_obs, rewards, terminations, truncations, _ = self.vec_env.step(actions)
            dones = terminations | truncations
            assert isinstance(next_obs, np.ndarray)
            self.buffer.push(self.next_obs, next_obs, actions, rewards, dones)  # all envs in one push
            self.next_obs = next_obs
        return n_steps * self.vec_env.num_envs

    def sample(self, batch_size: int, device=None) -> Batch:
        return self.buffer.sample(batch_size)
