"""Host-side environments behind the reference's gymnasium VectorEnv API
(rl_algo_impls/wrappers/vector_wrapper.py:16-20; rollout/sync_step_rollout.py:80-92,
202-209): reset() -> (obs, info); step(a) -> (obs, rew, term, trunc, info);
num_envs, single_observation_space, single_action_space.

Env stepping stays on the host CPU (north star).  Provided here:
  * minimal Box / Discrete spaces (gymnasium is not installed; real gymnasium
    spaces work too — the trainer duck-types on .n / .low / .shape),
  * SyntheticVecEnv: the seeded synthetic environments the benchmark and the
    golden fixtures use (SURVEY.md §8d "Synthetic inputs"),
  * CartPoleVecEnv: a vectorised CartPole-v1 restated from gymnasium's public
    dynamics, with same-step autoreset and RecordEpisodeStatistics-style
    episode returns, for return-parity runs.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import numpy as np


class Box:
    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        if shape is None:
            shape = np.shape(low) if np.ndim(low) else np.shape(high)
        self.shape = tuple(shape)
        self.low = np.broadcast_to(np.asarray(low, dtype=self.dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=self.dtype), self.shape).copy()

    def sample(self, rng: Optional[np.random.Generator] = None):
        rng = rng or np.random.default_rng()
        if np.issubdtype(self.dtype, np.integer):
            return rng.integers(self.low, self.high.astype(np.int64) + 1, size=self.shape).astype(self.dtype)
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return rng.uniform(lo, hi, size=self.shape).astype(self.dtype)


class Discrete:
    def __init__(self, n: int):
        self.n = int(n)
        self.shape = ()
        self.dtype = np.dtype(np.int64)

    def sample(self, rng: Optional[np.random.Generator] = None):
        rng = rng or np.random.default_rng()
        return np.int64(rng.integers(self.n))


class MultiDiscrete:
    def __init__(self, nvec):
        self.nvec = np.asarray(nvec, dtype=np.int64)
        self.shape = self.nvec.shape
        self.dtype = np.dtype(np.int64)

    def sample(self, rng: Optional[np.random.Generator] = None):
        rng = rng or np.random.default_rng()
        return rng.integers(0, self.nvec)


MICRORTS_NVEC = (6, 4, 4, 4, 4, 7, 49)  # MicroRTS per-cell action planes (78 logits)


def is_multidiscrete(space) -> bool:
    return hasattr(space, "nvec")


def is_discrete(space) -> bool:
    return hasattr(space, "n") and not hasattr(space, "nvec")


def is_box(space) -> bool:
    return hasattr(space, "low") and hasattr(space, "high")


class SyntheticVecEnv:
    """Seeded synthetic vector env with the shapes of the BASELINE configs.

    kind = "cartpole": obs ~ N(0,1) f32 (N,4), 2 actions, reward 1.0,
                       termination ~ Bernoulli(term_prob) (default 1/200)
    kind = "pong":     obs ~ U{0..255} u8 (N,4,84,84), 6 actions, reward ~ N(0,1),
                       termination ~ Bernoulli(1/1000)
    kind = "halfcheetah": obs ~ N(0,1) f32 (N,17), Box(6) actions in [-1,1],
                       reward ~ N(0,1), termination ~ Bernoulli(1/1000)
    kind = "microrts": obs ~ U{0,1} f32 (N,74,16,16) (CHW planes), GridNet actions
                       MultiDiscrete(tile(nvec, 256)) with action_plane_space
                       MultiDiscrete([6,4,4,4,4,7,49]), all-true action masks (N,256,78) from
                       get_action_mask(), K=3 rewards ~ N(0,1) (N,3), termination ~ Bernoulli(1/1000)
                       
    Truncations are always False (the reference treats them like terminations).

    Observation batches are drawn from a pool of `obs_pool` batches generated at construction
    (a uniformly chosen pool entry per step): the env's own cost would otherwise sit inside the
    timed rollout (numpy generates the 29 MB of uniform bytes of a 1024-env Pong step in ~45 ms,
    more than the whole device step) while saying nothing about the hot path.  Rewards and
    terminations are drawn fresh every step.  Returned observation arrays are shared with the
    pool: consumers copy them (the rollout stages them into pinned memory) and must not write.
    """

    def __init__(self, num_envs: int, kind: str = "cartpole", seed: int = 1,
                 term_prob: Optional[float] = None, obs_pool: Optional[int] = None):
        self.num_envs = int(num_envs)
        self.kind = kind
        self.rng = np.random.default_rng(seed)
        if kind == "cartpole":
            self.single_observation_space = Box(-np.inf, np.inf, (4,), np.float32)
            self.single_action_space = Discrete(2)
            self.term_prob = 1 / 200 if term_prob is None else term_prob
        elif kind == "pong":
            self.single_observation_space = Box(0, 255, (4, 84, 84), np.uint8)
            self.single_action_space = Discrete(6)
            self.term_prob = 1 / 1000 if term_prob is None else term_prob
        elif kind == "halfcheetah":
            self.single_observation_space = Box(-np.inf, np.inf, (17,), np.float32)
            self.single_action_space = Box(-1.0, 1.0, (6,), np.float32)
            self.term_prob = 1 / 1000 if term_prob is None else term_prob
        elif kind == "microrts":
            self.map_hw = (16, 16)
            cells = self.map_hw[0] * self.map_hw[1]
            self.single_observation_space = Box(0.0, 1.0, (74,) + self.map_hw, np.float32)
            self.action_plane_space = MultiDiscrete(MICRORTS_NVEC)
            self.single_action_space = MultiDiscrete(np.tile(MICRORTS_NVEC, cells))
            self.term_prob = 1 / 1000 if term_prob is None else term_prob
            self._mask = np.ones((self.num_envs, cells, int(sum(MICRORTS_NVEC))), dtype=np.bool_)
            self.get_action_mask = lambda: self._mask
        else:
            raise ValueError(f"unknown synthetic env kind {kind}")
        batch_bytes = self.num_envs * int(np.prod(self.single_observation_space.shape)) * \
            np.dtype(self.single_observation_space.dtype).itemsize
        if obs_pool is None:  # up to 16 batches within ~256 MB
            obs_pool = int(max(2, min(16, (256 << 20) // max(batch_bytes, 1))))
        self._pool = [self._draw_obs() for _ in range(int(obs_pool))]

    @property
    def unwrapped(self):
        return self

    def _obs(self) -> np.ndarray:
        return self._pool[int(self.rng.integers(len(self._pool)))]

    def _draw_obs(self) -> np.ndarray:
        N = self.num_envs
        shp = self.single_observation_space.shape
        if self.kind == "pong":
            return self.rng.integers(0, 256, size=(N,) + shp, dtype=np.uint8)
        if self.kind == "microrts":
            return (self.rng.random((N,) + shp, dtype=np.float32) < 0.5).astype(np.float32)
        return self.rng.standard_normal((N,) + shp, dtype=np.float32)

    def reset(self, **kwargs) -> Tuple[np.ndarray, Dict[str, Any]]:
        return self._obs(), {}

    def step(self, actions):
        N = self.num_envs
        obs = self._obs()
        if self.kind == "cartpole":
            rew = np.ones(N, dtype=np.float32)
        elif self.kind == "microrts":
            rew = self.rng.standard_normal((N, 3), dtype=np.float32)
        else:
            rew = self.rng.standard_normal(N, dtype=np.float32)
        term = self.rng.random(N) < self.term_prob
        trunc = np.zeros(N, dtype=np.bool_)
        return obs, rew, term, trunc, {}

    def close(self):
        pass


class MaskedMultiDiscreteVecEnv:
    """Seeded synthetic vector env with a flat MultiDiscrete(nvec) action space and get_action_mask():
    obs ~ N(0, 1) f32 (N, obs_dim), fresh every step; the (N, sum(nvec)) bool mask is a pure function of the
    current observation (mask_of), so a mask that lags its observation by a step shows; every group keeps at
    least one valid entry.  Reward: the fraction of a row's sub-actions that are valid under the mask the
    env handed out (1.0 for a policy that respects it); invalid_actions counts the others.  Termination
    ~ Bernoulli(term_prob)."""

    def __init__(self, num_envs: int, nvec=(3, 5, 2), obs_dim: int = 5, seed: int = 1, term_prob: float = 1 / 50):
        self.num_envs = int(num_envs)
        self.rng = np.random.default_rng(seed)
        self.single_observation_space = Box(-np.inf, np.inf, (obs_dim,), np.float32)
        self.single_action_space = MultiDiscrete(nvec)
        self.nvec = self.single_action_space.nvec
        self.term_prob = term_prob
        self.invalid_actions = 0
        self._obs = self._draw()

    @property
    def unwrapped(self):
        return self

    def _draw(self) -> np.ndarray:
        return self.rng.standard_normal((self.num_envs,) + self.single_observation_space.shape, dtype=np.float32)

    def mask_of(self, obs: np.ndarray) -> np.ndarray:
        """Entry a of a row is valid when obs[a % obs_dim] * (-1)^a > -0.4 (about two in three); entry
        floor(8 |obs[g % obs_dim]|) % nvec[g] of group g is always valid."""
        nvec = self.nvec
        obs = np.asarray(obs, dtype=np.float32)
        A, D = int(nvec.sum()), obs.shape[1]
        a = np.arange(A)
        mask = obs[:, a % D] * np.where(a % 2 == 0, 1.0, -1.0).astype(np.float32) > np.float32(-0.4)
        off = np.concatenate([[0], np.cumsum(nvec)])
        for g, n in enumerate(nvec):
            keep = np.floor(8.0 * np.abs(obs[:, g % D])).astype(np.int64) % int(n)
            mask[np.arange(obs.shape[0]), off[g] + keep] = True
        return mask

    def get_action_mask(self) -> np.ndarray:
        return self.mask_of(self._obs)

    def reset(self, **kwargs) -> Tuple[np.ndarray, Dict[str, Any]]:
        self._obs = self._draw()
        return self._obs, {}

    def step(self, actions):
        nvec = self.nvec
        a = np.asarray(actions).reshape(self.num_envs, len(nvec))
        off = np.concatenate([[0], np.cumsum(nvec)])[:-1]
        in_range = (a >= 0) & (a < nvec)
        valid = in_range & np.take_along_axis(self.get_action_mask(), off + np.where(in_range, a, 0), axis=1)
        self.invalid_actions += int((~valid).sum())
        self._obs = self._draw()
        term = self.rng.random(self.num_envs) < self.term_prob
        return self._obs, valid.mean(axis=1).astype(np.float32), term, np.zeros(self.num_envs, dtype=np.bool_), {}

    def close(self):
        pass


class CartPoleVecEnv:
    """Vectorised CartPole-v1 (gymnasium 0.29 public dynamics: Euler integration,
    tau=0.02, force 10, pole half-length 0.5, termination |x|>2.4 or
    |theta|>12deg, truncation at 500 steps, reward 1 per step, reset state
    ~ U(-0.05, 0.05)).  Same-step autoreset like gymnasium's vector envs; the
    finished episode's return/length arrive in info["episode"] with mask
    info["_episode"] (RecordEpisodeStatistics convention)."""

    gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    theta_threshold = 12 * 2 * np.pi / 360
    x_threshold = 2.4
    max_episode_steps = 500

    def __init__(self, num_envs: int, seed: int = 1):
        self.num_envs = int(num_envs)
        high = np.array([self.x_threshold * 2, np.finfo(np.float32).max,
                         self.theta_threshold * 2, np.finfo(np.float32).max], dtype=np.float32)
        self.single_observation_space = Box(-high, high, (4,), np.float32)
        self.single_action_space = Discrete(2)
        self.rngs = [np.random.default_rng(seed + i) for i in range(self.num_envs)]
        self.state = np.zeros((self.num_envs, 4), dtype=np.float64)
        self.steps = np.zeros(self.num_envs, dtype=np.int64)
        self.ep_return = np.zeros(self.num_envs, dtype=np.float64)

    @property
    def unwrapped(self):
        return self

    def _reset_idx(self, idx):
        for i in idx:
            self.state[i] = self.rngs[i].uniform(-0.05, 0.05, size=4)
        self.steps[idx] = 0
        self.ep_return[idx] = 0

    def reset(self, **kwargs):
        self._reset_idx(np.arange(self.num_envs))
        return self.state.astype(np.float32), {}

    def step(self, actions):
        a = np.asarray(actions).reshape(self.num_envs)
        x, x_dot, th, th_dot = self.state.T
        force = np.where(a == 1, self.force_mag, -self.force_mag)
        cos, sin = np.cos(th), np.sin(th)
        total_mass = self.masspole + self.masscart
        pml = self.masspole * self.length
        temp = (force + pml * th_dot ** 2 * sin) / total_mass
        th_acc = (self.gravity * sin - cos * temp) / (
            self.length * (4.0 / 3.0 - self.masspole * cos ** 2 / total_mass))
        x_acc = temp - pml * th_acc * cos / total_mass
        x = x + self.tau * x_dot
        x_dot = x_dot + self.tau * x_acc
        th = th + self.tau * th_dot
        th_dot = th_dot + self.tau * th_acc
        self.state = np.stack([x, x_dot, th, th_dot], axis=1)
        self.steps += 1
        term = (np.abs(x) > self.x_threshold) | (np.abs(th) > self.theta_threshold)
        trunc = (self.steps >= self.max_episode_steps) & ~term
        rew = np.ones(self.num_envs, dtype=np.float32)
        self.ep_return += 1.0
        done = term | trunc
        info: Dict[str, Any] = {}
        if done.any():
            idx = np.nonzero(done)[0]
            info["episode"] = {"r": np.where(done, self.ep_return, 0.0),
                               "l": np.where(done, self.steps, 0)}
            info["_episode"] = done.copy()
            self._reset_idx(idx)
        return self.state.astype(np.float32), rew, term, trunc, info

    def close(self):
        pass


class ScriptedBotGridVecEnv:
    """A MicroRTS-shaped vector env played by a scripted bot, for the reference-AI rollout generator
    (reference_rollout.ReferenceAIRolloutGenerator): GridNet actions MultiDiscrete(tile(nvec, cells)) with
    action_plane_space MultiDiscrete(nvec), get_action_mask() (N, cells, sum(nvec)) bool and last_action
    (N, cells, len(nvec)) int32, the bot's action of the step just taken.

    Observations f32 (N, PLANES, h, w) ~ U[0, 1) come from a pool of `obs_pool` batches drawn at construction
    (a seeded pool index per step).  Masks and the bot are pure functions of the current observation:
      mask_of(obs):  cell c is empty ("no unit": every entry false) when plane 0 is below 0.35; in a live cell
                     entry a is valid when (floor(64 obs[1 + a % 5]) + a) % 3 != 0, and group
                     d = floor(16 obs[6]) is all false when d < G (about 7 live cells in 16 have one);
      bot_action(obs, mask): per group the k-th valid entry, k = floor(1024 obs[1 + g % 5]) mod the group's
                     number of valid entries; 0 where the group has none.  Always legal.
    step(actions) ignores `actions` for the dynamics and appends a copy of what it received to self.received.
    With illegal_every = m > 0 the (step, env) pairs p = step * N + n with p % m == m - 1 get one in-range
    but masked-out component: illegal_component(mask[n]) names it (the first group, in (cell, group) order,
    that has both a valid and an invalid entry, set to its first invalid entry); a pair whose mask has no such
    group is left alone.  Out-of-range values are never emitted.  Reward ~ U[0, 1) f32 (N,), termination
    ~ Bernoulli(term_prob), both from the env's generator."""

    PLANES = 7

    def __init__(self, num_envs: int, map_hw=(4, 4), nvec=MICRORTS_NVEC, seed: int = 1, illegal_every: int = 0,
                 term_prob: float = 1 / 8, obs_pool: int = 8):
        self.num_envs = int(num_envs)
        self.map_hw = tuple(int(x) for x in map_hw)
        self.cells = self.map_hw[0] * self.map_hw[1]
        self.nvec = np.asarray(nvec, dtype=np.int64)
        self.illegal_every = int(illegal_every)
        self.term_prob = term_prob
        self.rng = np.random.default_rng(seed)
        self._make_spaces()
        self._pool = [self.rng.random((self.num_envs,) + self.single_observation_space.shape, dtype=np.float32)
                      for _ in range(int(obs_pool))]
        self.received: list = []
        self.steps = 0
        self._obs = self._pool[0]
        self.last_action = np.zeros(self._action_shape(), dtype=np.int32)

    def _make_spaces(self) -> None:
        self.single_observation_space = Box(0.0, 1.0, (self.PLANES,) + self.map_hw, np.float32)
        self.action_plane_space = MultiDiscrete(self.nvec)
        self.single_action_space = MultiDiscrete(np.tile(self.nvec, self.cells))

    def _action_shape(self) -> Tuple[int, ...]:
        return (self.num_envs, self.cells, len(self.nvec))

    def _mask_shape(self) -> Tuple[int, ...]:
        return (self.num_envs, self.cells, int(self.nvec.sum()))

    @property
    def unwrapped(self):
        return self

    def _planes(self, obs: np.ndarray) -> np.ndarray:
        """(N, cells, PLANES)"""
        o = np.asarray(obs, dtype=np.float32).reshape(-1, self.PLANES, self.cells)
        return np.moveaxis(o, 1, 2)

    def mask_of(self, obs: np.ndarray) -> np.ndarray:
        o = self._planes(obs)
        A, G = int(self.nvec.sum()), len(self.nvec)
        a = np.arange(A)
        m = (np.floor(64.0 * o[:, :, 1 + a % 5]).astype(np.int64) + a) % 3 != 0
        group_of = np.repeat(np.arange(G), self.nvec)
        dead = np.floor(16.0 * o[:, :, 6]).astype(np.int64)
        m &= group_of[None, None, :] != dead[:, :, None]
        m &= (o[:, :, 0] >= np.float32(0.35))[:, :, None]
        return m.reshape((o.shape[0],) + self._mask_shape()[1:])

    def bot_action(self, obs: np.ndarray, mask: np.ndarray) -> np.ndarray:
        o = self._planes(obs)
        m = np.asarray(mask).reshape(o.shape[0], self.cells, -1)
        out = np.zeros((o.shape[0], self.cells, len(self.nvec)), dtype=np.int32)
        off = 0
        for g, n in enumerate(self.nvec):
            mg = m[:, :, off:off + int(n)]
            cnt = mg.sum(-1)
            k = np.floor(1024.0 * o[:, :, 1 + g % 5]).astype(np.int64) % np.maximum(cnt, 1)
            pick = (np.cumsum(mg, -1) == (k + 1)[:, :, None]) & mg  # the k-th valid entry
            out[:, :, g] = np.where(cnt > 0, pick.argmax(-1), 0)
            off += int(n)
        return out.reshape((o.shape[0],) + self._action_shape()[1:])

    def illegal_component(self, mask_env: np.ndarray):
        """(cell, group, value) of the component illegal_every corrupts for an env with this mask, or None."""
        m = np.asarray(mask_env).reshape(self.cells, -1)
        for c in range(self.cells):
            off = 0
            for g, n in enumerate(self.nvec):
                mg = m[c, off:off + int(n)]
                if mg.any() and not mg.all():
                    return c, g, int(np.argmin(mg))
                off += int(n)
        return None

    def get_action_mask(self) -> np.ndarray:
        return self.mask_of(self._obs)

    def reset(self, **kwargs) -> Tuple[np.ndarray, Dict[str, Any]]:
        self._obs = self._pool[int(self.rng.integers(len(self._pool)))]
        return self._obs, {}

    def step(self, actions):
        N = self.num_envs
        self.received.append(np.array(actions, copy=True))
        mask = self.get_action_mask()
        act = self.bot_action(self._obs, mask).reshape(N, self.cells, len(self.nvec))
        if self.illegal_every > 0:
            for n in range(N):
                if (self.steps * N + n) % self.illegal_every == self.illegal_every - 1:
                    hit = self.illegal_component(mask[n])
                    if hit is not None:
                        act[n, hit[0], hit[1]] = hit[2]
        self.last_action = act.reshape(self._action_shape())
        self.steps += 1
        self._obs = self._pool[int(self.rng.integers(len(self._pool)))]
        rew = self.rng.random(N, dtype=np.float32)
        term = self.rng.random(N) < self.term_prob
        return self._obs, rew, term, np.zeros(N, dtype=np.bool_), {}

    def close(self):
        pass


class ScriptedBotDiscreteVecEnv(ScriptedBotGridVecEnv):
    """The flat sibling of ScriptedBotGridVecEnv: one cell, one group.  Observations (N, PLANES), a
    Discrete(n) action space, get_action_mask() (N, n) and last_action (N,) int32, by the same functions."""

    def __init__(self, num_envs: int, n: int = 6, seed: int = 1, illegal_every: int = 0, term_prob: float = 1 / 8,
                 obs_pool: int = 8):
        super().__init__(num_envs, map_hw=(1, 1), nvec=(n,), seed=seed, illegal_every=illegal_every,
                         term_prob=term_prob, obs_pool=obs_pool)

    def _make_spaces(self) -> None:
        self.single_observation_space = Box(0.0, 1.0, (self.PLANES,), np.float32)
        self.single_action_space = Discrete(int(self.nvec[0]))

    def _action_shape(self) -> Tuple[int, ...]:
        return (self.num_envs,)

    def _mask_shape(self) -> Tuple[int, ...]:
        return (self.num_envs, int(self.nvec[0]))
