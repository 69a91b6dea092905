"""DQN on MI355X — drop-in for rl_algo_impls/dqn/{q_net,policy,dqn}.py.

QNetwork / DQNPolicy are built from the existing Encoder and mlp (the hand-written NatureCNN and IMPALA
paths unchanged); state_dict keys and shapes are the reference's (`q_net._feature_extractor...`,
`q_net._fc.N...`), so model.pth is drop-in.

One gradient step on the device (csrc/dqn.hip):

    rai_replay_sample      keyed draw without replacement + gather into static batch buffers
    target forward         no_grad; up to the last hidden layer on the fused-head path
    online forward
    rai_dqn_head_fwd/_bwd  the final Linear(H -> A) of both networks + TD target + smooth-L1 + its one
                           non-zero per row gradient (H <= 512, A <= 32), or torch's linear +
                           rai_dqn_td_loss otherwise
    autograd backward      into the flat .grad buffer
    rai_clip_optim_step    clip_grad_norm_ + Adam

captured once into a hipGraph and replayed; the gradient_steps steps of one learn() iteration are enqueued
without a host sync between them.  The target network is a second flat buffer updated by rai_polyak_update.
On the CPU everything falls back to plain torch with the reference's own expressions.
"""
from __future__ import annotations

import copy
import ctypes as C
import logging
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .envs import is_discrete
from .optim import FlatOptimizer, FlatParams, struct_to_device
from .pg_common import load_optimizer, save_optimizer
from .policy import ActorCritic, Encoder, mlp
from .replay import Batch, ReplayBufferRolloutGenerator

__all__ = ["QNetwork", "DQNPolicy", "DQN", "Batch", "ReplayBufferRolloutGenerator", "argmax_rows", "td_loss",
           "polyak_update", "head_supported"]


# -- kernel wrappers -------------------------------------------------------------------------------------
def argmax_rows(x: torch.Tensor) -> torch.Tensor:
    """x.argmax(1) (first maximum, NaN counts as the maximum): rai_argmax_rows on the device."""
    if not x.is_cuda:
        return x.argmax(dim=1)
    x = x.contiguous()
    assert x.dtype == torch.float32 and x.dim() == 2
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().rai_argmax_rows(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), out.data_ptr(),
                                          _lib.stream_handle(x.device)), "rai_argmax_rows")
    return out


def _u8(d: torch.Tensor) -> torch.Tensor:
    return d.view(torch.uint8) if d.dtype == torch.bool else d


def td_loss(q, q_next, actions, rewards, dones, gamma: float):
    """(target (B), loss scalar, dq (B, A)) of dqn.py:114-117: rai_dqn_td_loss on the device for A <= 256,
    torch's own expressions otherwise."""
    B, A = int(q.shape[0]), int(q.shape[1])
    if q.is_cuda and A <= _lib.RAI_DQN_MAX_A:
        q, q_next = q.contiguous(), q_next.contiguous()
        target = torch.empty(B, dtype=torch.float32, device=q.device)
        loss = torch.empty((), dtype=torch.float32, device=q.device)
        dq = torch.empty_like(q)
        _lib.check(_lib.lib().rai_dqn_td_loss(q.data_ptr(), q_next.data_ptr(), actions.data_ptr(), rewards.data_ptr(),
                                              _u8(dones).data_ptr(), B, A, float(gamma), target.data_ptr(),
                                              loss.data_ptr(), dq.data_ptr(), _lib.stream_handle(q.device)),
                   "rai_dqn_td_loss")
        return target, loss, dq
    nd = ~dones if dones.dtype == torch.bool else dones == 0
    target = rewards + nd * gamma * q_next.max(1).values
    cur = q.gather(1, actions.unsqueeze(1)).squeeze(1)
    diff = cur - target
    loss = F.smooth_l1_loss(cur, target)
    dq = torch.zeros_like(q).scatter_(1, actions.unsqueeze(1), (diff.clamp(-1, 1) / B).unsqueeze(1))
    return target, loss, dq


def polyak_update(target: torch.Tensor, params: torch.Tensor, tau: float) -> None:
    """target = tau * params + (1 - tau) * target over flat buffers (dqn.py:125-131's rounding)."""
    if target.is_cuda:
        _lib.check(_lib.lib().rai_polyak_update(target.data_ptr(), params.data_ptr(), int(target.numel()), float(tau),
                                                1 - float(tau), _lib.stream_handle(target.device)),
                   "rai_polyak_update")
    else:
        target.copy_(tau * params + (1 - tau) * target)


def head_supported(H: int, A: int) -> bool:
    return 1 <= H <= _lib.RAI_DQN_HEAD_MAX_H and 1 <= A <= _lib.RAI_DQN_HEAD_MAX_A


def head_fwd(h, h_next, w, b, wt, bt, actions, rewards, dones, gamma: float, want_q: bool = False):
    """rai_dqn_head_fwd: (target (B), loss scalar, g (B)[, q, q_next]); None when the shape is unsupported
    (RAI_E_UNSUPPORTED: the caller takes the unfused path)."""
    B, H, A = int(h.shape[0]), int(h.shape[1]), int(w.shape[0])
    dev = h.device
    h, h_next = h.contiguous(), h_next.contiguous()
    target = torch.empty(B, dtype=torch.float32, device=dev)
    g = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    q = torch.empty((B, A), dtype=torch.float32, device=dev) if want_q else None
    qn = torch.empty((B, A), dtype=torch.float32, device=dev) if want_q else None
    L = _lib.lib()
    ws = torch.empty(max(int(L.rai_dqn_head_workspace_bytes(B)), 4), dtype=torch.uint8, device=dev)
    rc = L.rai_dqn_head_fwd(h.data_ptr(), h_next.data_ptr(), w.data_ptr(), b.data_ptr(), wt.data_ptr(), bt.data_ptr(),
                            actions.data_ptr(), rewards.data_ptr(), _u8(dones).data_ptr(), B, H, A, float(gamma),
                            target.data_ptr(), loss.data_ptr(), g.data_ptr(), _lib.ptr(q), _lib.ptr(qn),
                            ws.data_ptr(), ws.numel(), _lib.stream_handle(dev))
    if rc == _lib.RAI_E_UNSUPPORTED:
        return None
    _lib.check(rc, "rai_dqn_head_fwd")
    return (target, loss, g, q, qn) if want_q else (target, loss, g)


def head_bwd(h, w, actions, g, dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None):
    """rai_dqn_head_bwd: dh (B, H) returned; dw / db accumulated into the given tensors (the flat .grad
    views) or returned fresh."""
    B, H, A = int(h.shape[0]), int(h.shape[1]), int(w.shape[0])
    acc = dw is not None
    if acc:
        assert db is not None and dw.is_contiguous() and db.is_contiguous()
    else:
        dw, db = torch.empty_like(w), torch.empty(A, dtype=torch.float32, device=h.device)
    h = h.contiguous()
    dh = torch.empty_like(h)
    _lib.check(_lib.lib().rai_dqn_head_bwd(h.data_ptr(), w.data_ptr(), actions.data_ptr(), g.data_ptr(), B, H, A,
                                           dh.data_ptr(), dw.data_ptr(), db.data_ptr(), 1 if acc else 0,
                                           _lib.stream_handle(h.device)), "rai_dqn_head_bwd")
    return dh, dw, db


# -- network and policy ----------------------------------------------------------------------------------
class QNetwork(nn.Module):  # rl_algo_impls/dqn/q_net.py:12-41
    def __init__(self, observation_space, action_space, hidden_sizes: Sequence[int] = (), activation=nn.ReLU,
                 cnn_flatten_dim: int = 512, cnn_style: str = "nature",
                 cnn_layers_init_orthogonal: Optional[bool] = None,
                 impala_channels: Sequence[int] = (16, 32, 32)) -> None:
        super().__init__()
        assert is_discrete(action_space)
        self._feature_extractor = Encoder(observation_space, activation, cnn_flatten_dim=cnn_flatten_dim,
                                          cnn_style=cnn_style, cnn_layers_init_orthogonal=cnn_layers_init_orthogonal,
                                          impala_channels=tuple(impala_channels))
        layer_sizes = (self._feature_extractor.out_dim,) + tuple(hidden_sizes) + (action_space.n,)
        self._fc = mlp(layer_sizes, activation)

    @property
    def head(self) -> nn.Linear:
        """The final Linear(H -> A) (mlp() ends Linear, Identity)."""
        return self._fc[-2]

    def trunk(self, obs: torch.Tensor) -> torch.Tensor:
        """The last hidden activations (B, H): everything before the final Linear."""
        x = self._feature_extractor(obs)
        for m in list(self._fc)[:-2]:
            x = m(x)
        return x

    def forward(self, obs: torch.Tensor) -> torch.Tensor:
        return self._fc(self._feature_extractor(obs))

    def conv_weights(self) -> list:
        fe = self._feature_extractor
        return fe.feature_extractor.conv_weights() if fe.kind == "cnn" else []


class DQNPolicy(nn.Module):  # rl_algo_impls/dqn/policy.py:13-56 over shared/policy/policy.py:29-152
    def __init__(self, env, hidden_sizes: Sequence[int] = (), cnn_flatten_dim: int = 512, cnn_style: str = "nature",
                 cnn_layers_init_orthogonal: Optional[bool] = None, impala_channels: Sequence[int] = (16, 32, 32),
                 **kwargs) -> None:
        super().__init__()
        from .wrappers import NormalizeObservation, NormalizeReward, find_wrapper

        self.env = env
        norm_obs = find_wrapper(env, NormalizeObservation)
        self.norm_observation_rms = norm_obs.rms if norm_obs else None
        norm_rew = find_wrapper(env, NormalizeReward)
        self.norm_reward_rms = norm_rew.rms if norm_rew else None
        self._device: Optional[torch.device] = None
        self.load_path: Optional[str] = None
        self.q_net = QNetwork(env.single_observation_space, env.single_action_space, hidden_sizes,
                              cnn_flatten_dim=cnn_flatten_dim, cnn_style=cnn_style,
                              cnn_layers_init_orthogonal=cnn_layers_init_orthogonal, impala_channels=impala_channels)

    def to(self, device=None, *args, **kwargs):
        super().to(device, *args, **kwargs)
        if device is not None:
            self._device = torch.device(device)
        return self

    @property
    def device(self) -> torch.device:
        assert self._device is not None, "Expect device to be set"
        return self._device

    # checkpoint / normalisation plumbing shared with the actor-critic policy (shared/policy/policy.py)
    _as_tensor = ActorCritic._as_tensor
    save_weights = ActorCritic.save_weights
    load_weights = ActorCritic.load_weights
    save = ActorCritic.save
    load = ActorCritic.load
    sync_normalization = ActorCritic.sync_normalization
    num_parameters = ActorCritic.num_parameters
    reset_noise = ActorCritic.reset_noise

    def act(self, obs, eps: float = 0, deterministic: bool = True, action_masks=None) -> np.ndarray:
        assert eps == 0 if deterministic else eps >= 0
        assert action_masks is None, f"action_masks not currently supported in {self.__class__.__name__}"
        if not deterministic and np.random.random() < eps:  # ONE coin per call, shared by all envs
            return np.array([self.env.single_action_space.sample() for _ in range(self.env.num_envs)])
        o = self._as_tensor(obs)
        with torch.no_grad():
            return argmax_rows(self.q_net(o)).cpu().numpy()


def linear_schedule(start_val: float, end_val: float, end_progress: float = 1.0):  # shared/schedule.py
    def func(progress: float) -> float:
        if progress >= end_progress:
            return end_val
        return start_val + (end_val - start_val) * progress / end_progress

    return func


# -- the algorithm ----------------------------------------------------------------------------------------
class DQN:
    """rl_algo_impls/dqn/dqn.py:23-131: the same kwargs, defaults and learn() loop."""

    WARMUP = 2  # eager steps before the capture (lazy library handles, autograd stream state)

    def __init__(self, policy: DQNPolicy, device, tb_writer, learning_rate: float = 1e-4, batch_size: int = 32,
                 tau: float = 1.0, gamma: float = 0.99, gradient_steps: int = 1, target_update_interval: int = 10_000,
                 exploration_fraction: float = 0.1, exploration_initial_eps: float = 1.0,
                 exploration_final_eps: float = 0.05, max_grad_norm: float = 10.0, fused_head: bool = True) -> None:
        self.policy = policy
        self.device = torch.device(device)
        self.tb_writer = tb_writer
        self.learning_rate = learning_rate
        self.on_device = self.device.type == "cuda"
        q_net = policy.q_net
        self.target_q_net = copy.deepcopy(q_net).to(self.device)
        self.target_q_net.train(False)
        for p in self.target_q_net.parameters():
            p.requires_grad_(False)
        if self.on_device:
            self.flat = FlatParams(q_net, self.device, channels_last=q_net.conv_weights())
            self.optimizer = FlatOptimizer(self.flat, FlatOptimizer.ADAM, lr=learning_rate, eps=1e-8,
                                           max_grad_norm=max_grad_norm or 0.0)
            # the target network: a second flat buffer in the same layout, never trained
            self.target_flat = FlatParams(self.target_q_net, self.device,
                                          channels_last=self.target_q_net.conv_weights())
            for p in self.target_q_net.parameters():
                p.grad = None
            self.target_flat.grad = None
            self.state_dev = torch.empty(C.sizeof(_lib.TrainState), dtype=torch.uint8, device=self.device)
            off = _lib.TrainState.norm_index.offset
            self._norm_index = self.state_dev[off:off + 4].view(torch.int32)
            self.norms = torch.zeros(1, dtype=torch.float32, device=self.device)
            self._sync_train_state()
            self.stream = torch.cuda.Stream(self.device)
            self._graphs: dict = {}
        else:
            self.optimizer = torch.optim.Adam(q_net.parameters(), lr=learning_rate)
        self.tau = tau
        self.target_update_interval = target_update_interval
        self.batch_size = batch_size
        self.gradient_steps = gradient_steps
        self.gamma = gamma
        self.exploration_eps_schedule = linear_schedule(exploration_initial_eps, exploration_final_eps,
                                                        end_progress=exploration_fraction)
        self.max_grad_norm = max_grad_norm
        self.fused_head = fused_head
        self.last_targets: Optional[torch.Tensor] = None
        self.last_loss: Optional[torch.Tensor] = None
        self.last_grad_norm: Optional[torch.Tensor] = None
        self.target_updates = 0

    def enable_data_parallel(self, group=None, **kwargs) -> None:
        import torch.distributed as dist

        if dist.get_world_size(group) > 1:
            raise NotImplementedError("data-parallel DQN (world > 1) is out of scope")

    def _sync_train_state(self) -> None:
        struct_to_device(_lib.TrainState(opt_step=self.optimizer.step_count, stat_index=0, pi_coef_zero=0,
                                         norm_index=0), self.device, self.state_dev)

    # -- reference API -----------------------------------------------------------------------------------
    def learn(self, train_timesteps: int, rollout_generator: ReplayBufferRolloutGenerator,
              callbacks: Optional[List] = None, total_timesteps: Optional[int] = None,
              start_timesteps: int = 0) -> "DQN":
        if total_timesteps is None:
            total_timesteps = train_timesteps
        assert start_timesteps + train_timesteps <= total_timesteps
        timesteps_elapsed = max(start_timesteps, rollout_generator.learning_starts)
        steps_since_target_update = 0
        while timesteps_elapsed < total_timesteps:
            progress = timesteps_elapsed / total_timesteps
            eps = self.exploration_eps_schedule(progress)
            rollout_steps = rollout_generator.rollout(eps=eps)
            timesteps_elapsed += rollout_steps
            if len(rollout_generator.buffer) > self.batch_size:
                n = self.gradient_steps if self.gradient_steps > 0 else rollout_generator.train_freq
                if self.on_device:
                    self.train_sampled(rollout_generator.buffer, n)  # enqueued, no host sync between steps
                else:
                    for _ in range(n):
                        self.train(rollout_generator.sample(self.batch_size, self.device))
                steps_since_target_update += rollout_generator.train_freq
                if steps_since_target_update >= self.target_update_interval:
                    self._update_target()
                    steps_since_target_update = 0
            if self.tb_writer is not None and hasattr(self.tb_writer, "on_steps"):
                self.tb_writer.on_steps(rollout_steps)
            if callbacks and not all(c.on_step(timesteps_elapsed=rollout_steps) for c in callbacks):
                logging.info(f"Callback terminated training at {timesteps_elapsed} timesteps")
                break
        return self

    def train(self, batch: Batch) -> None:
        """One gradient step on an explicit batch (un-captured)."""
        self.policy.train(True)
        o, a, r, d, next_o = batch
        if not self.on_device:
            with torch.no_grad():
                target = r + ~d * self.gamma * self.target_q_net(next_o).max(1).values
            current = self.policy.q_net(o).gather(dim=1, index=a.unsqueeze(1)).squeeze(1)
            loss = F.smooth_l1_loss(current, target)
            self.optimizer.zero_grad()
            loss.backward()
            if self.max_grad_norm:
                self.last_grad_norm = nn.utils.clip_grad_norm_(self.policy.q_net.parameters(), self.max_grad_norm)
            self.optimizer.step()
            self.last_targets, self.last_loss = target, loss.detach()
            return
        self._step(o, a, r, _u8(d), next_o)
        self.optimizer.step_count += 1

    def _update_target(self) -> None:
        self.target_updates += 1
        if self.on_device:
            polyak_update(self.target_flat.flat, self.flat.flat, self.tau)
            return
        for target_param, param in zip(self.target_q_net.parameters(), self.policy.q_net.parameters()):
            target_param.data.copy_(self.tau * param.data + (1 - self.tau) * target_param.data)

    def save(self, path: str) -> None:
        save_optimizer(self.optimizer, path)

    def load(self, path: str) -> None:
        load_optimizer(self.optimizer, path, self.device)
        if self.on_device:
            self._sync_train_state()

    # -- the device step -----------------------------------------------------------------------------------
    def _loss_grads(self, o, a, r, d_u8, next_o) -> None:
        """Target forward, online forward, (fused head | TD loss), backward into the flat gradient."""
        from .cnn_ops import direct_grads

        q_net, t_net = self.policy.q_net, self.target_q_net
        head, t_head = q_net.head, t_net.head
        fused = self.fused_head and head_supported(head.in_features, head.out_features)
        with direct_grads(True):
            if fused:
                with torch.no_grad():
                    hn = t_net.trunk(next_o)
                h = q_net.trunk(o)
                hd = h.detach()
                target, loss, g = head_fwd(hd, hn, head.weight, head.bias, t_head.weight, t_head.bias, a, r, d_u8,
                                           self.gamma)
                dh, _, _ = head_bwd(hd, head.weight, a, g, head.weight.grad, head.bias.grad)
                if h.requires_grad:
                    h.backward(dh)
            else:
                with torch.no_grad():
                    qn = t_net(next_o)
                q = q_net(o)
                target, loss, dq = td_loss(q.detach(), qn, a, r, d_u8, self.gamma)
                q.backward(dq)
        self.last_targets, self.last_loss = target, loss

    def _step(self, o, a, r, d_u8, next_o) -> None:
        self.flat.check_views()
        self._loss_grads(o, a, r, d_u8, next_o)
        self._norm_index.zero_()  # one norm slot, rewritten every step
        self.optimizer.step(self.state_dev, self.norms, count=False)
        self.last_grad_norm = self.norms[0]

    def train_sampled(self, ring, n_steps: int = 1, positions=None) -> None:
        """n_steps gradient steps, each on a fresh device-side draw from `ring` (or, with `positions`
        (n_steps, B) deque positions, on injected draws): after WARMUP eager steps the whole step
        (sample + gather -> forwards -> loss -> backward -> clip + Adam) is captured once and replayed."""
        assert self.on_device and ring.on_device
        self.policy.train(True)
        B = self.batch_size
        if B > len(ring):
            raise ValueError("Sample larger than population")
        inject = None
        if positions is not None:
            positions = np.asarray(positions, dtype=np.int64).reshape(n_steps, B)
            assert positions.min() >= 0 and positions.max() < len(ring)
            host = torch.from_numpy(positions)
        key = (id(ring), B, positions is not None, self.fused_head)
        st = self._graphs.get(key)
        if st is None:
            st = self._graphs[key] = dict(graph=None, eager=0, ring=ring,
                                          inject=torch.zeros(B, dtype=torch.int64, device=self.device))
        if positions is not None:
            inject = st["inject"]

        def body():
            ring.launch_sample(B, inject, count=False)
            obs, nobs, act, rew, done, _ = ring.batch_buffers(B)
            self._step(obs, act, rew, done, nobs)

        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            for i in range(n_steps):
                if inject is not None:
                    inject.copy_(host[i], non_blocking=False)
                if st["graph"] is not None:
                    st["graph"].replay()
                elif st["eager"] < self.WARMUP:
                    body()
                    st["eager"] += 1
                else:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=self.stream):
                        body()
                    st["graph"] = g
                    g.replay()  # the capture executed nothing: this replay is the step
        cur.wait_stream(self.stream)
        self.optimizer.step_count += n_steps
        if positions is None:
            ring.count_draws(n_steps)
