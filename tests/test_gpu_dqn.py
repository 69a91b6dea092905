"""DQN on the device: the reference's fixture steps (tests/golden/make_golden_dqn.py -> dqn_steps.npz)
through DQN.train with the fused head and the unfused path, the captured-graph step against the
un-captured one, and the learn loop's mechanics on CartPoleVecEnv."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from rl_algo_impls_amd.dqn import DQN, DQNPolicy
from rl_algo_impls_amd.envs import CartPoleVecEnv
from rl_algo_impls_amd.replay import ReplayBufferRolloutGenerator
from test_dqn_cpu import case_batches, case_env, load_init, per_tensor_max

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("dqn_steps.npz")
    return z, json.loads(str(z["index"]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused-head", "unfused"])
@pytest.mark.parametrize("name", ["mlp", "impala"])
def test_fixture_steps(fx, name, fused):
    """Tolerances: max(rtol 1e-5, 4 x the fixture's own |f32 - f64| of the quantity) (the reference rerun in
    float64 from the same bits), as test_gpu_impala.py widens its base tolerances; the worst ratio
    |got - ref| / tolerance per quantity is printed."""
    z, index = fx
    meta = index[name]
    policy = DQNPolicy(case_env(meta), **meta["policy"])
    init = load_init(policy, meta["shapes"])
    policy.to(DEV)
    algo = DQN(policy, DEV, None, fused_head=fused, **meta["algo"])
    worst = {}

    def check(key, got, ref, err):
        tol = np.maximum(1e-5 * np.abs(ref), 4 * np.asarray(err))  # as tests/test_dqn_cpu.py's tol()
        ratio = float(np.max(np.abs(np.asarray(got, np.float64) - ref) / np.maximum(tol, 1e-300)))
        worst[key] = max(worst.get(key, 0.0), ratio)

    for i, b in enumerate(case_batches(z, name, meta, DEV)):
        algo.train(b)
        check("targets", algo.last_targets.cpu().numpy(), z[f"{name}_targets"][i].astype(np.float64),
              z[f"{name}_err_targets"][i])
        check("loss", float(algo.last_loss), z[f"{name}_loss"][i], z[f"{name}_err_loss"][i])
        check("norms", float(algo.last_grad_norm), z[f"{name}_norms"][i], z[f"{name}_err_norms"][i])
        if meta["update_after"] is not None and i + 1 == meta["update_after"]:
            algo._update_target()
    shapes = meta["shapes"]
    got = algo.flat.vector().cpu().numpy().astype(np.float64)
    d = per_tensor_max(got - z[f"{name}_params"], shapes)
    ptol = lambda key: np.maximum(1e-5 * per_tensor_max(z[f"{name}_{key}"], shapes), 4 * z[f"{name}_err_{key}"])
    worst["params"] = float(np.max(d / ptol("params")))
    tgt = algo.target_flat.vector(algo.target_flat.flat).cpu().numpy().astype(np.float64)
    if meta["update_after"] is not None:
        d = per_tensor_max(tgt - z[f"{name}_target_params"], shapes)
        worst["target_params"] = float(np.max(d / ptol("target_params")))
    else:
        np.testing.assert_array_equal(tgt.astype(np.float32), init)  # never updated
    m = per_tensor_max(got, shapes)  # optimizer moments: per-tensor norms
    for k, buf in (("opt_state1_norms", algo.optimizer.state1), ("opt_state2_norms", algo.optimizer.state2)):
        v = algo.flat.vector(buf).cpu().numpy().astype(np.float64)
        cut = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        norms = np.array([np.sqrt(np.sum(np.square(v[cut[j]:cut[j + 1]]))) for j in range(len(shapes))])
        check(k, norms, z[f"{name}_{k}"], z[f"{name}_err_{k}"])
    assert m.size and algo.optimizer.step_count == meta["steps"]
    print(f"dqn fixture {name} {'fused' if fused else 'unfused'}: worst |got - ref| / tolerance:",
          {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def _trainer(seed=0, **kw):
    env = CartPoleVecEnv(1, seed=seed)
    torch.manual_seed(seed)
    policy = DQNPolicy(env, hidden_sizes=[64, 64]).to(DEV)
    return env, policy, DQN(policy, DEV, None, learning_rate=1e-3, **kw)


def test_captured_step_equals_eager_train():
    """6 steps on the same injected draws: 2 eager warm-up steps, the capture, 3 replays; bit-equal parameters
    to six un-captured train(batch) calls."""
    B, steps = 16, 6
    np.random.seed(0)
    env, policy, algo = _trainer(batch_size=B)
    gen = ReplayBufferRolloutGenerator(policy, env, buffer_size=100, learning_starts=80, train_freq=4, seed=4)
    ring = gen.buffer
    pos = np.stack([np.random.default_rng(i).choice(len(ring), B, replace=False) for i in range(steps)])
    _, policy2, algo2 = _trainer(batch_size=B)
    assert torch.equal(algo.flat.flat, algo2.flat.flat)
    for p in pos:
        algo2.train(ring.sample(B, positions=p))
    algo.train_sampled(ring, steps, positions=pos)
    torch.cuda.synchronize()
    assert algo.optimizer.step_count == algo2.optimizer.step_count == steps
    assert torch.equal(algo.flat.flat, algo2.flat.flat)
    assert torch.equal(algo.optimizer.state2, algo2.optimizer.state2)
    assert ring.device_state()["err"] == 0


def _learn_run(device):
    np.random.seed(2)
    env = CartPoleVecEnv(1, seed=2)
    torch.manual_seed(2)
    policy = DQNPolicy(env, hidden_sizes=[64, 64]).to(device)
    algo = DQN(policy, device, None, batch_size=32, gradient_steps=4, target_update_interval=48,
               exploration_fraction=0.5, learning_rate=1e-3)
    gen = ReplayBufferRolloutGenerator(policy, env, buffer_size=256, learning_starts=64, train_freq=16, seed=1)
    steps = []

    class Count:
        def on_step(self, timesteps_elapsed=1):
            steps.append(timesteps_elapsed)
            return True

    total = 64 + 40 * 16
    algo.learn(total, gen, callbacks=[Count()], total_timesteps=total)
    return algo, gen, steps


def test_learn_mechanics_match_cpu_run():
    algo, gen, steps = _learn_run(DEV)
    torch.cuda.synchronize()
    cpu_algo, cpu_gen, cpu_steps = _learn_run(CPU)
    assert steps == cpu_steps == [16] * 40
    assert algo.target_updates == cpu_algo.target_updates == 40 * 16 // 48
    assert algo.optimizer.step_count == 40 * 4
    assert torch.isfinite(algo.flat.flat).all() and torch.isfinite(algo.target_flat.flat).all()
    st = gen.buffer.device_state()
    n = 64 + 40 * 16  # transitions pushed: the ring (256) wrapped
    assert (st["len"], st["head"], st["err"]) == (256, n % 256, 0)
    assert st["draws"] == 40 * 4 == gen.buffer.draws
    assert len(gen.buffer) == len(cpu_gen.buffer) == 256
