"""PPO's freeze_policy_head / freeze_value_head / freeze_backbone without a GPU: the constructor and the
attributes HyperparamTransitions sets, the optimizer's run table and per-parameter checkpoint steps, the
rejected cases, and the fixture the reference itself wrote (tests/golden/make_golden_freeze.py ->
freeze_steps.npz)."""
from __future__ import annotations

import json

import numpy as np
import pytest
import torch

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.callbacks import HyperparamTransitions
from rl_algo_impls_amd.envs import SyntheticVecEnv
from rl_algo_impls_amd.optim import FlatOptimizer, FlatParams
from rl_algo_impls_amd.policy import ActorCritic
from rl_algo_impls_amd.ppo import PPO
from test_impala_cpu import impala_policy
from test_teacher_kl_cpu import step_policy

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("freeze_steps.npz")
    return z, json.loads(str(z["index"]))


def cartpole_policy():
    torch.manual_seed(1)
    return ActorCritic(SyntheticVecEnv(4, "cartpole", seed=1))


def groups_of(pol):
    """(name, first parameter index, one past the last) per parameter group, parameters() order."""
    idx = {id(p): i for i, p in enumerate(pol.parameters())}
    net = pol.network
    mods = ((("backbone", net.backbone), ("actor", net.actor_head), ("critic", net.critic_heads)) if pol.gridnet else
            (("backbone", net._feature_extractor), ("actor", net._pi), ("critic", net._v)))
    out = []
    for name, m in mods:
        ids = sorted(idx[id(p)] for p in m.parameters())
        if ids:
            assert ids == list(range(ids[0], ids[-1] + 1)), f"{name}: parameters not contiguous"
            out.append((name, ids[0], ids[-1] + 1))
    return sorted(out, key=lambda g: g[1])


def test_constructor_takes_the_flags_and_keeps_them_as_attributes():
    algo = PPO(cartpole_policy(), CPU, None, freeze_backbone=True)  # raised NotImplementedError before
    assert (algo.freeze_policy_head, algo.freeze_value_head, algo.freeze_backbone) == (False, False, True)
    algo = PPO(cartpole_policy(), CPU, None)
    assert (algo.freeze_policy_head, algo.freeze_value_head, algo.freeze_backbone) == (False, False, False)


@pytest.mark.parametrize("kw", [dict(switch_range=1), dict(guide_probability=0.5), dict(autocast_loss=True)])
def test_other_options_are_still_rejected(kw):
    with pytest.raises(NotImplementedError):
        PPO(cartpole_policy(), CPU, None, **kw)


def test_hyperparam_transitions_switch_the_flags():
    algo = PPO(cartpole_policy(), CPU, None)
    phases = [dict(freeze_policy_head=True, freeze_backbone=True, learning_rate=1e-3),
              dict(freeze_policy_head=False, freeze_backbone=False, learning_rate=1e-4)]
    cb = HyperparamTransitions(None, None, algo, None, phases, [0.4, 0.2, 0.4], total_train_timesteps=100)
    assert algo.freeze_policy_head is True and algo.freeze_backbone is True and algo.freeze_value_head is False
    cb.on_step(timesteps_elapsed=50)  # inside the transition: a bool keeps the prior phase's value
    assert algo.freeze_policy_head is True and algo.freeze_backbone is True
    cb.on_step(timesteps_elapsed=20)
    assert algo.freeze_policy_head is False and algo.freeze_backbone is False
    assert algo.learning_rate == 1e-4


def expected_runs(pol, flat, frozen_groups, lags):
    out = []
    for name, a, b in groups_of(pol):
        begin = flat.offsets[a]
        end = flat.offsets[b - 1] + flat.params[b - 1].numel()
        row = [begin, end, lags.get(name, 0), 0 if name in frozen_groups else 1]
        if out and out[-1][2:] == row[2:]:
            out[-1][1] = end
        else:
            out.append(row)
    return [tuple(r) for r in out]


def squnet_policy():
    from test_squnet import C5_KW

    torch.manual_seed(3)
    env = SyntheticVecEnv(2, kind="microrts", obs_pool=2)
    return ActorCritic(env, actor_head_style="squeeze_unet", channels_per_level=[16, 16, 16],
                       **{k: v for k, v in C5_KW.items() if k != "init_layers_orthogonal"})


@pytest.mark.parametrize("make", [cartpole_policy,
                                  lambda: impala_policy(dict(obs_shape=[3, 20, 12], n_actions=15, policy=dict(
                                      activation_fn="relu", cnn_style="impala", cnn_flatten_dim=256))),
                                  squnet_policy], ids=["mlp", "impala", "squnet_gridnet"])
def test_runs_merge_the_frozen_mask_and_the_lags(make):
    pol = make()
    flat = FlatParams(pol, CPU)
    opt = FlatOptimizer(flat, FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    names = [g[0] for g in groups_of(pol)]
    assert ("backbone" in names) == (len(names) == 3)  # the MLP's Flatten backbone has no parameters
    assert opt.uniform() and opt.runs() == [(0, flat.P, 0, 1)]
    pol.freeze(True, False, True)
    opt.set_frozen([not p.requires_grad for p in flat.params])
    assert opt.runs() == expected_runs(pol, flat, {"backbone", "actor"}, {})
    assert len(opt.runs()) == 2 and not opt.uniform()
    opt.step_count = 6
    opt.account(6)
    pol.unfreeze()
    opt.set_frozen([not p.requires_grad for p in flat.params])
    lags = dict(backbone=6, actor=6)
    assert opt.runs() == expected_runs(pol, flat, set(), lags) and len(opt.runs()) == 2
    pol.freeze(False, True, False)
    opt.set_frozen([not p.requires_grad for p in flat.params])
    assert opt.runs() == expected_runs(pol, flat, {"critic"}, lags)
    runs = opt.runs()
    assert runs[0][0] == 0 and runs[-1][1] == flat.P and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
    assert opt._n_runs == len(runs)


def test_more_runs_than_the_table_holds_are_refused():
    n = _lib.RAI_OPTIM_MAX_RUNS + 1
    mod = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(3)) for _ in range(n)])
    opt = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    with pytest.raises(NotImplementedError, match=str(n)):
        opt.set_frozen([i % 2 == 1 for i in range(n)])
    opt2 = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    opt2.set_frozen([i % 2 == 1 for i in range(n - 1)] + [True])  # 64 runs: the limit itself is fine
    assert len(opt2.runs()) == _lib.RAI_OPTIM_MAX_RUNS


def torch_adam_checkpoint(equal_steps: bool):
    """A real torch.optim.Adam stepped on the CPU with some .grad = None for some steps (one parameter never
    stepped: no entry), and the module it stepped."""
    torch.manual_seed(5)
    mod = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Linear(8, 3), torch.nn.Linear(3, 1, bias=False))
    ps = list(mod.parameters())
    opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-7)
    skip = {0: (), 1: (0, 1), 2: (0,), 3: (0, 1, 2), 4: (0, 1, 2, 3, 4, 5)}  # parameter -> steps it sits out
    for s in range(6):
        for i, p in enumerate(ps):
            p.grad = None if (not equal_steps and s in skip[i]) else torch.randn_like(p)
        opt.step()
    return mod, opt.state_dict()


def test_checkpoint_with_differing_steps_round_trips():
    mod, sd = torch_adam_checkpoint(equal_steps=False)
    assert sorted(sd["state"]) == [0, 1, 2, 3] and [int(sd["state"][i]["step"]) for i in range(4)] == [6, 4, 5, 3]
    opt = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    opt.state1.fill_(9.0)  # (a missing entry means zero moments, whatever the buffers held)
    opt.load_state_dict(sd)  # raised "per-parameter step counts differ" before
    assert opt.step_count == 6 and opt.lag.tolist() == [0, 2, 1, 3, 6]
    assert opt.param_groups[0]["lr"] == 3e-4
    out = opt.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"])
    for i, s in sd["state"].items():
        assert float(out["state"][i]["step"]) == float(s["step"])
        assert torch.equal(out["state"][i]["exp_avg"], s["exp_avg"])
        assert torch.equal(out["state"][i]["exp_avg_sq"], s["exp_avg_sq"])
    n4 = opt.flat.offsets[4]
    assert not opt.state1[n4:].any() and not opt.state2[n4:].any()
    assert len(opt.runs()) == 5 and not opt.uniform()


def test_checkpoint_with_equal_steps_keeps_the_format():
    mod, sd = torch_adam_checkpoint(equal_steps=True)
    opt = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    opt.load_state_dict(sd)
    assert opt.step_count == 6 and opt.uniform() and opt._n_runs == 0
    out = opt.state_dict()
    assert sorted(out["state"]) == list(range(5))
    for i in range(5):  # what tests/test_flat_params.py expects of an entry: torch's keys, layout and dtype
        s = out["state"][i]
        assert list(s) == ["step", "exp_avg", "exp_avg_sq"] and float(s["step"]) == 6.0
        assert s["step"].dtype == torch.float32 and s["step"].dim() == 0
        assert s["exp_avg"].is_contiguous() and torch.equal(s["exp_avg"], sd["state"][i]["exp_avg"])
    assert out["param_groups"][0]["params"] == list(range(5))
    fresh = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
    assert fresh.state_dict()["state"] == {}


class NoRollout:
    total_steps = 40

    def num_minibatches(self, batch_size):
        return 3


def test_everything_frozen_and_data_parallel_are_rejected():
    algo = PPO(cartpole_policy(), CPU, None, freeze_policy_head=True, freeze_value_head=True, freeze_backbone=True)
    with pytest.raises(ValueError, match="frozen"):
        algo.update(NoRollout())
    assert all(p.requires_grad for p in algo.policy.parameters()), "unfreeze() ran"
    algo = PPO(cartpole_policy(), CPU, None, freeze_value_head=True)
    algo.world = 2
    with pytest.raises(NotImplementedError, match="data parallel"):
        algo.update(NoRollout())
    algo = PPO(cartpole_policy(), CPU, None)
    algo.world = 2
    algo.optimizer.step_count = 6
    algo.optimizer.lag[:6] = 6
    with pytest.raises(NotImplementedError, match="data parallel"):
        algo.update(NoRollout())


def test_a_policy_with_uneven_steps_leaves_the_whole_epoch_kernels():
    algo = PPO(cartpole_policy(), CPU, None)
    assert algo.fused_mlp_spec() is not None
    algo.freeze_value_head = True
    assert algo.fused_mlp_spec() is None
    algo.freeze_value_head = False
    assert algo.fused_mlp_spec() is not None
    algo.optimizer.step_count = 6
    algo.optimizer.lag[:6] = 6
    assert algo.fused_mlp_spec() is None and algo._fused_kernels_off()


def test_fixture_frozen_tensors_stay_and_steps_follow_the_updates(fx):
    z, index = fx
    meta = index["cat"]
    sizes = [int(np.prod(s)) for s in meta["shapes"]]
    cut = np.cumsum([0] + sizes)
    flag_of = dict(actor="freeze_policy_head", critic="freeze_value_head", backbone="freeze_backbone")
    per = index["steps_per_update"]
    assert per == index["epochs"] * -(-index["T"] * index["N"] // index["batch"]) == 6
    steps = np.zeros(len(sizes))
    for u, flags in enumerate(index["updates"]):
        for suffix in ("", "_f32"):
            prev = z["cat_init"] if u == 0 else z["cat_params" + suffix][u - 1]
            cur = z["cat_params" + suffix][u]
            for j, g in enumerate(meta["groups"]):
                same = np.array_equal(cur[cut[j]:cut[j + 1]], prev[cut[j]:cut[j + 1]].astype(cur.dtype))
                assert same == flags[flag_of[g]], (u, j, suffix)
        steps += [0 if flags[flag_of[g]] else per for g in meta["groups"]]
        assert np.array_equal(z["cat_steps"][u], steps), u
        assert np.array_equal(z["cat_has_state"][u], steps > 0), u
    by_group = {g: {int(s) for s, gg in zip(z["cat_steps"][-1], meta["groups"]) if gg == g} for g in ("actor", "critic")}
    assert by_group == dict(actor={12}, critic={12})
    after_a = {g: {bool(h) for h, gg in zip(z["cat_has_state"][0], meta["groups"]) if gg == g} for g in ("actor", "critic")}
    assert after_a == dict(actor={False}, critic={True}) and set(z["cat_steps"][0][6:]) == {6.0}
    assert len(z["cat_loss"]) == len(z["cat_norms"]) == per * len(index["updates"])
    assert index["cat"]["single_step_ratio"] > 100
    pol = step_policy(meta, z["cat_init"])
    assert [g[0] for g in groups_of(pol)] == ["actor", "critic"]


def test_steps_taken_before_a_failed_update_are_accounted_for():
    algo = PPO(cartpole_policy(), CPU, None, freeze_policy_head=True)

    def broken(r):
        algo.optimizer.step_count += 2  # two optimizer steps ran, then the update raised
        raise RuntimeError("boom")

    algo._update = broken
    with pytest.raises(RuntimeError, match="boom"):
        algo.update(NoRollout())
    opt = algo.optimizer
    assert opt.step_count == 2 and opt.lag.tolist() == [2] * 6 + [0] * 6 and not opt.frozen.any()
    assert sorted(opt.state_dict()["state"]) == list(range(6, 12)), "the frozen actor is still at step 0"
    assert all(p.requires_grad for p in algo.policy.parameters())


def test_only_ppo_continues_from_a_checkpoint_with_differing_steps(tmp_path):
    from rl_algo_impls_amd.pg_common import load_optimizer, save_optimizer

    for equal in (False, True):
        mod, sd = torch_adam_checkpoint(equal_steps=equal)
        src = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
        src.load_state_dict(sd)
        d = tmp_path / str(equal)
        d.mkdir()
        save_optimizer(src, str(d))
        dst = FlatOptimizer(FlatParams(mod, CPU), FlatOptimizer.ADAM, lr=1e-3, eps=1e-7)
        if equal:
            load_optimizer(dst, str(d), CPU)  # A2C / ACBC / DQN's call
            assert dst.step_count == 6 and dst.uniform()
        else:
            with pytest.raises(NotImplementedError, match="per-parameter step"):
                load_optimizer(dst, str(d), CPU)
            assert dst.step_count == 0 and dst.uniform(), "refused before anything was loaded"
            load_optimizer(dst, str(d), CPU, per_parameter_steps=True)  # PPO's call
            assert dst.step_count == 6 and not dst.uniform()
