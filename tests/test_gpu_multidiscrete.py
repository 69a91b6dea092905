"""The MultiDiscrete actor head and flat action masks on the GPU through the module path:
ActorCritic over the head kernels (md_ops.MdHeadLogpEntropy), the real PPO and A2C classes and the rollout
generator with the synthetic masked env, against the fixture the reference itself wrote
(tests/golden/make_golden_multidiscrete.py -> multidiscrete_steps.npz).  Tolerance:
max(1e-5 |ref|, 4 x the fixture's own |f32 - f64|), as tests/test_multidiscrete_cpu.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rl_algo_impls_amd.a2c import A2C
from rl_algo_impls_amd.envs import MaskedMultiDiscreteVecEnv
from rl_algo_impls_amd.policy import ActorCritic
from rl_algo_impls_amd.ppo import PPO
from rl_algo_impls_amd.rollout import Batch, DeviceRollout, SyncStepRolloutGenerator
from test_multidiscrete_cpu import (CASES, assert_close, case_policy, check_forward_and_grads, flat_params, fx,  # noqa: F401
                                    masks_of, per_tensor)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("name", CASES)
def test_gpu_forward_and_gradients_match_reference(fx, name):
    z, index = fx
    pol = case_policy(index[name], DEV)
    from rl_algo_impls_amd import md_ops

    calls = []
    real = md_ops.MdHeadLogpEntropy.apply
    try:
        md_ops.MdHeadLogpEntropy.apply = lambda *a: (calls.append(1), real(*a))[1]
        check_forward_and_grads(pol, z, index[name], name, DEV)
    finally:
        md_ops.MdHeadLogpEntropy.apply = real
    want = len(index["fwd_B"]) if index[name]["nvec"] is not None else 0
    assert len(calls) == want, "the head kernels' autograd Function was (not) taken"


def test_fallback_routes_agree_with_the_fused_head(fx):
    """A non-contiguous head input takes torch's Linear and the GridNet operator with one cell; the plain torch
    formula on the device is the third route.  All three agree on the masked fixture batch to float32 accuracy."""
    from rl_algo_impls_amd import md_ops

    z, index = fx
    meta = index["md_masked"]
    pol = case_policy(meta, DEV)
    pi = pol.network._pi
    t = lambda k: torch.from_numpy(z["md_masked_fwd130_" + k]).to(DEV)
    with torch.no_grad():
        hidden = pi.params(pol.network._feature_extractor(t("obs")))
        fused = pi.logp_entropy(hidden, t("actions"), t("masks"))
        strided = torch.empty(130, 40, device=DEV)[:, ::2]
        strided.copy_(hidden)
        assert not md_ops.fusable(strided, pi.final, pi._sizes)
        grid = pi.logp_entropy(strided, t("actions"), t("masks"))
        plain = md_ops.logp_entropy_torch(pi.final(hidden), pi._sizes, t("actions"), t("masks"))
    for other in (grid, plain):
        for a, b in zip(fused, other):
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=2e-6)


def fixed_rollout(z, name, meta):
    """The case's n fixed minibatches as a (n, B, ...) device rollout whose epoch order is the identity:
    minibatch i of an epoch is fixture batch i, on the graphed and the eager update path alike."""
    t = lambda f: torch.stack([torch.from_numpy(z[f"{name}_b{i}_{f}"]) for i in range(meta["n"])]).to(DEV)
    masks = t("masks") if f"{name}_b0_masks" in z.files else None
    return DeviceRollout.from_fields(DEV, t("obs"), t("actions"), t("values"), t("advantages"), t("returns"),
                                     t("logprobs"), action_masks=masks,
                                     perm_source=lambda k: torch.arange(k, device=DEV))


@pytest.mark.parametrize("graphs", [True, False], ids=["graphed", "eager"])
@pytest.mark.parametrize("name", ["md", "cat_masked"])
def test_ppo_steps_match_reference(fx, name, graphs):
    z, index = fx
    meta = index[name]
    pol = case_policy(meta, DEV)
    algo = PPO(pol, DEV, None, n_epochs=1, **meta["kw"])
    algo.use_graphs = graphs
    r = fixed_rollout(z, name, meta)
    stats, norms, _ = algo.update(r)
    assert (algo._graphed is not None) == graphs, "update path"
    if name == "md":  # (the masked Categorical policy has the wide structure; its masks keep it off those kernels)
        assert algo._wide in (None, False), "a MultiDiscrete policy takes the per-minibatch path"
    assert_close(stats[:, 0], z[f"{name}_loss"], z[f"{name}_err_loss"], (name, "loss"))
    assert_close(norms, z[f"{name}_norms"], z[f"{name}_err_norms"], (name, "norms"))
    assert_close(flat_params(pol), z[f"{name}_params"][-1], per_tensor(z[f"{name}_err_params"][-1], meta["shapes"]),
                 (name, "params"))


def test_masked_discrete_policy_is_refused_by_the_whole_epoch_kernels(fx):
    """The same Categorical policy qualifies for the CartPole-class epoch kernel without masks; a rollout that
    carries masks must not reach it (the kernel has no mask input)."""
    z, index = fx
    meta = index["cat_masked"]
    pol = case_policy(meta, DEV)
    algo = PPO(pol, DEV, None, n_epochs=1, **meta["kw"])
    assert algo.fused_mlp_spec() is not None
    r = fixed_rollout(z, "cat_masked", meta)
    algo.kernel_events = []
    algo.update(r)
    assert algo.kernel_events == [] and algo._wide_epoch_step(r) is None


def test_a2c_steps_match_reference(fx):
    z, index = fx
    name = "md_masked"
    meta = index[name]
    pol = case_policy(meta, DEV)
    algo = A2C(pol, DEV, None, **meta["kw"])

    class OneBatch:
        def __init__(self, b):
            self.b, self.total_steps = b, len(b)

        def minibatches(self, bs, shuffle=True):
            return iter([self.b])

        def explained_variance(self):
            return float("nan")

    t = lambda i, f: torch.from_numpy(z[f"{name}_b{i}_{f}"]).to(DEV)
    rollouts = iter([OneBatch(Batch(t(i, "obs"), None, t(i, "actions"), t(i, "masks"), None, t(i, "values"),
                                    t(i, "advantages"), t(i, "returns"))) for i in range(meta["n"])])

    class Gen:
        def rollout(self, gamma, gae_lambda):
            return next(rollouts)

    rec = dict(loss=[], norms=[], params=[])

    class Record:
        def on_step(self, timesteps_elapsed):
            rec["loss"].append(algo.last_train_stats.data["loss"])
            rec["norms"].append(float(algo.blocks.norms[0]))
            rec["params"].append(flat_params(pol))
            return True

    algo.learn(meta["n"] * meta["B"], Gen(), callbacks=[Record()])
    assert_close(rec["loss"], z[f"{name}_loss"], z[f"{name}_err_loss"], (name, "loss"))
    assert_close(rec["norms"], z[f"{name}_norms"], z[f"{name}_err_norms"], (name, "norms"))
    for i in range(meta["n"]):
        assert_close(rec["params"][i], z[f"{name}_params"][i], per_tensor(z[f"{name}_err_params"][i], meta["shapes"]),
                     (name, "params", i))


def masked_generator(N=16, T=8, nvec=(3, 5, 2)):
    torch.manual_seed(5)
    env = MaskedMultiDiscreteVecEnv(N, nvec, seed=9)
    pol = ActorCritic(env, pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64]).to(DEV)
    with torch.no_grad():  # logits away from uniform, so a mask that is ignored shows in the actions
        pol.network._pi.final.weight.mul_(150.0)
    return env, pol, SyncStepRolloutGenerator(pol, env, n_steps=T, seed=11)


def test_rollout_masks_actions_and_first_ppo_pass():
    env, pol, gen = masked_generator()
    assert gen.multidiscrete and gen.fused_step is None and gen.action_masks.shape == (8, 16, 10)
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert r.total_steps == 128 and r.num_actions is None
    obs, masks, actions = gen.obs.cpu().numpy(), gen.action_masks.cpu().numpy(), gen.actions.cpu().numpy()
    assert actions.shape == (8, 16, 3) and actions.dtype == np.int64
    for s in range(8):  # the stored mask is the env's mask of the stored observation: not a step late
        np.testing.assert_array_equal(masks[s], env.mask_of(obs[s]))
    off = np.array([0, 3, 8])
    assert ((actions >= 0) & (actions < np.array([3, 5, 2]))).all()
    assert np.take_along_axis(masks, off + actions, axis=2).all(), "a stored action is masked"
    assert env.invalid_actions == 0, "the env received the actions unchanged"
    assert not masks.all() and np.unique(actions.reshape(-1, 3), axis=0).shape[0] > 4
    # the logged log-probabilities, recomputed step by step: bit for bit
    with torch.no_grad():
        for s in range(8):
            lp = pol(gen.obs[s], gen.actions[s], action_masks=gen.action_masks[s]).logp_a
            assert torch.equal(lp, gen.logprobs[s]), (s, float((lp - gen.logprobs[s]).abs().max()))
    assert gen.rng_offset == 8  # one sampler key per env step
    algo = PPO(pol, DEV, None, batch_size=32, n_epochs=1, learning_rate=3e-4, ent_coef=0.01)
    stats, norms, _ = algo.update(r)
    print(f"MultiDiscrete first PPO minibatch: approx_kl {stats[0, 3]!r} clipped_frac {stats[0, 4]!r}")
    assert np.isfinite(stats).all() and np.isfinite(norms).all()
    assert stats[0, 3] == 0.0 and stats[0, 4] == 0.0
    assert stats.shape[0] == 4 and stats[1, 3] != 0.0  # the second minibatch sees the stepped weights


def test_rollout_forward_is_one_graph_replay_plus_the_sample_launch():
    _, pol, gen = masked_generator(N=4, T=4)
    from rl_algo_impls_amd import md_ops

    calls = []
    real = md_ops.sample
    try:
        md_ops.sample = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        gen.rollout(gamma=0.99, gae_lambda=0.95)
    finally:
        md_ops.sample = real
    assert gen._fwd_graph is not None and len(calls) == 4


def test_masked_discrete_rollout_and_learn():
    """A masked Discrete env through the existing rai_categorical_sample mask argument, then PPO.learn and
    A2C.learn on the device for both kinds of policy."""
    from rl_algo_impls_amd.envs import Discrete

    class MaskedDiscreteEnv(MaskedMultiDiscreteVecEnv):  # one group of 6 presented as Discrete(6): (N,) actions
        def __init__(self, n):
            super().__init__(n, (6,), seed=4)
            self.single_action_space = Discrete(6)

    torch.manual_seed(2)
    env = MaskedDiscreteEnv(16)
    pol = ActorCritic(env).to(DEV)
    with torch.no_grad():
        pol.network._pi._fc[-2].weight.mul_(150.0)
    gen = SyncStepRolloutGenerator(pol, env, n_steps=8, seed=3)
    assert gen.fused_step is None, "the fused step kernel has no mask input"
    PPO(pol, DEV, None, batch_size=32, n_epochs=2, learning_rate=3e-4).learn(256, gen)
    masks, actions = gen.action_masks.cpu().numpy(), gen.actions.cpu().numpy()
    assert not masks.all() and np.take_along_axis(masks, actions[..., None], axis=2).all()
    assert env.invalid_actions == 0
    A2C(pol, DEV, None, learning_rate=7e-4).learn(128, gen)
    assert env.invalid_actions == 0 and all(torch.isfinite(p).all() for p in pol.parameters())
    # and the MultiDiscrete policy through both learn loops
    env2, pol2, gen2 = masked_generator()
    PPO(pol2, DEV, None, batch_size=32, n_epochs=2, learning_rate=3e-4).learn(256, gen2)
    A2C(pol2, DEV, None, learning_rate=7e-4).learn(128, gen2)
    assert env2.invalid_actions == 0 and all(torch.isfinite(p).all() for p in pol2.parameters())
