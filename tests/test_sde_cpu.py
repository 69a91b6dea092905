"""The gSDE actor head (use_sde, squash_output) without a GPU: the module tree, the plain-torch head and the
policy plumbing against the fixture the reference itself wrote (tests/golden/make_golden_sde.py ->
sde_steps.npz).  Tolerance everywhere: max(1e-5 |ref|, 4 x the fixture's own |f32 - f64|), the rule of
tests/test_dqn_cpu.py."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rl_algo_impls_amd.envs import Box
from rl_algo_impls_amd.policy import (ActorCritic, GaussianActorHead, StateDependentNoiseActorHead, clamp_actions,
                                      mlp_actor_critic_spec)

sys.path.insert(0, str(GOLDEN))
from make_golden_sde import sde_init  # noqa: E402  (numpy-only recipe, no reference import)

CASES = ["full", "squash"]


class SpaceEnv:
    def __init__(self, num_envs, obs_space, act_space):
        self.num_envs = num_envs
        self.single_observation_space = obs_space
        self.single_action_space = act_space
        self.unwrapped = self


def case_env(meta, n=1, low=-1.0, high=1.0):
    return SpaceEnv(n, Box(-np.inf, np.inf, (meta["obs_dim"],), np.float32),
                    Box(low, high, (meta["act_dim"],), np.float32))


def case_policy(meta, device=torch.device("cpu")):
    torch.manual_seed(7)
    pol = ActorCritic(case_env(meta), **meta["policy"])
    flat = sde_init(meta["shapes"], meta["log_std_index"], meta["policy"]["log_std_init"])
    off = 0
    with torch.no_grad():
        for p in pol.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(flat[off:off + n]).reshape(p.shape))
            off += n
    return pol.to(device)


def tol(ref, err, rtol=1e-5):
    """max(rtol * |ref|, 4 x the fixture's own |f32 - f64|)"""
    return np.maximum(rtol * np.abs(ref), 4 * np.asarray(err, np.float64))


def per_tensor(err, shapes):
    """A per-tensor bound spread over the flat parameter vector."""
    return np.concatenate([np.full(int(np.prod(s)), e, np.float64) for s, e in zip(shapes, err)])


def assert_close(got, ref, err, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d, bound = np.abs(got - ref), tol(ref, err)
    assert (d <= bound).all(), (what, float((d / bound).max()), float(d.max()))


def flat_params(pol):
    return torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu().numpy()


def flat_grads(pol):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                      for p in pol.parameters()]).cpu().numpy()


def check_forward_and_grads(pol, z, meta, name, device):
    for B in json.loads(str(z["index"]))["fwd_B"]:
        P = f"{name}_fwd{B}_"
        t = lambda k: torch.from_numpy(z[P + k]).to(device)
        pol.zero_grad(set_to_none=True)
        lp, ent, v = pol(t("obs"), t("actions"))
        assert lp.shape == ent.shape == v.shape == (B,)
        for k, got in (("logp", lp), ("entropy", ent), ("v", v)):
            assert_close(got.detach().cpu().numpy(), z[P + k], z[P + "err_" + k], (name, B, k))
        w = t("w")
        (w[:, 0] * lp + w[:, 1] * ent + w[:, 2] * v).sum().backward()
        assert_close(flat_grads(pol), z[P + "grads"], per_tensor(z[P + "err_grads"], meta["shapes"]), (name, B, "grads"))


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("sde_steps.npz")
    return z, json.loads(str(z["index"]))


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_reference_and_loads_strictly(fx, name):
    _, index = fx
    meta = index[name]
    pol = ActorCritic(case_env(meta), **meta["policy"])
    assert [[k, list(v.shape)] for k, v in pol.state_dict().items()] == meta["state_dict"]
    assert [list(p.shape) for p in pol.parameters()] == meta["shapes"]
    pol.load_state_dict({k: torch.full(s, 0.5) for k, s in meta["state_dict"]}, strict=True)
    pi = pol.network._pi
    assert isinstance(pi, StateDependentNoiseActorHead) and pol.use_sde
    assert pi.full_std == meta["policy"]["full_std"] and pi.squash_output == meta["policy"]["squash_output"]
    assert isinstance(pi.latent_net, torch.nn.Sequential) and isinstance(pi.mu_net, torch.nn.Sequential)


def test_identity_latent_net_and_initialisation():
    """No hidden layers: latent_net is Identity and log_std has the encoder's width; log_std starts at
    log_std_init, mu_net at gain 0.01, and the constructor draws the exploration matrices."""
    env = SpaceEnv(3, Box(-np.inf, np.inf, (5,), np.float32), Box(-1.0, 1.0, (2,), np.float32))
    torch.manual_seed(0)
    pol = ActorCritic(env, pi_hidden_sizes=[], use_sde=True, full_std=False, log_std_init=-1.5)
    pi = pol.network._pi
    assert isinstance(pi.latent_net, torch.nn.Identity) and tuple(pi.log_std.shape) == (5, 1)
    assert torch.equal(pi.log_std.detach(), torch.full((5, 1), -1.5))
    w = pi.mu_net[0].weight.detach()
    np.testing.assert_allclose((w @ w.T).numpy(), 1e-4 * np.eye(2), atol=1e-9)  # orthogonal rows, gain 0.01
    assert tuple(pi.exploration_mat.shape) == (5, 2) and tuple(pi.exploration_matrices.shape) == (1, 5, 2)
    assert "exploration_mat" not in "".join(pol.state_dict())


@pytest.mark.parametrize("name", CASES)
def test_cpu_forward_and_gradients_match_reference(fx, name):
    z, index = fx
    check_forward_and_grads(case_policy(index[name]), z, index[name], name, torch.device("cpu"))


def cpu_steps(pol, z, name, meta):
    """The PPO / A2C minibatch step on the CPU (the trainer classes drive HIP kernels and take a GPU only):
    rl_algo_impls/ppo/ppo.py:299-371 and rl_algo_impls/a2c/a2c.py:116-164,202-205 over this repo's policy."""
    kw = meta["kw"]
    ppo = meta["algo"] == "ppo"
    if ppo:
        opt = torch.optim.Adam(pol.parameters(), lr=kw["learning_rate"], eps=1e-7)
    else:
        opt = torch.optim.RMSprop(pol.parameters(), lr=kw["learning_rate"], eps=1e-5)
    loss_rows, norms, params = [], [], []
    for i in range(meta["n"]):
        t = lambda f: torch.from_numpy(z[f"{name}_b{i}_{f}"])
        obs, act, adv, ret = t("obs"), t("actions"), t("advantages"), t("returns")
        lp, ent, v = pol(obs, act)
        if ppo:
            adv = (adv - adv.mean(0)) / (adv.std(0) + 1e-8)
            ratio = torch.exp(lp - t("logprobs"))
            clip = kw["clip_range"]
            pi_loss = -torch.min(ratio * adv, torch.clamp(ratio, min=1 - clip, max=1 + clip) * adv).mean()
        else:
            pi_loss = -(adv * lp).mean()
        v_loss = ((v - ret) ** 2).mean(0)
        loss = pi_loss + kw["ent_coef"] * -ent.mean() + kw["vf_coef"] * v_loss
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)))
        opt.step()
        opt.zero_grad(set_to_none=True)
        loss_rows.append(float(loss.detach()))
        params.append(flat_params(pol))
    return np.array(loss_rows), np.array(norms), np.stack(params)


@pytest.mark.parametrize("name", CASES)
def test_cpu_update_steps_match_reference(fx, name):
    z, index = fx
    meta = index[name]
    loss, norms, params = cpu_steps(case_policy(meta), z, name, meta)
    assert_close(loss, z[f"{name}_loss"], z[f"{name}_err_loss"], (name, "loss"))
    assert_close(norms, z[f"{name}_norms"], z[f"{name}_err_norms"], (name, "norms"))
    for i in range(meta["n"]):
        assert_close(params[i], z[f"{name}_params"][i], per_tensor(z[f"{name}_err_params"][i], meta["shapes"]),
                     (name, "params", i))


def test_constructor_accepts_sde_and_rejects_squash_alone(fx):
    _, index = fx
    env = case_env(index["full"])
    assert isinstance(ActorCritic(env, use_sde=True).network._pi, StateDependentNoiseActorHead)
    assert isinstance(ActorCritic(env, use_sde=True, squash_output=True).network._pi, StateDependentNoiseActorHead)
    assert isinstance(ActorCritic(env).network._pi, GaussianActorHead)
    with pytest.raises(AssertionError, match="squash_output only valid if use_sde"):
        ActorCritic(env, squash_output=True)


def test_fused_mlp_specs_stay_none_for_gsde():
    """Both whole-network kernel families key on the head's class: a gSDE policy takes the generic path."""
    from rl_algo_impls_amd.mlp_wide import wide_mlp_spec

    env = SpaceEnv(1, Box(-np.inf, np.inf, (5,), np.float32), Box(-1.0, 1.0, (3,), np.float32))
    kw = dict(pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64])
    assert wide_mlp_spec(ActorCritic(env, **kw)) is not None  # the same shape with the Gaussian head qualifies
    pol = ActorCritic(env, use_sde=True, **kw)
    assert wide_mlp_spec(pol) is None and mlp_actor_critic_spec(pol) is None


def test_step_act_and_reset_noise(fx):
    _, index = fx
    meta = index["squash"]
    env = case_env(meta, n=4, low=-3.0, high=2.0)
    pol = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    pi = pol.network._pi
    pol.reset_noise()  # defaults to env.num_envs
    assert tuple(pi.exploration_matrices.shape) == (4, 20, 3)
    e_before = pi.exploration_matrices.clone()
    pol.reset_noise(7)
    assert tuple(pi.exploration_matrices.shape) == (7, 20, 3)
    pol.reset_noise()
    assert not torch.equal(pi.exploration_matrices, e_before)
    obs = np.random.default_rng(0).standard_normal((4, 5)).astype(np.float32)
    with torch.no_grad():
        (mu, latent), v = pol.network.dist_params_and_value(torch.from_numpy(obs))
    s = pol.step(obs)
    # the batch matches the matrices: row n uses matrix n; squashed and rescaled to the bounds
    want = torch.tanh(mu + torch.bmm(latent.unsqueeze(1), pi.exploration_matrices).squeeze(1)).numpy()
    np.testing.assert_array_equal(s.a, want)
    np.testing.assert_array_equal(s.clamped_a, -3.0 + 0.5 * (want + 1) * 5.0)
    np.testing.assert_array_equal(s.v, v.numpy())
    with torch.no_grad():
        lp = pol(torch.from_numpy(obs), torch.from_numpy(s.a)).logp_a.numpy()
    np.testing.assert_array_equal(s.logp_a, lp)
    # another batch size: the one shared matrix (the forward redone at that size: a GEMM's rounding may
    # depend on its row count)
    s3 = pol.step(obs[:3])
    with torch.no_grad():
        (mu3, latent3), _ = pol.network.dist_params_and_value(torch.from_numpy(obs[:3]))
    np.testing.assert_array_equal(s3.a, torch.tanh(mu3 + latent3 @ pi.exploration_mat).numpy())
    # deterministic: mode = tanh(mu), rescaled
    np.testing.assert_array_equal(pol.act(obs), -3.0 + 0.5 * (torch.tanh(mu).numpy() + 1) * 5.0)


def test_load_and_load_from_reset_the_noise(fx, tmp_path):
    _, index = fx
    meta = index["full"]
    env = case_env(meta, n=3)
    a = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    b = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    a.save(str(tmp_path))
    e0 = b.network._pi.exploration_mat.clone()
    b.load(str(tmp_path))
    assert tuple(b.network._pi.exploration_matrices.shape) == (3, 64, 3)
    assert not torch.equal(b.network._pi.exploration_mat, e0)
    e1 = b.network._pi.exploration_mat.clone()
    assert b.load_from(a) is b and not torch.equal(b.network._pi.exploration_mat, e1)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_clamp_actions_rescales_when_squashing():
    space = Box(low=np.array([-3.0, 0.0], np.float32), high=np.array([2.0, 10.0], np.float32))
    a = np.array([[-1.0, -1.0], [0.0, 0.5], [1.0, 1.0]], np.float32)
    np.testing.assert_array_equal(clamp_actions(a, space, True), np.array([[-3, 0], [-0.5, 7.5], [2, 10]], np.float32))
    np.testing.assert_array_equal(clamp_actions(a * 20, space, False), np.array([[-3, 0], [0, 10], [2, 10]], np.float32))


def test_rollout_generator_signature_accepts_sde_sample_freq():
    """(The generator itself allocates pinned host memory and HIP events, so it is constructed in
    tests/test_gpu_sde.py; here: the keyword is a parameter and no longer listed as unsupported.)"""
    import inspect

    from rl_algo_impls_amd import rollout

    inspect.signature(rollout.SyncStepRolloutGenerator).bind(object(), object(), n_steps=8, sde_sample_freq=4)
    assert "sde_sample_freq" not in rollout._UNSUPPORTED_GEN_KW
