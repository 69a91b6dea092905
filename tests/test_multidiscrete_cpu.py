"""The MultiDiscrete actor head and flat action masks without a GPU: the module tree, the plain-torch head and
the policy plumbing against the fixture the reference itself wrote (tests/golden/make_golden_multidiscrete.py
-> multidiscrete_steps.npz).  Tolerance everywhere: max(1e-5 |ref|, 4 x the fixture's own |f32 - f64|), the
rule of tests/test_sde_cpu.py."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rl_algo_impls_amd.envs import Box, Discrete, MaskedMultiDiscreteVecEnv, MultiDiscrete
from rl_algo_impls_amd.policy import (ActorCritic, CategoricalActorHead, MultiDiscreteActorHead,
                                      mlp_actor_critic_spec)

sys.path.insert(0, str(GOLDEN))
from make_golden_pong import pong_init  # noqa: E402  (numpy-only recipe, no reference import)

CASES = ["md", "md_masked", "cat_masked", "md_w1"]
STEP_CASES = ["md", "md_masked", "cat_masked"]


class SpaceEnv:
    def __init__(self, num_envs, obs_space, act_space):
        self.num_envs = num_envs
        self.single_observation_space = obs_space
        self.single_action_space = act_space
        self.unwrapped = self


def case_env(meta, n=1):
    act = MultiDiscrete(meta["nvec"]) if meta["nvec"] is not None else Discrete(meta["n_act"])
    return SpaceEnv(n, Box(-np.inf, np.inf, (meta["obs_dim"],), np.float32), act)


def case_policy(meta, device=torch.device("cpu")):
    torch.manual_seed(7)
    pol = ActorCritic(case_env(meta), **meta["policy"])
    flat = pong_init([tuple(s) for s in meta["shapes"]])
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


RATIOS = {}  # what -> worst |got - ref| / bound seen (printed by the tests)


def assert_close(got, ref, err, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d, bound = np.abs(got - ref), tol(ref, err)
    ratio = float((d / bound).max())
    RATIOS[str(what)] = ratio
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert (d <= bound).all(), (what, ratio, float(d.max()))


def flat_params(pol):
    return torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).cpu().numpy()


def flat_grads(pol):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                      for p in pol.parameters()]).cpu().numpy()


def masks_of(z, key, device):
    return torch.from_numpy(z[key]).to(device) if key in z.files else None


def check_forward_and_grads(pol, z, meta, name, device):
    for B in json.loads(str(z["index"]))["fwd_B"]:
        P = f"{name}_fwd{B}_"
        t = lambda k: torch.from_numpy(z[P + k]).to(device)
        pol.zero_grad(set_to_none=True)
        lp, ent, v = pol(t("obs"), t("actions"), action_masks=masks_of(z, P + "masks", device))
        assert lp.shape == ent.shape == v.shape == (B,)
        for k, got in (("logp", lp), ("entropy", ent), ("v", v)):
            assert_close(got.detach().cpu().numpy(), z[P + k], z[P + "err_" + k], (name, B, k))
        w = t("w")
        (w[:, 0] * lp + w[:, 1] * ent + w[:, 2] * v).sum().backward()
        assert_close(flat_grads(pol), z[P + "grads"], per_tensor(z[P + "err_grads"], meta["shapes"]), (name, B, "grads"))


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("multidiscrete_steps.npz")
    return z, json.loads(str(z["index"]))


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_reference_and_loads_strictly(fx, name):
    _, index = fx
    meta = index[name]
    pol = ActorCritic(case_env(meta), **meta["policy"])  # the constructor no longer raises
    assert [[k, list(v.shape)] for k, v in pol.state_dict().items()] == meta["state_dict"]
    assert [list(p.shape) for p in pol.parameters()] == meta["shapes"]
    pol.load_state_dict({k: torch.full(s, 0.5) for k, s in meta["state_dict"]}, strict=True)
    pi = pol.network._pi
    if meta["nvec"] is not None:
        assert isinstance(pi, MultiDiscreteActorHead) and pol.is_multidiscrete and not pol.is_discrete
        assert pol.action_shape == (len(meta["nvec"]),) and pi.act_dim == sum(meta["nvec"])
        assert pi.final.out_features == sum(meta["nvec"])
    else:
        assert isinstance(pi, CategoricalActorHead) and pol.is_discrete and pol.action_shape == ()


def test_head_initialisation_and_rejected_styles():
    env = SpaceEnv(3, Box(-np.inf, np.inf, (5,), np.float32), MultiDiscrete([3, 5, 2]))
    torch.manual_seed(0)
    pol = ActorCritic(env, pi_hidden_sizes=[])
    w = pol.network._pi.final.weight.detach()  # (10, 5): orthogonal columns, gain 0.01
    np.testing.assert_allclose((w.T @ w).numpy(), 1e-4 * np.eye(5), atol=1e-9)
    assert torch.equal(pol.network._pi.final.bias.detach(), torch.zeros(10))
    for style in ("gridnet", "gridnet_decoder"):
        with pytest.raises(NotImplementedError, match="actor_head_style"):
            ActorCritic(env, actor_head_style=style)
    with pytest.raises(NotImplementedError):
        ActorCritic(env, share_features_extractor=False)


@pytest.mark.parametrize("name", CASES)
def test_cpu_forward_and_gradients_match_reference(fx, name):
    z, index = fx
    check_forward_and_grads(case_policy(index[name]), z, index[name], name, torch.device("cpu"))


def test_fixture_masks_hold_the_edge_rows(fx):
    """Row 0 fully valid, row 1 with one valid entry in its widest group, row 2 with an all-false first group."""
    z, index = fx
    for name in ("md_masked", "cat_masked", "md_w1"):
        groups = index[name]["nvec"] or [index[name]["n_act"]]
        off = np.concatenate([[0], np.cumsum(groups)])
        wide = int(np.argmax(groups))
        for B in index["fwd_B"]:
            m = z[f"{name}_fwd{B}_masks"]
            assert m[0].all() and m[1, off[wide]:off[wide + 1]].sum() == 1 and not m[2, off[0]:off[1]].any()
    assert "md_fwd7_masks" not in z.files


def test_all_false_group_contributes_nothing():
    """finfo.min + log n rounds back to finfo.min in float32: the group's normalised logits are 0, so its
    log-prob, entropy and gradient are 0 whatever the action (the reference's result, kept as it is)."""
    env = SpaceEnv(1, Box(-np.inf, np.inf, (5,), np.float32), MultiDiscrete([3, 5, 2]))
    torch.manual_seed(3)
    pol = ActorCritic(env, pi_hidden_sizes=[8], v_hidden_sizes=[8])
    pi = pol.network._pi
    with torch.no_grad():
        pi.final.weight.mul_(100.0)  # logits far from uniform
    obs = torch.randn(4, 5)
    mask = torch.ones(4, 10, dtype=torch.bool)
    mask[:, 3:8] = False  # group 1 all false
    act = torch.tensor([[0, 0, 1], [1, 4, 0], [2, 2, 1], [0, 3, 0]])
    hidden = pi.params(pol.network._feature_extractor(obs))
    logits = pi.final(hidden).detach().requires_grad_()
    from rl_algo_impls_amd.md_ops import logp_entropy_torch

    lp, ent = logp_entropy_torch(logits, [3, 5, 2], act, mask)
    two = torch.cat([logits[:, :3], logits[:, 8:]], dim=1)
    lp2, ent2 = logp_entropy_torch(two, [3, 2], act[:, [0, 2]], None)
    assert torch.equal(lp, lp2)
    np.testing.assert_allclose(ent.detach().numpy(), ent2.detach().numpy(), rtol=1e-6, atol=1e-7)
    (lp.sum() + ent.sum()).backward()
    assert torch.equal(logits.grad[:, 3:8], torch.zeros(4, 5)) and logits.grad[:, :3].abs().sum() > 0
    # through the policy: the same rows
    lp3, ent3, _ = pol(obs, act, action_masks=mask)
    assert torch.equal(lp3.detach(), lp.detach()) and torch.equal(ent3.detach(), ent.detach())


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
        lp, ent, v = pol(obs, act, action_masks=masks_of(z, f"{name}_b{i}_masks", torch.device("cpu")))
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


@pytest.mark.parametrize("name", STEP_CASES)
def test_cpu_update_steps_match_reference(fx, name):
    z, index = fx
    meta = index[name]
    loss, norms, params = cpu_steps(case_policy(meta), z, name, meta)
    assert_close(loss, z[f"{name}_loss"], z[f"{name}_err_loss"], (name, "loss"))
    assert_close(norms, z[f"{name}_norms"], z[f"{name}_err_norms"], (name, "norms"))
    for i in range(meta["n"]):
        assert_close(params[i], z[f"{name}_params"][i], per_tensor(z[f"{name}_err_params"][i], meta["shapes"]),
                     (name, "params", i))


def test_whole_network_kernel_specs_stay_none():
    """Both whole-network kernel families key on the head's class: a MultiDiscrete policy takes the
    per-minibatch path, and so does the fused CNN heads path (cnn_ops.heads_fusable)."""
    from rl_algo_impls_amd.cnn_ops import _heads_ok
    from rl_algo_impls_amd.mlp_wide import wide_mlp_spec

    obs = Box(-np.inf, np.inf, (5,), np.float32)
    kw = dict(pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64])
    cat = ActorCritic(SpaceEnv(1, obs, Discrete(6)), **kw)
    assert mlp_actor_critic_spec(cat) is not None  # the same shape with the Categorical head qualifies
    pol = ActorCritic(SpaceEnv(1, obs, MultiDiscrete([3, 5, 2])), **kw)
    assert wide_mlp_spec(pol) is None and mlp_actor_critic_spec(pol) is None
    flat = ActorCritic(SpaceEnv(1, obs, MultiDiscrete([3, 5, 2])), pi_hidden_sizes=[], v_hidden_sizes=[])
    assert not _heads_ok(flat.network, None)
    flat_cat = ActorCritic(SpaceEnv(1, obs, Discrete(6)), pi_hidden_sizes=[], v_hidden_sizes=[])
    assert _heads_ok(flat_cat.network, None) and not _heads_ok(flat_cat.network, torch.ones(1, 6, dtype=torch.bool))


def test_step_act_mode_respect_masks(fx):
    _, index = fx
    meta = index["md_masked"]
    env = MaskedMultiDiscreteVecEnv(64, meta["nvec"], obs_dim=meta["obs_dim"], seed=3)
    pol = case_policy(meta).to(torch.device("cpu"))
    obs, _ = env.reset()
    mask = env.get_action_mask()
    off = np.concatenate([[0], np.cumsum(meta["nvec"])])[:-1]
    torch.manual_seed(0)
    for _ in range(8):
        s = pol.step(obs, action_masks=mask)
        assert s.a.shape == (64, 3) and s.a.dtype == np.int64 and s.logp_a.shape == (64,) and s.v.shape == (64,)
        assert np.take_along_axis(mask, off + s.a, axis=1).all(), "a masked action was drawn"
        np.testing.assert_array_equal(s.clamped_a, s.a)
        with torch.no_grad():
            lp = pol(torch.from_numpy(obs), torch.from_numpy(s.a), action_masks=torch.from_numpy(mask)).logp_a
        np.testing.assert_array_equal(s.logp_a, lp.numpy())
    a = pol.act(obs, deterministic=True, action_masks=mask)
    with torch.no_grad():
        hidden, _ = pol.network.dist_params_and_value(torch.from_numpy(obs))
        logits = pol.network._pi.final(hidden).numpy()
    masked = np.where(mask, logits, np.finfo(np.float32).min)
    want = np.stack([masked[:, o:o + n].argmax(1) for o, n in zip(off, meta["nvec"])], axis=1)
    np.testing.assert_array_equal(a, want)
    assert pol.act(obs, deterministic=False, action_masks=mask).shape == (64, 3)
    assert pol.act(obs).shape == (64, 3)  # no mask: every entry valid


def test_load_and_load_from(fx, tmp_path):
    _, index = fx
    meta = index["md"]
    env = case_env(meta, n=3)
    a = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    b = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    a.save(str(tmp_path))
    b.load(str(tmp_path))
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    c = ActorCritic(env, **meta["policy"]).to(torch.device("cpu"))
    assert c.load_from(a) is c
    for k, v in a.state_dict().items():
        assert torch.equal(v, c.state_dict()[k]), k


def test_synthetic_env_masks_follow_the_observation():
    env = MaskedMultiDiscreteVecEnv(32, (3, 5, 2), seed=5)
    obs, _ = env.reset()
    m0 = env.get_action_mask()
    assert m0.shape == (32, 10) and m0.dtype == np.bool_
    np.testing.assert_array_equal(m0, env.mask_of(obs))
    for lo, hi in ((0, 3), (3, 8), (8, 10)):
        assert m0[:, lo:hi].any(axis=1).all()
    assert not m0.all() and m0.mean() > 0.4
    off = np.array([0, 3, 8])
    valid = np.stack([m0[:, lo:hi].argmax(1) for lo, hi in ((0, 3), (3, 8), (8, 10))], axis=1)
    obs2, rew, term, trunc, _ = env.step(valid)
    assert env.invalid_actions == 0 and (rew == 1.0).all()
    m1 = env.get_action_mask()
    np.testing.assert_array_equal(m1, env.mask_of(obs2))
    assert (m1 != m0).any(), "the mask moves with the observation"
    bad = np.stack([(~m1[:, lo:hi]).argmax(1) for lo, hi in ((0, 3), (3, 8), (8, 10))], axis=1)
    n_bad = int((~np.take_along_axis(m1, off + bad, axis=1)).sum())
    env.step(bad)
    assert env.invalid_actions == n_bad > 0


def test_flat_masks_carry_no_num_actions():
    """Batch.num_actions stays None for flat masks, so scale_loss_by_num_actions keeps raising on them (the
    generator itself allocates pinned host memory and HIP events: tests/test_gpu_multidiscrete.py)."""
    from rl_algo_impls_amd import rollout

    with pytest.raises(NotImplementedError, match="flat"):
        rollout._num_actions(None, torch.ones(2, 3, 10, dtype=torch.bool), None, None)
