"""DoubleCone GridNet actor-critic on the GPU (MIOpen convolutions on NHWC activations, the fused SE gate
of csrc/se_gate.hip, the fused GridNet head) against the reference's CPU run (tests/golden/
double_cone_cases.npz, double_cone_ppo_steps.npz; tests/golden/make_golden_double_cone.py).

Weights and gradients of the large tensors are compared on their recorded elements and moments
(tests/double_cone_common.py)."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from double_cone_common import FLAT_SAMPLE, SMALL_KW, check_moments, moments, sample_idx, sampled
from test_double_cone_cpu import small_net

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return np.load(GOLDEN / "double_cone_cases.npz", allow_pickle=False)


def _run(cases, i, fused):
    """Forward and the gradients of sum(wl*logp + we*entropy + wv.v) of small network i on the GPU."""
    from rl_algo_impls_amd.backbone import set_fused_gate

    net = small_net(cases, i).to(DEV)
    set_fused_gate(net, fused)
    t = lambda k: torch.tensor(cases[f"c{i}_{k}"], device=DEV)
    logp, ent, v = net(t("obs"), t("actions"), action_masks=t("masks"))
    ((t("wl") * logp).sum() + (t("we") * ent).sum() + (t("wv") * v).sum()).backward()
    out = dict(logp=logp, entropy=ent, v=v)
    grads = {k: p.grad.cpu().numpy() for k, p in net.named_parameters()}
    return {k: x.detach().cpu().numpy() for k, x in out.items()}, grads


@pytest.fixture(scope="module")
def runs(cases):
    """(i, fused) -> (outputs, gradients), computed once."""
    cache = {}

    def get(i, fused):
        if (i, fused) not in cache:
            cache[(i, fused)] = _run(cases, i, fused)
        return cache[(i, fused)]

    return get


@pytest.mark.parametrize("i", [0, 1])
def test_forward_backward_vs_reference(cases, runs, monkeypatch, i):
    """Both small networks (gelu_pool_conv True / False) with the fused gate on, against the reference's CPU
    forward and autograd, at test_squnet.py's tolerances (the same engines, a similar depth): logp / entropy
    rtol 1e-4 atol 2e-3; values rtol 1e-4 atol 1e-5; gradients atol 2e-4 + 2e-3 of each tensor's max |grad|."""
    from rl_algo_impls_amd import backbone as bb

    calls = []
    orig = bb._SETail.apply
    monkeypatch.setattr(bb._SETail, "apply", staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    out, grads = _run(cases, i, True)
    assert len(calls) == 4  # every SE block took the one-launch gate
    np.testing.assert_allclose(out["logp"], cases[f"c{i}_logp"], rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(out["entropy"], cases[f"c{i}_entropy"], rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(out["v"], cases[f"c{i}_v"], rtol=1e-4, atol=1e-5)
    for k, g in grads.items():
        ref, m = cases[f"c{i}_grad/{k}"], cases[f"c{i}_gradm/{k}"]
        tol = 2e-4 + 2e-3 * float(m[2])
        assert np.isfinite(g).all(), k
        np.testing.assert_allclose(sampled(g), ref, rtol=0, atol=tol, err_msg=k)
        check_moments(g, m, tol, k)


@pytest.mark.parametrize("i", [0, 1])
def test_fused_gate_on_against_off(cases, runs, i):
    """The same network and inputs with the fused gate on and off (the torch gate).  Bound, per compared
    array: the kernel test's rule (4 x the float32 torch path's error + one float32 ulp of the array's largest
    magnitude) with the torch-GPU path's error against the reference's golden values in the place of the
    torch-float32 error, times the network's 4 SE blocks:
        |on - off| <= 4 blocks * (4 * max|off - golden| + ulp(max|golden|)).
    Gradients are compared on the recorded elements."""
    (on, gon), (off, goff) = runs(i, True), runs(i, False)
    n_blocks = 4

    def check(name, a, b, ref):
        e_t = float(np.abs(b.astype(np.float64) - ref).max())
        bound = n_blocks * (4 * e_t + float(np.spacing(np.float32(np.abs(ref).max()))))
        d = float(np.abs(a.astype(np.float64) - b).max())
        print(f"double_cone case {i} {name}: on-off {d:.3e} off-golden {e_t:.3e} bound {bound:.3e}")
        assert d <= bound, (name, d, bound)

    for k, gk in (("logp", "logp"), ("entropy", "entropy"), ("v", "v")):
        check(k, on[k], off[k], cases[f"c{i}_{gk}"])
    for k in gon:
        check(k, sampled(gon[k]), sampled(goff[k]), cases[f"c{i}_grad/{k}"])


class _FixedRollout:
    def __init__(self, batches):
        self.batches = batches

    @property
    def total_steps(self):
        return sum(len(b) for b in self.batches)

    def num_minibatches(self, bs):
        return len(self.batches)

    def minibatches(self, bs, shuffle=True):
        return iter(self.batches)

    def explained_variance(self):
        y = torch.cat([b.returns for b in self.batches]).double()
        p = torch.cat([b.values for b in self.batches]).double()
        return float(1 - torch.var(y - p, unbiased=False) / torch.var(y, unbiased=False))


class _SpacesEnv:
    def __init__(self, side):
        from test_double_cone_cpu import _spaces

        self.single_observation_space, self.single_action_space, self.action_plane_space = _spaces(side)
        self.num_envs = 1
        self.unwrapped = self


def test_ppo_update_matches_reference():
    """Two minibatch steps with the Microrts-selfplay-dc-phases hyperparameters (K = 3 critics, gamma /
    gae_lambda / vf_coef vectors, multi_reward_weights, clip_range_vf, vf halving) against the reference's
    PPO.learn_epoch on the same minibatches, checked as test_squnet.py checks squnet_ppo_steps.npz: stats
    rtol 5e-4 atol 5e-5 (value losses atol 2e-6); grad norms rtol 5e-4; parameters atol 0.05 * lr.  The
    policy is rebuilt from the fixture's seed and checked against the recorded initial elements."""
    from rl_algo_impls_amd.policy import ActorCritic
    from rl_algo_impls_amd.ppo import PPO
    from rl_algo_impls_amd.rollout import Batch

    name = "dc_phases_vclip"
    z = np.load(GOLDEN / "double_cone_ppo_steps.npz", allow_pickle=False)
    meta = json.loads(str(z["index"]))[name]
    torch.manual_seed(meta["seed"])
    pol = ActorCritic(_SpacesEnv(8), actor_head_style="double_cone", gelu_pool_conv=False, **SMALL_KW)
    init = torch.nn.utils.parameters_to_vector(pol.parameters()).detach().numpy()
    assert len(init) == meta["num_params"]
    idx = sample_idx(len(init), small=0, sample=FLAT_SAMPLE)
    scale = float(np.abs(z[f"{name}/init"]).max())
    np.testing.assert_allclose(init[idx], z[f"{name}/init"], rtol=0, atol=1e-5 * scale)
    check_moments(init, z[f"{name}/init_moments"], 1e-5 * scale, "init")
    pol = pol.to(DEV)
    kw = dict(meta["kw"])
    algo = PPO(pol, DEV, None, **kw)
    bs = []
    for i in range(meta["n"]):
        t = lambda k: torch.from_numpy(z[f"{name}/b{i}_{k}"]).to(DEV)
        bs.append(Batch(t("obs"), t("logprobs"), t("actions"), t("action_masks"), None, t("values"),
                        t("advantages"), t("returns")))
    stats, norms, K = algo.update(_FixedRollout(bs))
    assert K == 3
    ref = z[f"{name}/stats"]
    np.testing.assert_allclose(stats[:, :5], ref[:, :5], rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(stats[:, 5:8], ref[:, 5:8], rtol=5e-4, atol=2e-6)
    np.testing.assert_allclose(norms, z[f"{name}/norms"], rtol=5e-4)
    tol = 0.05 * float(kw["learning_rate"])
    last = algo.flat.flat.cpu().numpy()
    np.testing.assert_allclose(last[idx], z[f"{name}/params"][-1], rtol=0, atol=tol)
    check_moments(last, z[f"{name}/params_moments"][-1], tol, "params")
    assert float(algo.optimizer.state_dict()["state"][0]["step"]) == meta["opt_step"]


@pytest.mark.parametrize("freeze_backbone", [False, True], ids=["train", "freeze_backbone"])
def test_rollout_and_update(freeze_backbone):
    """SyncStepRolloutGenerator on SyntheticVecEnv(kind="microrts") with a small DoubleCone policy: 4 envs,
    n_steps 4, one epoch of one minibatch, through the graph-captured rollout forward and the replayed
    update.  Parameters end finite and changed; the first pass over fresh data has ratio 1 (no clipped
    sample, approx_kl at rounding level: the update recomputes the rollout's log-probs); with
    freeze_backbone the backbone's parameters keep their bits."""
    from rl_algo_impls_amd.envs import SyntheticVecEnv
    from rl_algo_impls_amd.policy import ActorCritic
    from rl_algo_impls_amd.ppo import PPO
    from rl_algo_impls_amd.rollout import SyncStepRolloutGenerator

    torch.manual_seed(1)
    env = SyntheticVecEnv(4, kind="microrts", seed=1, obs_pool=2)
    pol = ActorCritic(env, actor_head_style="double_cone", gelu_pool_conv=False, **SMALL_KW).to(DEV)
    gen = SyncStepRolloutGenerator(pol, env, n_steps=4)
    algo = PPO(pol, DEV, None, batch_size=16, n_epochs=1, gamma=[0.99, 0.999, 0.999], gae_lambda=[0.95, 0.99, 0.99],
               clip_range=0.1, clip_range_vf=0.1, ppo2_vf_coef_halving=True, multi_reward_weights=[0.8, 0.01, 0.19],
               vf_coef=[0.5, 0.1, 0.2], ent_coef=0.01, learning_rate=1e-4, freeze_backbone=freeze_backbone)
    before = {k: p.detach().clone() for k, p in pol.named_parameters()}
    algo.learn(4 * 4, gen)
    assert gen._fwd_graph is not None
    if not freeze_backbone:  # (an update with a freeze_* flag runs on the per-minibatch path)
        assert algo.use_graphs and algo._graphed is not None
    ts = algo.last_train_stats
    assert np.isfinite([ts.loss, ts.pi_loss, ts.entropy_loss, ts.approx_kl, ts.grad_norm]).all()
    assert ts.clipped_frac == 0.0 and abs(ts.approx_kl) < 1e-5
    assert gen.actions.shape == (4, 4, 256, 7) and gen.values.shape == (4, 4, 3)
    changed = {k: not torch.equal(p.detach(), before[k]) for k, p in pol.named_parameters()}
    assert all(bool(torch.isfinite(p).all()) for p in pol.parameters())
    for k, c in changed.items():
        if k.startswith("network.backbone."):
            assert c != freeze_backbone or (not freeze_backbone and ".fc." in k), k
        else:
            assert c, k
