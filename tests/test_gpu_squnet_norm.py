"""The squeeze-U-Net with `normalization="layer"` on the device: every (conv, ChannelLayerNorm2d[, GELU])
through the fused HIP pass (rai_chan_ln_fwd / _bwd) on NHWC activations, against the reference network's
recorded CPU run (tests/golden/squnet_norm_cases.npz, squnet_norm_case_b.npz, squnet_norm_ppo_steps.npz;
tests/golden/make_golden_squnet_norm.py).

Tolerances are those of tests/test_squnet.py's GPU tests (fp32 convolutions on different engines, 20+
layers deep): logp / entropy rtol 1e-4 atol 2e-3; values rtol 1e-4 atol 1e-5; gradients atol 2e-4 + 2e-3 of
each tensor's max |grad|; PPO stats rtol 5e-4 atol 5e-5 (v_loss atol 2e-6), grad norms rtol 5e-4,
parameters atol 0.05 * lr."""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from squnet_norm_common import C5_KW, CASE_FILES, SpacesEnv, build_net, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cases():
    return {i: np.load(GOLDEN / f, allow_pickle=False) for i, f in CASE_FILES.items()}


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the entries into the fused autograd Function (a silent fall-back to torch would pass the
    numeric checks)."""
    from rl_algo_impls_amd import backbone

    calls = []
    real = backbone.chan_ln_fused

    def counted(y, bias, norm, gelu):
        calls.append((int(y.shape[1]), bool(gelu), int(y.shape[2] * y.shape[3])))
        return real(y, bias, norm, gelu)

    monkeypatch.setattr(backbone, "chan_ln_fused", counted)
    return calls


def _n_chan_norms(net):
    from rl_algo_impls_amd.backbone import ChannelLayerNorm2d

    return sum(isinstance(m, ChannelLayerNorm2d) for m in net.modules())


def _forward_backward(net, z, i):
    t = lambda k: torch.tensor(z[f"c{i}_{k}"], device=DEV)
    net.zero_grad(set_to_none=True)
    logp, ent, v = net(t("obs"), t("actions"), action_masks=t("masks"))
    ((t("wl") * logp).sum() + (t("we") * ent).sum() + (t("wv") * v).sum()).backward()
    h = lambda a: a.detach().cpu().numpy()
    return h(logp), h(ent), h(v), {k: h(p.grad) for k, p in net.named_parameters()}


def _assert_close(got, ref, what):
    (logp, ent, v, grads), (rlogp, rent, rv, rgrads) = got, ref
    np.testing.assert_allclose(logp, rlogp, rtol=1e-4, atol=2e-3, err_msg=what)
    np.testing.assert_allclose(ent, rent, rtol=1e-4, atol=2e-3, err_msg=what)
    np.testing.assert_allclose(v, rv, rtol=1e-4, atol=1e-5, err_msg=what)
    assert list(grads) == list(rgrads)
    for k, r in rgrads.items():
        np.testing.assert_allclose(grads[k], r, rtol=0, atol=2e-4 + 2e-3 * float(np.abs(r).max()),
                                   err_msg=f"{what} {k}")


@pytest.mark.parametrize("i", [0, 1])
def test_forward_backward_vs_reference(cases, fused_calls, monkeypatch, i):
    from rl_algo_impls_amd import backbone

    z = cases[i]
    net = load_case(build_net(i), z, i).to(DEV)
    n_norm = _n_chan_norms(net)
    assert n_norm + net._critic_features == int(z[f"c{i}_meta"][3])  # + one nn.LayerNorm per critic head
    fused = _forward_backward(net, z, i)
    assert len(fused_calls) == n_norm, "every (conv, norm[, GELU]) takes the fused pass on the NHWC path"
    assert any(g for _, g, _ in fused_calls) and any(not g for _, g, _ in fused_calls)  # SE blocks: a norm without GELU
    golden = (z[f"c{i}_logp"], z[f"c{i}_entropy"], z[f"c{i}_v"],
              {k: z[f"c{i}_grad/{k}"] for k, _ in net.named_parameters()})
    _assert_close(fused, golden, "fused vs reference")
    # the same network on an NCHW-contiguous input: the modules' torch path.  (A 1x1 activation is NCHW-
    # and NHWC-contiguous at once, the same bytes either way: case (b)'s deepest level still takes the
    # fused pass.)  Both are fp32 evaluations of one function, each held to the bounds above against the
    # reference; they are held to the same bounds against each other
    del fused_calls[:]
    monkeypatch.setattr(backbone, "_CHANNELS_LAST", False)
    plain = _forward_backward(net, z, i)
    assert all(hw == 1 for _, _, hw in fused_calls) and len(fused_calls) < n_norm // 2
    _assert_close(plain, golden, "torch path vs reference")
    _assert_close(fused, plain, "fused vs torch path")


@pytest.mark.parametrize("graphs", [True, False], ids=["graphed", "eager"])
def test_ppo_steps_match_reference(fused_calls, graphs):
    """The two recorded PPO minibatch steps of case (a) through PPO.update, replayed from a hipGraph and
    eagerly; every gamma / beta moves."""
    from make_golden_networks import load_flat
    from rl_algo_impls_amd.policy import ActorCritic
    from rl_algo_impls_amd.ppo import PPO
    from rl_algo_impls_amd.rollout import DeviceRollout

    z = np.load(GOLDEN / "squnet_norm_ppo_steps.npz", allow_pickle=False)
    meta = json.loads(str(z["index"]))
    pol = ActorCritic(SpacesEnv(meta["side"]), actor_head_style="squeeze_unet", normalization="layer",
                      **meta["policy_kw"])
    assert [k for k, _ in pol.named_parameters()] == [str(k) for k in z["keys"]]
    load_flat(pol, z["init"])
    pol = pol.to(DEV)
    kw = dict(meta["kw"])
    algo = PPO(pol, DEV, None, n_epochs=1, **kw)
    algo.use_graphs = graphs
    t = lambda f: torch.stack([torch.from_numpy(z[f"b{i}_{f}"]) for i in range(meta["n"])]).to(DEV)
    r = DeviceRollout.from_fields(DEV, t("obs"), t("actions"), t("values"), t("advantages"), t("returns"),
                                  t("logprobs"), action_masks=t("action_masks"),
                                  perm_source=lambda k: torch.arange(k, device=DEV))
    before = {k: p.detach().clone() for k, p in pol.named_parameters()}
    stats, norms, K = algo.update(r)
    assert K == 1 and (algo._graphed is not None) == graphs, "update path"
    assert len(fused_calls) > 0
    ref = z["stats"]
    np.testing.assert_allclose(stats[:, :5], ref[:, :5], rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(stats[:, 5], ref[:, 5], rtol=5e-4, atol=2e-6)
    np.testing.assert_allclose(norms, z["norms"], rtol=5e-4)
    np.testing.assert_allclose(algo.flat.flat.cpu().numpy(), z["params_last"], rtol=0,
                               atol=0.05 * float(kw["learning_rate"]))
    assert float(algo.optimizer.state_dict()["state"][0]["step"]) == meta["opt_step"]
    moved = [k for k, p in pol.named_parameters() if k.endswith((".gamma", ".beta"))]
    assert len(moved) == 20
    for k, p in pol.named_parameters():
        if k in moved:
            assert not torch.equal(p.detach(), before[k]), k


def test_rollout_captured_forward_and_training(fused_calls):
    """ActorCritic(env, actor_head_style="squeeze_unet", normalization="layer"): the rollout's graph-captured
    forward gives the eager forward's logits and values (the same kernels, replayed), and a rollout + update
    with graphs on trains."""
    from rl_algo_impls_amd.envs import SyntheticVecEnv
    from rl_algo_impls_amd.policy import ActorCritic
    from rl_algo_impls_amd.ppo import PPO
    from rl_algo_impls_amd.rollout import SyncStepRolloutGenerator

    torch.manual_seed(1)
    env = SyntheticVecEnv(4, kind="microrts", seed=1, obs_pool=2)
    pol = ActorCritic(env, actor_head_style="squeeze_unet", normalization="layer", channels_per_level=[16, 16, 16],
                      **{k: v for k, v in C5_KW.items() if k != "init_layers_orthogonal"}).to(DEV)
    gen = SyncStepRolloutGenerator(pol, env, n_steps=4)
    algo = PPO(pol, DEV, None, batch_size=8, n_epochs=1, gamma=[0.99, 0.999, 0.999], gae_lambda=[0.95, 0.99, 0.99],
               clip_range=0.1, clip_range_vf=None, ppo2_vf_coef_halving=True, multi_reward_weights=[0.8, 0.01, 0.19],
               vf_coef=[0.5, 0.1, 0.2], ent_coef=0.01, learning_rate=1e-4)
    assert algo.use_graphs and gen.rollout_graph
    p0 = algo.flat.flat.detach().clone()
    algo.learn(4 * 4, gen)
    assert gen._fwd_graph is not None and algo._graphed is not None
    ts = algo.last_train_stats
    assert np.isfinite([ts.loss, ts.pi_loss, ts.entropy_loss, ts.approx_kl, ts.grad_norm]).all()
    assert not torch.equal(p0, algo.flat.flat) and bool(torch.isfinite(algo.flat.flat).all())
    with torch.no_grad():
        logits_g, v_g = gen._policy_forward(pol.network.logits_and_value)  # one captured step, replayed
        logits_g, v_g = logits_g.clone(), v_g.clone()
        n = len(fused_calls)
        logits_e, v_e = pol.network.logits_and_value(gen.next_obs_dev)
    assert len(fused_calls) - n == _n_chan_norms(pol.network)
    # the same kernels on the same inputs; MIOpen may pick another solver outside the capture: fp32 bounds
    np.testing.assert_allclose(logits_g.cpu().numpy(), logits_e.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(v_g.cpu().numpy(), v_e.cpu().numpy(), rtol=1e-4, atol=1e-5)
