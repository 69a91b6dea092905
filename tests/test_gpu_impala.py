"""cnn_style: impala on the GPU: the encoder's fused path (impala_ops.py, csrc/conv3x3.hip) against the
same module in float64 on the CPU, the reference's own PPO minibatch steps (tests/golden/impala_steps.npz,
made by tests/golden/make_golden_impala.py) through the product path, the uint8 gather path, and one full
trainer update over the device rollout."""
import copy
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rl_algo_impls_amd import _lib, impala_ops
from rl_algo_impls_amd.envs import Box, Discrete, SyntheticVecEnv
from rl_algo_impls_amd.policy import ActorCritic, ImpalaCnnEncoder
from rl_algo_impls_amd.ppo import PPO
from rl_algo_impls_amd.rollout import DeviceRollout, SyncStepRolloutGenerator
import make_golden_networks as nets

sys.path.insert(0, str(GOLDEN))
from make_golden_pong import pong_init  # noqa: E402  (numpy-only recipe, no reference import)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, global_step=None):
        self.scalars[tag] = float(value)


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN / "impala_steps.npz", allow_pickle=False)
    return z, json.loads(str(z["index"]))


def _policy(meta):
    env = nets._Env(Box(0, 255, tuple(meta["obs_shape"]), np.uint8), Discrete(meta["n_actions"]), 1)
    torch.manual_seed(7)
    pol = ActorCritic(env, **meta["policy"])
    assert [list(p.shape) for p in pol.parameters()] == meta["shapes"]
    nets.load_flat(pol, pong_init([tuple(s) for s in meta["shapes"]], meta["init_seed"]))
    return pol


def test_encoder_matches_float64_module(fx):
    """Forward and the gradients of a fixed random cotangent, fused GPU path against the same module in
    float64 on the CPU.  Per tensor the GPU's maximum error may be 4x the maximum error the float32
    module on the CPU shows against the same float64 values in this test: the reference implementation's
    own rounding is the yardstick, and another summation order is another draw from that distribution."""
    z, meta = fx
    enc32 = _policy(meta).network._feature_extractor.feature_extractor
    assert isinstance(enc32, ImpalaCnnEncoder)
    enc64 = copy.deepcopy(enc32).double()
    encg = copy.deepcopy(enc32).to(DEV)
    obs = torch.from_numpy(z["b0_obs"][:7])
    cot = torch.from_numpy(np.random.default_rng(3).standard_normal((7, enc32.out_dim)).astype(np.float32))

    def run(enc, fwd, ct):
        out = fwd(enc)
        grads = torch.autograd.grad(out, list(enc.parameters()), ct)
        return [out.detach().double().cpu()] + [g.double().cpu() for g in grads]

    want = run(enc64, lambda e: e.fc(e.cnn(obs.double() / e.range_size)), cot.double())
    cpu32 = run(enc32, lambda e: e(obs), cot)
    obs_d = obs.to(DEV)
    assert impala_ops.fusable(encg, obs_d)
    gpu = run(encg, lambda e: e(obs_d), cot.to(DEV))
    names = ["out"] + [n for n, _ in enc32.named_parameters()]
    assert len(names) == len(want) == 33
    worst = []
    for n, w, c, g in zip(names, want, cpu32, gpu):
        assert torch.isfinite(g).all(), n
        e_cpu, e_gpu = float((c - w).abs().max()), float((g - w).abs().max())
        worst.append((e_gpu / max(e_cpu, 1e-300), n, e_gpu, e_cpu))
    print("gpu / cpu32 error ratios:", sorted(worst, reverse=True)[:5])
    for ratio, n, e_gpu, e_cpu in worst:
        assert e_gpu <= 4 * e_cpu, (n, e_gpu, e_cpu)


def _fixture_rollout(z, meta):
    """As test_gpu_pong._fixture_rollout: the fixture's minibatches, in order, as one HBM rollout."""
    n = meta["n"]
    cat = lambda f: np.concatenate([z[f"b{i}_{f}"] for i in range(n)])[None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs, act, lp, val = t(cat("obs")), t(cat("actions")), t(cat("logprobs")), t(cat("values"))
    N = obs.shape[1]
    r = DeviceRollout(DEV, t(np.zeros(N, np.bool_)), t(np.zeros(N, np.float32)), obs, act,
                      t(np.zeros((1, N), np.float32)), t(np.zeros((1, N), np.bool_)), val, lp, None, 0.99, 0.95,
                      perm_source=lambda k: torch.arange(k))
    r.advantages.copy_(t(cat("advantages")))
    r.returns.copy_(t(cat("returns")))
    return r


@pytest.mark.parametrize("graphs", [True, False], ids=["graph_replay", "eager"])
def test_impala_minibatch_steps_match_reference(fx, graphs):
    """The three fixture steps through PPO on the GPU.  Tolerances: those of test_gpu_pong.py:110-125, and,
    where 4x the fixture's own |f32 - f64| for the quantity (the reference rerun in float64 from the same
    bits) is larger, that.  With the fixture as generated this replaces:
      norms   step 2: 4 * 0.8357 = 3.34 (2e-4 * 3591.4 = 0.72); step 3: 4 * 0.0713 = 0.285 (~ 2e-4 * 1442.4 = 0.288
              stays)
      stats   loss / v_loss of steps 2, 3: 4 * 5.4e-4, 4 * 7.7e-4 / 4 * 1.07e-3, 4 * 1.52e-3 stay below
              2e-4 * value; approx_kl of step 3: 4 * 2.15e-5 = 8.6e-5 (2e-4 * 0.4035 = 8.1e-5)
      params  per tensor atol 4 * max|f32 - f64| of that tensor, 3.5e-7 .. 1.8e-3 (0.02 * lr = 1e-5): Adam's
              early, sign-like steps move a weight whose gradient is within rounding of zero by ~lr = 5e-4
              either way, in the reference's own two precisions already
      displacement  per-tensor norm of (final - init): rtol 1e-4, or 4 * the fixture's err_param_delta_norms
      moved   disagreement 4 * the fixture's err_moved_fraction where that exceeds 0.001
      opt_state1 norms  rtol 4 * 1.03e-3 = 4.1e-3 at the worst tensor (2e-3)"""
    z, meta = fx
    pol = _policy(meta).to(DEV)
    kw = dict(meta["kw"])
    algo = PPO(pol, DEV, Recorder(), n_epochs=1, **kw)
    algo.use_graphs = graphs
    assert algo.fused_mlp_spec() is None
    assert len(pol.channels_last_params()) == 15
    r = _fixture_rollout(z, meta)
    stats, norms, K = algo.update(r)
    torch.cuda.synchronize()
    if graphs:
        assert algo._graphed is not None and any(g.graph is not None for g in algo._graphed.graphs.values())
        kinds = {x.kind for g in algo._graphed.graphs.values() if g.xforms for x in g.xforms if x is not None}
        assert kinds == {_lib.RAI_XFORM_U8_CHW_TO_F32_HWC}  # 3 channels: the float32 gather transform
    lr = float(kw["learning_rate"])
    ref_n, ref = z["norms"], z["stats"]
    print("norms", norms, "ref", ref_n, "4*err", 4 * z["err_norms"])
    print("stats", stats[:, :6], "ref", ref[:, :6])
    tol_n = np.maximum(2e-4 * np.abs(ref_n), 4 * z["err_norms"])
    assert (np.abs(norms - ref_n) <= tol_n).all(), (norms, ref_n, tol_n)
    tol_s = np.maximum(2e-4 * np.abs(ref[:, :6]) + np.array([2e-6] * 5 + [0.0]), 4 * z["err_stats"][:, :6])
    assert (np.abs(stats[:, :6] - ref[:, :6]) <= tol_s).all(), (stats[:, :6], ref[:, :6], tol_s)
    got = algo.flat.vector().cpu().numpy()
    cut = np.cumsum([0] + [int(np.prod(s)) for s in meta["shapes"]])
    for j, s in enumerate(meta["shapes"]):
        a, b = got[cut[j]:cut[j + 1]], z["params"][cut[j]:cut[j + 1]]
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=max(0.02 * lr, 4 * float(z["err_params"][j])),
                                   err_msg=f"tensor {j} {s}")
    init = pong_init([tuple(s) for s in meta["shapes"]], meta["init_seed"])
    # Where 4 * err_params exceeds the 3 * lr a weight can travel in three Adam steps (the worst tensor: 1.8e-3
    # against 1.5e-3) the element check above cannot tell an updated tensor from its initial values.  So per
    # tensor the norm of the whole displacement (final - init) is held to the fixture's too: rtol 1e-4 as for
    # the parameters, or 4x the fixture's own |f32 - f64| of that norm where larger (at most 0.4 % of the norm).
    dn = np.array([np.linalg.norm((got[cut[j]:cut[j + 1]] - init[cut[j]:cut[j + 1]]).astype(np.float64))
                   for j in range(len(meta["shapes"]))])
    tol_d = np.maximum(1e-4 * z["param_delta_norms"], 4 * z["err_param_delta_norms"])
    print("displacement norms: worst |got - ref| / tol", float((np.abs(dn - z["param_delta_norms"]) / tol_d).max()),
          "worst tol / norm", float((tol_d / z["param_delta_norms"]).max()))
    assert (np.abs(dn - z["param_delta_norms"]) <= tol_d).all(), (dn, z["param_delta_norms"], tol_d)
    moved = np.abs(got - init) > 0.5 * lr
    ref_moved = np.abs(z["params"] - init) > 0.5 * lr
    print("moved disagreement", (moved != ref_moved).mean(), "fixture f32/f64", float(z["err_moved_fraction"]))
    assert (moved != ref_moved).mean() < max(0.001, 4 * float(z["err_moved_fraction"]))
    sd = algo.optimizer.state_dict()
    assert float(sd["state"][0]["step"]) == meta["opt_step"]
    m = np.array([np.linalg.norm(s["exp_avg"].double().cpu().numpy()) for s in sd["state"].values()])
    tol_m = np.maximum(2e-3 * z["opt_state1_norms"], 4 * z["err_opt_state1_norms"])
    assert (np.abs(m - z["opt_state1_norms"]) <= tol_m).all(), (m, z["opt_state1_norms"], tol_m)


def test_uint8_rows_through_the_gather_transform_equal_the_unprepared_forward(fx):
    """uint8 rollout rows through obs_transform + forward(prepared=True) == the unprepared forward, bit for
    bit, for 3 channels (float32 transform; the unprepared forward's first convolution divides the uint8
    frames in-kernel) and 4 channels (uint8 transform)."""
    from rl_algo_impls_amd import graphs

    rng = np.random.default_rng(11)
    for C in (3, 4):
        torch.manual_seed(5)
        enc = ImpalaCnnEncoder(Box(0, 255, (C, 20, 12), np.uint8), torch.nn.ReLU, None, True, 64).to(DEV)
        obs = torch.from_numpy(rng.integers(0, 256, size=(9, C, 20, 12), dtype=np.uint8)).to(DEV)
        xf = enc.obs_transform(obs)
        assert xf is not None
        assert xf.kind == (_lib.RAI_XFORM_U8_CHW_TO_U8_HWC if C == 4 else _lib.RAI_XFORM_U8_CHW_TO_F32_HWC)
        fields = [obs]
        gu = graphs.GraphedUpdate(DEV)
        gu.set_rollout(fields, 9, True)
        perm = torch.randperm(9, generator=torch.Generator(device="cpu").manual_seed(C))
        gu.start_epoch(perm.to(DEV))
        bufs = graphs.static_buffers(fields, 9, DEV, [xf])
        graphs.gather_next(DEV, gu.desc, bufs, [int(obs[0].numel())], [xf])
        assert bufs[0].dtype == (torch.uint8 if C == 4 else torch.float32)
        with torch.no_grad():
            a = enc(bufs[0], prepared=True)
            b = enc(obs[perm.to(DEV)])
        assert torch.isfinite(a).all() and torch.equal(a, b)


class _FrameEnv(SyntheticVecEnv):
    """The seeded synthetic env with procgen-like spaces: uint8 3x20x12 frames, 15 actions."""

    def __init__(self, num_envs, seed):
        super().__init__(num_envs, "pong", seed=seed, obs_pool=2)
        self.single_observation_space = Box(0, 255, (3, 20, 12), np.uint8)
        self.single_action_space = Discrete(15)
        self._pool = [self._draw_obs() for _ in range(4)]


def test_trainer_update_over_device_rollout():
    """One full update, 8 envs x 16 steps, batch 32, 2 epochs, through the device rollout: the gather
    transform, graph replay, flat gradients, clip + Adam."""
    torch.manual_seed(1)
    env = _FrameEnv(8, seed=1)
    policy = ActorCritic(env, activation_fn="relu", cnn_style="impala", cnn_flatten_dim=256).to(DEV)
    p0 = torch.nn.utils.parameters_to_vector(policy.parameters()).detach().clone()
    gen = SyncStepRolloutGenerator(policy, env, n_steps=16, seed=3)
    rec = Recorder()
    algo = PPO(policy, DEV, rec, batch_size=32, n_epochs=2, learning_rate=5e-4, ent_coef=0.01, clip_range=0.2,
               clip_range_vf=0.2)
    algo.learn(8 * 16, gen)
    ts = algo.last_train_stats
    assert np.isfinite([ts.loss, ts.pi_loss, ts.v_loss, ts.entropy_loss, ts.approx_kl, ts.grad_norm]).all()
    assert algo.optimizer.step_count == 2 * (8 * 16 // 32)
    p1 = algo.flat.vector().detach()
    assert torch.isfinite(p1).all() and float((p1 - p0).abs().max()) > 0
    if algo.use_graphs:
        assert algo._graphed is not None and any(g.graph is not None for g in algo._graphed.graphs.values())
