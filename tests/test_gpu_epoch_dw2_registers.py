"""dW2 of the CartPole epoch kernel (csrc/mlp_mc8.h) in the geometries with one row tile per CU and one
column tile per wave (G = 16 at batch 256; the per-rank M8Geo<8, 16> at batch <= 128): formed in the loss
phase from the dZ2 values each wave holds and stored from the accumulators straight to the round-1 slot,
ahead of dH1, with the slot's padding columns written once per launch.  A slot written too early shows
as run-to-run differences, a wrong operand or offset as a mismatch with the per-minibatch path, unwritten
padding as a difference between a fresh and a reused workspace.  RAI_MLP_CUS=8 (two row tiles per CU)
keeps the P_B phase and is checked alongside.

320 rows (8 envs x 40 steps): at batch 256 one full step and a 64-row tail in which CUs 4-15 of G = 16
own no rows; at batch 128 two full steps and the same tail."""
import numpy as np
import pytest
import torch

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.ppo import PPO
from rl_algo_impls_amd.rollout import DeviceRollout

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N_ACT = 2
T_SMALL, N_SMALL = 40, 8

# (in_dim, activation, batch, RAI_MLP_CUS): in_dim 3 leaves a zero-padded observation column
CASES = [
    (4, "tanh", 256, None),
    (3, "relu", 256, None),
    (4, "relu", 128, None),
    (3, "tanh", 128, None),
    (4, "tanh", 256, "8"),
]


class _SpaceEnv:
    """Just the spaces ActorCritic reads (obs Box(d), Discrete(n))."""

    def __init__(self, d, n):
        from rl_algo_impls_amd.envs import Box, Discrete

        self.single_observation_space = Box(-1.0, 1.0, shape=(d,))
        self.single_action_space = Discrete(n)
        self.num_envs = 1


def _random_rollout(T, N, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = lambda x: x.to(DEV)
    obs = t(torch.randn(T, N, d, generator=g))
    act = t(torch.randint(0, N_ACT, (T, N), generator=g))
    rew = t(torch.randn(T, N, generator=g))
    starts = t((torch.rand(T, N, generator=g) < 0.05).to(torch.uint8))
    vals = t(torch.randn(T, N, generator=g))
    logp = t(torch.log(torch.full((T, N), 1.0 / N_ACT)) + 0.1 * torch.randn(T, N, generator=g))
    nstarts = t((torch.rand(N, generator=g) < 0.05).to(torch.uint8))
    nvals = t(torch.randn(N, generator=g))
    return obs, act, rew, starts, vals, logp, nstarts, nvals


def _update(roll, T, N, d, act, bs, generic=False, workspace=None):
    """Two epochs of PPO.update on `roll` with injected permutations, from seed 5: the parameters, both
    Adam moments, the stats rows and the per-step gradient norms (and the epoch kernel's workspace).
    `workspace`: "fill" = a fresh workspace of 0xFF bytes (NaN floats) instead of zeros; a tensor = that
    workspace, as an earlier update left it."""
    from rl_algo_impls_amd.policy import ActorCritic

    torch.manual_seed(5)
    policy = ActorCritic(_SpaceEnv(d, N_ACT), activation_fn=act).to(DEV)
    algo = PPO(policy, DEV, None, batch_size=bs, n_epochs=2, learning_rate=3e-3, ent_coef=0.01,
               clip_range=0.2, gamma=0.98, gae_lambda=0.9)
    algo.force_generic = generic
    assert (algo.fused_mlp_spec() is None) == generic
    if isinstance(workspace, torch.Tensor):
        algo._mlp_ws = workspace
    elif workspace == "fill":
        need = int(_lib.lib().rai_mlp_ppo_workspace_bytes(T * N, bs))
        algo._mlp_ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    obs, a_, rew, starts, vals, logp, nstarts, nvals = roll
    perms = [torch.randperm(T * N, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    r = DeviceRollout(DEV, nstarts, nvals, obs, a_, rew, starts, vals, logp, None, 0.98, 0.9,
                      perm_source=lambda k: perms.pop(0))
    stats, norms, _ = algo.update(r)
    torch.cuda.synchronize()
    out = dict(params=algo.flat.flat.cpu().numpy().copy(), exp_avg=algo.optimizer.state1.cpu().numpy().copy(),
               exp_avg_sq=algo.optimizer.state2.cpu().numpy().copy(), stats=np.asarray(stats).copy(),
               norms=np.asarray(norms).copy())
    return out, algo._mlp_ws


def _assert_same_bits(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k} differs {what}"


_ROLLS, _FUSED = {}, {}


def _small_roll(d, bs):
    if (d, bs) not in _ROLLS:
        _ROLLS[d, bs] = _random_rollout(T_SMALL, N_SMALL, d, seed=d * 100 + N_ACT * 10 + bs)
    return _ROLLS[d, bs]


def _fused(case, monkeypatch):
    """The fused update of a case on a zeroed workspace, run once and shared by the tests below."""
    d, act, bs, cus = case
    if cus:
        monkeypatch.setenv("RAI_MLP_CUS", cus)
    if case not in _FUSED:
        _FUSED[case] = _update(_small_roll(d, bs), T_SMALL, N_SMALL, d, act, bs)[0]
    return _FUSED[case]


@pytest.mark.parametrize("case", CASES)
def test_dw2_registers_repeat_bitwise(case, monkeypatch):
    """The same update twice from identical seeds: identical parameters, Adam moments, stats rows and
    gradient norms (and no wait expired: update would raise)."""
    d, act, bs, _ = case
    first = _fused(case, monkeypatch)
    second = _update(_small_roll(d, bs), T_SMALL, N_SMALL, d, act, bs)[0]
    assert len(first["norms"]) == 2 * -(-T_SMALL * N_SMALL // bs)
    for k, v in first.items():
        assert np.isfinite(v).all(), k
    _assert_same_bits(first, second, "between two runs from the same seeds")


@pytest.mark.parametrize("case", CASES)
def test_dw2_registers_match_per_minibatch_path(case, monkeypatch):
    """Against the per-minibatch path PPO takes with the fused epoch kernels off, same rollout and
    permutations: the tolerances of test_gpu_trainer.py::test_fused_epoch_matches_generic_path (norms,
    stats rows, parameters, and its first-moment tolerance for both Adam moments)."""
    d, act, bs, _ = case
    f = _fused(case, monkeypatch)
    g = _update(_small_roll(d, bs), T_SMALL, N_SMALL, d, act, bs, generic=True)[0]
    np.testing.assert_allclose(f["norms"], g["norms"], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(f["stats"][:, :6], g["stats"][:, :6], rtol=2e-3, atol=2e-6)
    np.testing.assert_allclose(f["params"], g["params"], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(f["exp_avg"], g["exp_avg"], rtol=2e-2, atol=1e-6)
    np.testing.assert_allclose(f["exp_avg_sq"], g["exp_avg_sq"], rtol=2e-2, atol=1e-6)


@pytest.mark.parametrize("case", CASES)
def test_dw2_registers_fresh_workspace_same_bits(case, monkeypatch):
    """The first launch on a workspace the kernel never wrote, filled with 0xFF bytes (every float a NaN), and
    a later update on that same, now used, workspace: both the bits of the update on a zeroed workspace.
    Whatever the share sums read -- the W2 rows' padding columns included -- the launch wrote first."""
    d, act, bs, _ = case
    zeroed = _fused(case, monkeypatch)
    fresh, ws = _update(_small_roll(d, bs), T_SMALL, N_SMALL, d, act, bs, workspace="fill")
    for k, v in fresh.items():
        assert np.isfinite(v).all(), k
    _assert_same_bits(zeroed, fresh, "between a zeroed and a 0xFF-filled fresh workspace")
    reused, _ = _update(_small_roll(d, bs), T_SMALL, N_SMALL, d, act, bs, workspace=ws)
    _assert_same_bits(fresh, reused, "between the first launch on a workspace and a later one")


@pytest.mark.parametrize("cus,bs", [
    (None, 256),   # G = 16
    ("8", 256),    # RAI_MLP_CUS=8: two row tiles per CU, the P_B phase
    (None, 128),   # the per-rank geometry M8Geo<8, 16>
])
def test_dw2_registers_64_dependent_steps_per_launch(cus, bs, monkeypatch):
    """64 dependent steps per launch (64 x batch rows, two epochs): each parity's round-1 slot is
    rewritten 31 times per launch, every time from the loss phase of the step two after the one that
    read it.  Finite and bitwise repeatable in each geometry."""
    if cus:
        monkeypatch.setenv("RAI_MLP_CUS", cus)
    T, N, d = 64, bs, 4
    roll = _random_rollout(T, N, d, seed=d * 100 + N_ACT * 10 + bs + 2)
    first = _update(roll, T, N, d, "tanh", bs)[0]
    second = _update(roll, T, N, d, "tanh", bs)[0]
    assert len(first["norms"]) == 2 * 64
    for k, v in first.items():
        assert np.isfinite(v).all(), k
    _assert_same_bits(first, second, "between two runs from the same seeds")
