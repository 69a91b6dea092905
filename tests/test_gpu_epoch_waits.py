"""The arrival waits of the CartPole epoch kernel (csrc/mlp_mc8.h): round 1 polls its one counter with
one load per iteration, round 2 polls both networks' counters from two lanes of wave 0.  A wait that
lets a CU through early reads a slot another CU is still writing, which shows as run-to-run
differences; a wait that expires sets the kernel's error flag, which PPO.update raises on.  So every
case runs the same update twice from identical seeds and requires identical bits, in each geometry
the kernel is instantiated for."""
import numpy as np
import pytest
import torch

from rl_algo_impls_amd.ppo import PPO
from rl_algo_impls_amd.rollout import DeviceRollout

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
D, N_ACT = 4, 2


class _SpaceEnv:
    """Just the spaces ActorCritic reads (obs Box(d), Discrete(n))."""

    def __init__(self, d, n):
        from rl_algo_impls_amd.envs import Box, Discrete

        self.single_observation_space = Box(-1.0, 1.0, shape=(d,))
        self.single_action_space = Discrete(n)
        self.num_envs = 1


def _random_rollout(T, N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = lambda x: x.to(DEV)
    obs = t(torch.randn(T, N, D, generator=g))
    act = t(torch.randint(0, N_ACT, (T, N), generator=g))
    rew = t(torch.randn(T, N, generator=g))
    starts = t((torch.rand(T, N, generator=g) < 0.05).to(torch.uint8))
    vals = t(torch.randn(T, N, generator=g))
    logp = t(torch.log(torch.full((T, N), 1.0 / N_ACT)) + 0.1 * torch.randn(T, N, generator=g))
    nstarts = t((torch.rand(N, generator=g) < 0.05).to(torch.uint8))
    nvals = t(torch.randn(N, generator=g))
    return obs, act, rew, starts, vals, logp, nstarts, nvals


def _update(roll, T, N, bs, generic=False, n_epochs=2):
    """Two epochs of PPO.update on `roll` with injected permutations, from seed 5: the parameters, both
    Adam moments, the stats rows and the per-step gradient norms."""
    from rl_algo_impls_amd.policy import ActorCritic

    torch.manual_seed(5)
    policy = ActorCritic(_SpaceEnv(D, N_ACT), activation_fn="tanh").to(DEV)
    algo = PPO(policy, DEV, None, batch_size=bs, n_epochs=n_epochs, learning_rate=3e-3, ent_coef=0.01,
               clip_range=0.2, gamma=0.98, gae_lambda=0.9)
    algo.force_generic = generic
    assert (algo.fused_mlp_spec() is None) == generic
    obs, a_, rew, starts, vals, logp, nstarts, nvals = roll
    perms = [torch.randperm(T * N, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    r = DeviceRollout(DEV, nstarts, nvals, obs, a_, rew, starts, vals, logp, None, 0.98, 0.9,
                      perm_source=lambda k: perms.pop(0))
    stats, norms, _ = algo.update(r)
    torch.cuda.synchronize()
    return dict(params=algo.flat.flat.cpu().numpy().copy(), exp_avg=algo.optimizer.state1.cpu().numpy().copy(),
                exp_avg_sq=algo.optimizer.state2.cpu().numpy().copy(), stats=np.asarray(stats).copy(),
                norms=np.asarray(norms).copy())


def _assert_same_bits(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{k} differs between two runs from the same seeds"


@pytest.mark.parametrize("cus,bs,T,N", [
    (None, 256, 9, 100),   # the default: 16 CUs per network; 900 rows -> 3 full minibatches and 132 rows
    ("8", 256, 9, 100),    # RAI_MLP_CUS=8: two 16-row tiles per CU
    (None, 128, 5, 78),    # <= 128 rows per minibatch: the per-rank geometry M8Geo<8, 16>; 390 rows -> 3 and 6 rows
])
def test_epoch_waits_repeat_bitwise(cus, bs, T, N, monkeypatch):
    """Two epochs over a rollout with a ragged last minibatch, twice from identical seeds: identical
    parameters, Adam moments, stats rows and gradient norms (and no wait expired: update would raise)."""
    if cus:
        monkeypatch.setenv("RAI_MLP_CUS", cus)
    roll = _random_rollout(T, N, seed=D * 100 + N_ACT * 10 + bs)
    first = _update(roll, T, N, bs)
    second = _update(roll, T, N, bs)
    assert len(first["norms"]) == 2 * -(-T * N // bs)
    for k, v in first.items():
        assert np.isfinite(v).all(), k
    _assert_same_bits(first, second)


def test_epoch_waits_64_dependent_steps_per_launch():
    """64 dependent steps per launch (16,384 rows at batch 256, two epochs): both parities of every slot
    and both counters are reused 32 times per launch.  Finite, bitwise repeatable, and the first step's
    gradient norm (before any update: the same weights on both paths) within the tolerance
    test_fused_epoch_matches_generic_path uses for the norms against the per-minibatch PyTorch path."""
    T, N, bs = 64, 256, 256
    roll = _random_rollout(T, N, seed=D * 100 + N_ACT * 10 + bs + 1)
    first = _update(roll, T, N, bs)
    second = _update(roll, T, N, bs)
    assert len(first["norms"]) == 2 * 64
    for k, v in first.items():
        assert np.isfinite(v).all(), k
    _assert_same_bits(first, second)
    generic = _update(roll, T, N, bs, generic=True, n_epochs=1)
    np.testing.assert_allclose(first["norms"][0], generic["norms"][0], rtol=2e-4)
