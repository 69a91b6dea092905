"""The two-slot preparation of the whole-epoch updates (ppo_epoch.py): epoch k + 1's permuted copy is
gathered on a side stream into the slot epoch k - 1 read, while epoch k's kernel reads the other.  A slot
rewritten while a kernel still reads it shows as a difference from the same update with every epoch
prepared in order on the current stream, where nothing overlaps."""
import numpy as np
import pytest
import torch

from rl_algo_impls_amd.ppo import PPO
from rl_algo_impls_amd.rollout import DeviceRollout

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N_EPOCHS = 4  # each slot is refilled once while the other is being read


class _InOrder:
    """A rollout without DeviceRollout's two epoch slots: PPO prepares such a rollout's epochs in order
    on the current stream (epoch_batch without a slot: one permuted copy, rewritten in stream order)."""

    def __init__(self, r):
        self._r = r

    def __getattr__(self, name):
        if name == "alloc_epoch_buffers":
            raise AttributeError(name)
        return getattr(self._r, name)


def _update(kind, T, N, bs, in_order):
    from rl_algo_impls_amd.envs import SyntheticVecEnv
    from rl_algo_impls_amd.policy import ActorCritic

    torch.manual_seed(7)
    env = SyntheticVecEnv(4, kind, seed=3)
    if kind == "cartpole":  # d = 4, n = 2, 64 wide: rai_mlp_ppo_epoch
        policy = ActorCritic(env, activation_fn="tanh").to(DEV)
    else:  # rai_mlp_wide_epoch
        policy = ActorCritic(env, pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64], activation_fn="relu",
                             log_std_init=-1.0, init_layers_orthogonal=False).to(DEV)
    algo = PPO(policy, DEV, None, batch_size=bs, n_epochs=N_EPOCHS, learning_rate=3e-3, ent_coef=0.01)
    assert (algo.fused_mlp_spec() is not None) == (kind == "cartpole")
    g = torch.Generator(device="cpu").manual_seed(11)
    obs = torch.randn((T, N) + env.single_observation_space.shape, generator=g)
    act = (torch.randint(0, 2, (T, N), generator=g) if kind == "cartpole"
           else torch.randn(T, N, 6, generator=g).clamp(-1, 1))
    t = lambda x: x.to(DEV)
    perms = [torch.randperm(T * N, generator=torch.Generator().manual_seed(s)) for s in range(1, N_EPOCHS + 1)]
    r = DeviceRollout(DEV, t(torch.zeros(N, dtype=torch.uint8)), t(torch.randn(N, generator=g)), t(obs), t(act),
                      t(torch.randn(T, N, generator=g)), t((torch.rand(T, N, generator=g) < 0.05).to(torch.uint8)),
                      t(torch.randn(T, N, generator=g)), t(-1.0 + 0.1 * torch.randn(T, N, generator=g)), None,
                      0.99, 0.95, perm_source=lambda n: perms.pop(0))
    algo.kernel_events = []
    stats, norms, _ = algo.update(_InOrder(r) if in_order else r)
    torch.cuda.synchronize()
    assert not perms and len(algo.kernel_events) == N_EPOCHS, "one whole-epoch launch per epoch"
    assert (algo._we_ws is not None) == (kind != "cartpole")
    assert (1 in r._perm_bufs) == (not in_order), "only the overlapped preparation fills a second slot"
    return dict(params=algo.flat.flat.cpu().numpy(), exp_avg=algo.optimizer.state1.cpu().numpy(),
                exp_avg_sq=algo.optimizer.state2.cpu().numpy(), stats=np.asarray(stats), norms=np.asarray(norms))


@pytest.mark.parametrize("kind,T,N,bs", [
    ("cartpole", 5, 50, 40),      # 250 rows: six full minibatches and a tail of 10
    ("halfcheetah", 16, 25, 64),  # 400 rows: six full minibatches and a tail of 16
])
def test_overlapped_epoch_preparation_matches_in_order(kind, T, N, bs):
    overlapped = _update(kind, T, N, bs, in_order=False)
    in_order = _update(kind, T, N, bs, in_order=True)
    assert len(overlapped["norms"]) == N_EPOCHS * 7
    for k, v in overlapped.items():
        assert np.isfinite(v).all(), k
        np.testing.assert_array_equal(v, in_order[k], err_msg=k)
