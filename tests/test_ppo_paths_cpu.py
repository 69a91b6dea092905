"""PPO's path selection and read-back without a device: which options leave an update to a whole-epoch
kernel (ppo_epoch.py), and the one D2H copy of the stats / norms / train-state tables (PPO._read_tables)."""
import numpy as np
import pytest
import torch

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.ppo import PPO

CPU = torch.device("cpu")


class _SpaceEnv:
    """Just the spaces ActorCritic reads: the CartPole-class MLP policy (obs Box(4), Discrete(2))."""

    def __init__(self):
        from rl_algo_impls_amd.envs import Box, Discrete

        self.single_observation_space = Box(-1.0, 1.0, shape=(4,))
        self.single_action_space = Discrete(2)
        self.num_envs = 1


def _ppo(**kw):
    from rl_algo_impls_amd.policy import ActorCritic

    torch.manual_seed(0)
    return PPO(ActorCritic(_SpaceEnv(), activation_fn="tanh"), CPU, None, **kw)


# One option switched on at a time -> (fused_mlp_spec() is not None, _wide_epoch_options_ok()), read off the
# two methods as they stood before they shared _plain_options / _fused_kernels_off: each wrote out the same
# six-term test; fused_mlp_spec alone also gave up under force_generic or a teacher term.
OPTION_TABLE = [
    ("none", {}, {}, (True, True)),
    ("gradient_accumulation", dict(gradient_accumulation=True), {}, (False, False)),
    ("kl_cutoff", dict(kl_cutoff=0.01), {}, (False, False)),
    ("multi_reward_weights", dict(multi_reward_weights=[0.8, 0.2]), {}, (False, False)),
    ("vf_weights", dict(vf_weights=[0.5, 0.5]), {}, (False, False)),
    ("normalize_advantages_after_scaling", dict(normalize_advantages_after_scaling=True), {}, (False, False)),
    ("vector_vf_coef", dict(vf_coef=[0.5, 0.25]), {}, (False, False)),
    ("force_generic", {}, dict(force_generic=True), (False, True)),
    ("teacher", dict(teacher_kl_loss_coef=5e-3, teacher_kl_loss_fn=object()), {}, (False, True)),
    ("teacher_coef_0", dict(teacher_kl_loss_coef=0, teacher_kl_loss_fn=object()), {}, (True, True)),
    ("batch_size_1", dict(batch_size=1), {}, (False, False)),
    ("batch_size_65", dict(batch_size=65), {}, (True, False)),
]


@pytest.mark.parametrize("name,kw,attrs,expected", OPTION_TABLE, ids=[c[0] for c in OPTION_TABLE])
def test_option_predicates_keep_each_decision(name, kw, attrs, expected, monkeypatch):
    monkeypatch.delenv("RAI_WIDE_EPOCH", raising=False)
    algo = _ppo(**kw)
    for k, v in attrs.items():
        setattr(algo, k, v)
    assert (algo.fused_mlp_spec() is not None, algo._wide_epoch_options_ok()) == expected
    six = name in ("gradient_accumulation", "kl_cutoff", "multi_reward_weights", "vf_weights",
                   "normalize_advantages_after_scaling", "vector_vf_coef")
    assert algo._plain_options() == (not six)
    assert algo._fused_kernels_off() == (name in ("force_generic", "teacher"))
    assert algo._wide_step() is None  # no device: never the fused wide-MLP step


def test_wide_epoch_needs_adam_and_its_switch(monkeypatch):
    monkeypatch.delenv("RAI_WIDE_EPOCH", raising=False)
    algo = _ppo()
    assert algo._wide_epoch_options_ok()
    algo.optimizer.kind = algo.optimizer.RMSPROP
    assert not algo._wide_epoch_options_ok() and algo._plain_options()
    algo.optimizer.kind = algo.optimizer.ADAM
    monkeypatch.setenv("RAI_WIDE_EPOCH", "0")
    assert not algo._wide_epoch_options_ok() and algo.fused_mlp_spec() is not None


def test_a_masked_rollout_takes_no_fused_kernel():
    class R:
        action_masks = None

    algo = _ppo()
    assert not algo._fused_kernels_off(R())
    R.action_masks = torch.ones(4, 2, dtype=torch.bool)
    assert algo._fused_kernels_off(R()) and not algo._fused_kernels_off()
    assert algo.fused_mlp_spec() is not None  # the policy still fits: update() keeps the masked rollout off it


def _tables(algo, n_rows):
    """Hand-made tables larger than the update's n_steps, and a clean train-state block."""
    S = _lib.RAI_STAT_STRIDE
    b = algo.blocks
    b.stats = (torch.arange(n_rows * S, dtype=torch.float32).reshape(n_rows, S) + 1) / 8
    b.norms = torch.arange(n_rows + 2, dtype=torch.float32) + 100
    b.teacher_stats = torch.arange(n_rows, dtype=torch.float32) + 200
    b.state = torch.zeros_like(b.state)
    return b.stats.numpy().copy(), b.norms.numpy().copy(), b.teacher_stats.numpy().copy()


def test_read_back_after_a_whole_epoch_kernel():
    algo = _ppo(vf_coef=0.25)
    table, norms_t, _ = _tables(algo, 7)
    stats, norms, K = algo._read_tables(3, 3, what="rai_some_epoch: a device-side wait")
    expect = table[:3].copy()
    expect[:, 0] += np.float32(0.25) * expect[:, 5]  # the value term of the loss column
    np.testing.assert_array_equal(stats, expect)
    np.testing.assert_array_equal(norms, norms_t[:3])
    assert K == 1 and stats.shape == (3, _lib.RAI_STAT_STRIDE) and norms.shape == (3,)
    np.testing.assert_array_equal(algo.blocks.stats.numpy(), table)  # the device table is left as it was
    algo.blocks.state.view(torch.int32)[5] = 1  # the err flag a kernel sets when a device-side wait expires
    with pytest.raises(RuntimeError, match=r"rai_some_epoch: a device-side wait timed out \(err flag set\)"):
        algo._read_tables(3, 3, what="rai_some_epoch: a device-side wait")
    algo.blocks.state.view(torch.int32)[5] = 0
    algo.blocks.state.view(torch.int32)[4] = 7  # any other word of the block is not the flag
    algo._read_tables(3, 3, what="rai_some_epoch: a device-side wait")


def test_read_back_after_the_per_minibatch_path():
    """Raw slices (rai_ppo_loss wrote the whole loss column), n_norms apart from n_steps (gradient
    accumulation), the teacher table in the same copy, and no look at the train-state block."""
    algo = _ppo(vf_coef=0.25, teacher_kl_loss_coef=5e-3, teacher_kl_loss_fn=object())
    table, norms_t, teacher_t = _tables(algo, 7)
    algo.blocks.state.view(torch.int32)[5] = 1
    stats, norms, K = algo._read_tables(3, 2, 2, teacher=True)
    np.testing.assert_array_equal(stats, table[:3])
    np.testing.assert_array_equal(norms, norms_t[:2])
    np.testing.assert_array_equal(algo._teacher_stats, teacher_t[:3])
    assert K == 2
    algo._teacher_stats = None
    algo.teacher_kl_loss_coef = 0  # the launch stays, its stat is off
    algo._read_tables(3, 2, 2, teacher=True)
    assert algo._teacher_stats is None
