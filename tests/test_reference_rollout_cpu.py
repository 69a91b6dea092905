"""The reference-AI rollout generator without a GPU: the host twin of rai_ref_actions_store against the integer
oracle on the kernel test's case list, the generator's CPU path on the scripted-bot envs (what it records, what
the env receives, what it does not touch), the illegal-action count, the registry and the refusals."""
import logging
import sys

import numpy as np
import pytest
import torch

import ref_actions_ref as R
from conftest import GOLDEN
from rl_algo_impls_amd import registry
from rl_algo_impls_amd.envs import (Box, MaskedMultiDiscreteVecEnv, ScriptedBotDiscreteVecEnv, ScriptedBotGridVecEnv,
                                    SyntheticVecEnv)
from rl_algo_impls_amd.policy import ActorCritic
from rl_algo_impls_amd.reference_rollout import ReferenceAIRolloutGenerator, store_host
from rl_algo_impls_amd.rollout import SyncStepRolloutGenerator

CPU = torch.device("cpu")
SQUNET_KW = dict(actor_head_style="squeeze_unet", channels_per_level=[8, 16], strides_per_level=[2],
                 encoder_residual_blocks_per_level=[1, 1], critic_channels=16)
T, N = 6, 3


@pytest.mark.parametrize("name,nvec,cells,n,dtype,with_mask,seed", R.cases(), ids=[c[0] for c in R.cases()])
def test_host_twin_matches_oracle(name, nvec, cells, n, dtype, with_mask, seed):
    src, mask = R.make_case(nvec, cells, n, dtype, with_mask, seed)
    want_dst, want_bad = R.oracle(src, nvec, mask, cells)
    dst, bad = store_host(src, nvec, mask, cells)
    assert dst.dtype == np.int64 and bad.dtype == np.int32
    np.testing.assert_array_equal(dst, want_dst)
    np.testing.assert_array_equal(bad, want_bad)


def test_host_twin_converts_other_integer_dtypes():
    src = np.array([[5, 200, 3]], dtype=np.uint8)
    dst, bad = store_host(src, (6, 4, 4), None, 1)
    np.testing.assert_array_equal(dst, [[5, 0, 3]])
    np.testing.assert_array_equal(bad, [1])
    dst, bad = store_host(np.array([[2**63 + 5, 1, 1]], dtype=np.uint64), (6, 4, 4), None, 1)
    np.testing.assert_array_equal(dst, [[0, 1, 1]])
    np.testing.assert_array_equal(bad, [1])


def grid_setup(include_logp=False, illegal_every=0, seed=3):
    torch.manual_seed(5)
    env = ScriptedBotGridVecEnv(N, map_hw=(4, 4), seed=seed, illegal_every=illegal_every)
    pol = ActorCritic(env, **SQUNET_KW).to(CPU)
    gen = ReferenceAIRolloutGenerator(pol, env, n_steps=T, include_logp=include_logp, seed=11)
    return env, pol, gen


def test_scripted_bot_env_is_legal_and_has_empty_cells_and_groups():
    env = ScriptedBotGridVecEnv(8, map_hw=(4, 4), seed=2)
    obs, _ = env.reset()
    mask = env.get_action_mask()
    assert mask.shape == (8, 16, 78) and mask.dtype == np.bool_
    rows = mask.reshape(-1, 78)
    live = rows.any(axis=1)
    assert live.any() and (~live).any(), "some cells hold no unit"
    off = np.concatenate([[0], np.cumsum(R.GRID_NVEC)])
    dead_groups = sum(int((~rows[live][:, off[g]:off[g + 1]].any(axis=1)).sum()) for g in range(7))
    assert dead_groups > 0, "some groups inside live cells are all false"
    env.step(np.zeros((8, 16, 7), dtype=np.int64))
    assert env.last_action.dtype == np.int32 and env.last_action.shape == (8, 16, 7)
    _, bad = R.oracle(env.last_action, R.GRID_NVEC, mask, 16)
    assert not bad.any(), "the bot's actions are legal"
    np.testing.assert_array_equal(env.last_action, env.bot_action(obs, mask))  # a function of obs and mask


def test_records_the_bots_actions_without_logp():
    env, pol, gen = grid_setup()
    offset0 = gen.rng_offset
    seen = []
    step = env.step

    def spy(actions):
        out = step(actions)
        seen.append((env.last_action.copy(), env.get_action_mask().copy()))
        return out

    env.step = spy
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert r.logprobs is None
    assert gen.rng_offset == offset0, "no sampling: no RNG offset consumed"
    assert gen.invalid_action_count == 0 and not gen.invalid_actions.any()
    assert gen.invalid_actions.shape == (T, N) and gen.invalid_actions.dtype == torch.int32
    assert r.actions.dtype == torch.int64 and tuple(r.actions.shape) == (T, N, 16, 7)
    for s in range(T):
        np.testing.assert_array_equal(r.actions[s].numpy(), seen[s][0])
        # the stored mask is the one the bot acted under: the mask of the slot's own observation
        np.testing.assert_array_equal(r.action_masks[s].numpy(), env.mask_of(r.obs[s].numpy()))
        np.testing.assert_array_equal(r.actions[s].numpy(), env.bot_action(r.obs[s].numpy(),
                                                                           r.action_masks[s].numpy()))
        if s + 1 < T:
            np.testing.assert_array_equal(r.action_masks[s + 1].numpy(), seen[s][1])
    assert len(env.received) == T
    for a in env.received:
        assert a.shape == (N, 16, 7) and a.dtype == np.int64 and not a.any()
    with torch.no_grad():
        pol.eval()
        for s in range(T):
            np.testing.assert_allclose(r.values[s].numpy(), pol.network.value(r.obs[s]).numpy(), rtol=1e-5,
                                       atol=1e-6)
    # GAE of the CPU path against the project's C oracle of the reference's compute_advantages
    import oracle

    adv, ret = oracle.gae_c(r.rewards.numpy(), r.values.numpy(), r.episode_starts.numpy(),
                            r.next_episode_starts.numpy(), r.next_values.numpy(), 0.99, 0.95)
    np.testing.assert_allclose(r.advantages.numpy(), adv, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r.returns.numpy(), ret, rtol=1e-5, atol=1e-6)


def test_with_logp_the_env_gets_the_samples_and_the_batch_the_bots_actions():
    torch.manual_seed(5)
    env = ScriptedBotDiscreteVecEnv(N, n=6, seed=4)
    pol = ActorCritic(env).to(CPU)
    gen = ReferenceAIRolloutGenerator(pol, env, n_steps=T, include_logp=True, seed=11)
    sampled = []
    step = pol.step

    def spy(obs, action_masks=None):
        st = step(obs, action_masks=action_masks)
        sampled.append((np.array(st.a), np.array(st.logp_a)))
        return st

    pol.step = spy
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert r.logprobs is not None and tuple(r.logprobs.shape) == (T, N)
    for s in range(T):
        np.testing.assert_array_equal(env.received[s], sampled[s][0])
        np.testing.assert_array_equal(r.logprobs[s].numpy(), sampled[s][1].astype(np.float32))
        np.testing.assert_array_equal(r.actions[s].numpy(), env.bot_action(r.obs[s].numpy(),
                                                                           r.action_masks[s].numpy()))
    lp = r.logprobs.numpy()
    assert len({lp[s].tobytes() for s in range(T)}) == T, "T distinct log-prob slots"
    assert gen.invalid_action_count == 0


def expected_invalid(env, r, every):
    want = np.zeros((T, N), dtype=np.int32)
    for s in range(T):
        masks = r.action_masks[s].numpy()
        for n in range(N):
            if (s * N + n) % every == every - 1 and env.illegal_component(masks[n]) is not None:
                want[s, n] = 1
    return want


@pytest.mark.parametrize("flat", [False, True])
def test_illegal_actions_are_counted_and_warned(caplog, flat):
    if flat:
        torch.manual_seed(5)
        env = ScriptedBotDiscreteVecEnv(N, n=6, seed=4, illegal_every=5)
        gen = ReferenceAIRolloutGenerator(ActorCritic(env).to(CPU), env, n_steps=T, include_logp=False, seed=11)
    else:
        env, _, gen = grid_setup(illegal_every=5)
    with caplog.at_level(logging.WARNING):
        r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    want = expected_invalid(env, r, 5)
    assert want.sum() > 0
    np.testing.assert_array_equal(gen.invalid_actions.numpy(), want)
    assert gen.invalid_action_count == int(want.sum())
    assert any("reference-AI rollout" in rec.getMessage() and rec.levelno == logging.WARNING
               for rec in caplog.records)
    # masked-out actions are stored as they are
    for s in range(T):
        clean = env.bot_action(r.obs[s].numpy(), r.action_masks[s].numpy())
        assert int((r.actions[s].numpy() != clean).sum()) == int(want[s].sum())
    # the next rollout overwrites the counts
    env.illegal_every = 0
    gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert gen.invalid_action_count == 0 and not gen.invalid_actions.any()


def test_flat_multidiscrete_records_last_action():
    torch.manual_seed(5)
    env = MaskedMultiDiscreteVecEnv(4, seed=2)
    step = env.step

    def bot_step(actions):  # a bot that plays the first valid entry of every group, as int16
        m = env.get_action_mask()
        off = np.concatenate([[0], np.cumsum(env.nvec)])
        env.last_action = np.stack([m[:, off[g]:off[g + 1]].argmax(1) for g in range(3)], 1).astype(np.int16)
        return step(actions)

    env.step = bot_step
    gen = ReferenceAIRolloutGenerator(ActorCritic(env).to(CPU), env, n_steps=4, include_logp=False, seed=1)
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert tuple(r.actions.shape) == (4, 4, 3) and gen.invalid_action_count == 0
    off = np.concatenate([[0], np.cumsum(env.nvec)])
    for s in range(4):
        m = r.action_masks[s].numpy()
        want = np.stack([m[:, off[g]:off[g + 1]].argmax(1) for g in range(3)], 1)
        np.testing.assert_array_equal(r.actions[s].numpy(), want)


def test_registry_and_export():
    import rl_algo_impls_amd as pkg

    assert registry.ROLLOUT_GENERATORS == {"sync": SyncStepRolloutGenerator,
                                           "reference": ReferenceAIRolloutGenerator}
    assert issubclass(ReferenceAIRolloutGenerator, SyncStepRolloutGenerator)
    assert pkg.ReferenceAIRolloutGenerator is ReferenceAIRolloutGenerator
    assert registry.DEFAULT_ROLLOUT_GENERATORS["acbc"] is SyncStepRolloutGenerator


def test_refusals():
    class BoxEnv:
        num_envs = 2
        single_observation_space = Box(-np.inf, np.inf, (4,), np.float32)
        single_action_space = Box(-1.0, 1.0, (2,), np.float32)
        unwrapped = None

    with pytest.raises(NotImplementedError, match="Box"):
        ReferenceAIRolloutGenerator(object(), BoxEnv())

    class DictSpace(dict):
        pass

    class DictEnv(BoxEnv):
        single_action_space = DictSpace(per_position=None, pick_position=None)

    with pytest.raises(NotImplementedError, match="dict"):
        ReferenceAIRolloutGenerator(object(), DictEnv())

    torch.manual_seed(1)
    env = SyntheticVecEnv(2, "cartpole", seed=1)  # no last_action
    gen = ReferenceAIRolloutGenerator(ActorCritic(env).to(CPU), env, n_steps=2, include_logp=False)
    with pytest.raises(AttributeError, match="last_action"):
        gen.rollout(gamma=0.99, gae_lambda=0.95)

    env = ScriptedBotDiscreteVecEnv(2, seed=1)
    gen = ReferenceAIRolloutGenerator(ActorCritic(env).to(CPU), env, n_steps=2, include_logp=False)
    step = env.step

    def dict_step(actions):
        out = step(actions)
        env.last_action = {"per_position": env.last_action, "pick_position": env.last_action}
        return out

    env.step = dict_step
    with pytest.raises(NotImplementedError, match="dict last_action"):
        gen.rollout(gamma=0.99, gae_lambda=0.95)


def test_golden_rollout_of_the_reference_generator(golden):
    """tests/golden/make_golden_reference_rollout.py: the reference's own ReferenceAIRolloutGenerator on an env
    replaying a recorded script (T = 6, N = 3, 4x4 map, three reward columns), the weights of
    the fixture's small squeeze-U-Net (K = 3 critics, per-critic gamma / lambda).  Our generator on
    an env replaying the same script with the same weights: integer fields and rewards exactly, values within
    the values tolerance, advantages / returns within the GAE tests' float32 tolerance (rtol = atol = 1e-5)."""
    z = golden("reference_rollout.npz")
    script = {k[len("script_"):]: z[k] for k in z.files if k.startswith("script_")}
    Tg, Ng = script["dones"].shape

    class ReplayEnv(ScriptedBotGridVecEnv):
        def __init__(self):
            super().__init__(Ng, map_hw=(4, 4), seed=0)
            self.t = 0

        def reset(self, **kw):
            return script["obs"][0], {}

        def get_action_mask(self):
            return script["masks"][self.t]

        def step(self, actions):
            self.received.append(np.array(actions, copy=True))
            t = self.t
            self.last_action = script["last_action"][t]
            self.t += 1
            return script["obs"][t + 1], script["rewards"][t], script["dones"][t], np.zeros(Ng, dtype=np.bool_), {}

    env = ReplayEnv()
    sys.path.insert(0, str(GOLDEN))
    from make_golden_reference_rollout import POLICY_KW  # numpy / torch imports only at module level

    pol = ActorCritic(env, **POLICY_KW).to(CPU)
    pre = "init/"
    pol.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}, strict=True)
    gen = ReferenceAIRolloutGenerator(pol, env, n_steps=Tg, include_logp=False,
                                      subaction_mask=POLICY_KW["subaction_mask"])
    r = gen.rollout(gamma=z["gamma"], gae_lambda=z["gae_lambda"])
    assert r.logprobs is None and gen.invalid_action_count == 0
    np.testing.assert_array_equal(r.actions.numpy(), z["rollout_actions"])
    np.testing.assert_array_equal(r.episode_starts.numpy(), z["rollout_episode_starts"])
    np.testing.assert_array_equal(r.next_episode_starts.numpy(), z["rollout_next_episode_starts"])
    np.testing.assert_array_equal(r.rewards.numpy(), z["rollout_rewards"])
    np.testing.assert_array_equal(r.action_masks.numpy(), z["rollout_action_masks"])
    np.testing.assert_array_equal(r.obs.numpy(), z["rollout_obs"])
    np.testing.assert_allclose(r.values.numpy(), z["rollout_values"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r.advantages.numpy(), z["rollout_advantages"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r.returns.numpy(), z["rollout_returns"], rtol=1e-5, atol=1e-5)
