"""The reference-AI rollout generator on the device (4x4 map, N <= 8, T <= 8): the device path against the CPU
path on the same env seed and weights, graph replay against eager, no action device-to-host copy without
log-probs, the illegal-action counts, one ACBC update from a reference rollout against the same losses in
plain torch on the CPU path's rollout, and ACBC learning the bot over a few updates."""
import numpy as np
import pytest
import torch

from rl_algo_impls_amd.envs import ScriptedBotDiscreteVecEnv, ScriptedBotGridVecEnv
from rl_algo_impls_amd.policy import ActorCritic
from rl_algo_impls_amd.reference_rollout import ReferenceAIRolloutGenerator

pytestmark = pytest.mark.gpu

SQUNET_KW = dict(actor_head_style="squeeze_unet", channels_per_level=[8, 16], strides_per_level=[2],
                 encoder_residual_blocks_per_level=[1, 1], critic_channels=16)
T, N = 6, 5
INT_FIELDS = ("actions", "action_masks", "episode_starts", "rewards", "invalid_actions")


def make(device, grid=True, include_logp=False, illegal_every=0, state=None, n_steps=T, num_envs=N):
    torch.manual_seed(5)
    if grid:
        env = ScriptedBotGridVecEnv(num_envs, map_hw=(4, 4), seed=3, illegal_every=illegal_every)
        pol = ActorCritic(env, **SQUNET_KW)
    else:
        env = ScriptedBotDiscreteVecEnv(num_envs, n=6, seed=3, illegal_every=illegal_every)
        pol = ActorCritic(env)
    if state is not None:
        pol.load_state_dict(state)
    pol = pol.to(device)
    gen = ReferenceAIRolloutGenerator(pol, env, n_steps=n_steps, include_logp=include_logp, seed=11)
    return env, pol, gen


def fields(gen):
    return {k: getattr(gen, k).cpu().numpy().copy() for k in INT_FIELDS + ("values", "obs")}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("grid", [True, False], ids=["gridnet", "discrete"])
@pytest.mark.parametrize("illegal_every", [0, 4])
def test_device_path_equals_cpu_path(dev, grid, illegal_every):
    """illegal_every: the counts are those of the CPU path, masked-out actions only (no update is run)."""
    _, pol_c, gen_c = make(torch.device("cpu"), grid, illegal_every=illegal_every)
    state = {k: v.clone() for k, v in pol_c.state_dict().items()}
    r_c = gen_c.rollout(gamma=0.99, gae_lambda=0.95)
    _, _, gen_d = make(dev, grid, illegal_every=illegal_every, state=state)
    r_d = gen_d.rollout(gamma=0.99, gae_lambda=0.95)
    fc, fd = fields(gen_c), fields(gen_d)
    for k in INT_FIELDS + ("obs",):
        assert fc[k].dtype == fd[k].dtype and fc[k].tobytes() == fd[k].tobytes(), k
    np.testing.assert_allclose(fd["values"], fc["values"], rtol=1e-5, atol=1e-6)
    assert r_d.logprobs is None and r_c.logprobs is None
    assert gen_d.invalid_action_count == gen_c.invalid_action_count
    assert (gen_d.invalid_action_count > 0) == (illegal_every > 0)
    if illegal_every:
        assert fd["invalid_actions"].max() == 1  # one masked-out component per marked (step, env) pair


def test_graph_replay_equals_eager(dev, monkeypatch):
    _, pol, gen = make(dev)
    assert gen.rollout_graph
    gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert gen._fwd_graph is not None, "the value forward is graph-replayed"
    want = fields(gen)
    monkeypatch.setenv("RAI_ROLLOUT_GRAPH", "0")
    _, _, eager = make(dev, state={k: v.clone() for k, v in pol.state_dict().items()})
    assert not eager.rollout_graph
    eager.rollout(gamma=0.99, gae_lambda=0.95)
    got = fields(eager)
    for k in INT_FIELDS:
        assert got[k].tobytes() == want[k].tobytes(), k
    np.testing.assert_allclose(got["values"], want["values"], rtol=1e-5, atol=1e-6)


def test_no_action_copy_without_logp(dev, monkeypatch):
    _, _, gen = make(dev)

    def refuse(self, s):
        raise AssertionError("an action device-to-host copy without log-probs")

    monkeypatch.setattr(ReferenceAIRolloutGenerator, "_actions_to_host", refuse)
    off0 = gen.rng_offset
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert gen.rng_offset == off0 and r.logprobs is None and gen.invalid_action_count == 0


def test_with_logp_records_the_bot_and_keeps_every_slot(dev):
    env, _, gen = make(dev, include_logp=True)
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    lp = r.logprobs.cpu().numpy()
    assert lp.shape == (T, N) and len({lp[s].tobytes() for s in range(T)}) == T
    assert gen.rng_offset == T
    acts, obs, masks = r.actions.cpu().numpy(), r.obs.cpu().numpy(), r.action_masks.cpu().numpy()
    for s in range(T):
        np.testing.assert_array_equal(acts[s], env.bot_action(obs[s], masks[s]))
        assert env.received[s].any(), "the env received the sampled actions"


def torch_acbc_losses(pol, r):
    """acbc.py:94-128 on the whole rollout in plain torch: pi_loss = -mean(logp), v_loss = mean((v - R)^2)."""
    fl = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))
    with torch.no_grad():
        logp, _, v = pol(fl(r.obs), fl(r.actions), action_masks=fl(r.action_masks))
        return float(-logp.double().mean()), float(((v - fl(r.returns)).double() ** 2).mean())


def test_one_acbc_update_from_a_reference_rollout(dev):
    """A Discrete policy (its head has a torch form on the CPU): the device update's pi_loss / v_loss of its one
    full-batch step against the same losses in torch on the CPU path's rollout (tolerances of
    test_gpu_acbc.py's scalars)."""
    from rl_algo_impls_amd.acbc import ACBC

    _, pol_c, gen_c = make(torch.device("cpu"), grid=False, n_steps=8, num_envs=8)
    state = {k: v.clone() for k, v in pol_c.state_dict().items()}
    r_c = gen_c.rollout(gamma=0.99, gae_lambda=0.95)
    pi_ref, v_ref = torch_acbc_losses(pol_c, r_c)
    _, pol_d, gen_d = make(dev, grid=False, state=state, n_steps=8, num_envs=8)
    algo = ACBC(pol_d, dev, None, learning_rate=1e-3, batch_size=64, n_epochs=1, vf_coef=0.25, gamma=0.99,
                gae_lambda=0.95)
    algo.learn(64, gen_d)  # one rollout, one full-batch step
    stats = algo.last_train_stats.step_stats
    print("pi_loss", stats["pi_loss"], pi_ref, "v_loss", stats["v_loss"], v_ref)
    np.testing.assert_allclose(stats["pi_loss"], pi_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(stats["v_loss"], v_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(stats["loss"], pi_ref + 0.25 * v_ref, rtol=1e-4, atol=1e-6)


def bot_match_share(pol, env, gen):
    """Share of (live) components where the policy's masked argmax is the bot's action."""
    obs = torch.from_numpy(np.concatenate(env._pool)).to(gen.device)
    masks = env.mask_of(obs.cpu().numpy())
    bot = env.bot_action(obs.cpu().numpy(), masks)
    mode = pol.act(obs.cpu().numpy(), deterministic=True, action_masks=masks)
    live = masks.any(axis=-1)
    return float((np.asarray(mode).reshape(bot.shape) == bot)[live].mean())


def test_acbc_learns_the_bot(dev):
    from rl_algo_impls_amd.acbc import ACBC

    env, pol, gen = make(dev, grid=False, n_steps=8, num_envs=8)
    algo = ACBC(pol, dev, None, learning_rate=3e-3, batch_size=64, n_epochs=4, vf_coef=0.25, gamma=0.99,
                gae_lambda=0.95)
    share0 = bot_match_share(pol, env, gen)
    pi = []
    for _ in range(6):
        algo.learn(64, gen)
        pi.append(algo.last_train_stats.step_stats["pi_loss"])
    share1 = bot_match_share(pol, env, gen)
    print("pi_loss", pi, "share", share0, share1)
    assert gen.invalid_action_count == 0
    assert pi[-1] < pi[0]
    assert share1 > share0


def test_host_stages_wait_for_their_copies_when_the_forward_is_slow(dev, monkeypatch):
    """Without log-probs no action wait drains the stream, so a forward slower than the env would let the host
    refill the pinned staging buffers (rewards, dones, observations, masks, the bot's actions) before the
    queued copies have read them.  Here every value step is preceded by ~10 ms of queued matmuls, against an
    env that answers in well under a millisecond: the fields must still be the CPU path's, bit for bit, and
    at every host write the previous step's copies have completed."""
    _, pol_c, gen_c = make(torch.device("cpu"))
    state = {k: v.clone() for k, v in pol_c.state_dict().items()}
    gen_c.rollout(gamma=0.99, gae_lambda=0.95)
    _, _, gen_d = make(dev, state=state)
    a = torch.randn(4096, 4096, device=dev)
    value_step = gen_d._value_step

    def slow_value_step(s):
        b = a
        for _ in range(12):
            b = (b @ a) * 1e-2
        value_step(s)

    drained = []
    take = gen_d._take_env_results

    def checked_take(*args):
        drained.append(gen_d._staged.query())
        take(*args)

    monkeypatch.setattr(gen_d, "_value_step", slow_value_step)
    monkeypatch.setattr(gen_d, "_take_env_results", checked_take)
    gen_d.rollout(gamma=0.99, gae_lambda=0.95)
    assert drained == [True] * T
    fc, fd = fields(gen_c), fields(gen_d)
    for k in INT_FIELDS + ("obs",):
        assert fc[k].tobytes() == fd[k].tobytes(), k
    np.testing.assert_array_equal(gen_d.next_episode_starts.cpu().numpy(), gen_c.next_episode_starts.numpy())
    np.testing.assert_allclose(fd["values"], fc["values"], rtol=1e-5, atol=1e-6)


def test_one_acbc_update_from_a_gridnet_reference_rollout(dev):
    """The MicroRTS path end to end: GridNet actions written by rai_ref_actions_store, consumed by ACBC's
    rai_gridnet_* update.  The step's pi_loss is -mean(logp) of the policy's own forward on the rollout before
    the step (test_gpu_acbc.py's scalar tolerances), the stats are finite and nothing was counted."""
    from rl_algo_impls_amd.acbc import ACBC

    _, pol, gen = make(dev, n_steps=8, num_envs=8)
    algo = ACBC(pol, dev, None, learning_rate=1e-3, batch_size=64, n_epochs=1, vf_coef=0.25, gamma=0.99,
                gae_lambda=0.95)
    r = gen.rollout(gamma=0.99, gae_lambda=0.95)
    assert gen.invalid_action_count == 0
    pi_ref, v_ref = torch_acbc_losses(pol, r)
    before = algo.flat.flat.detach().clone()

    class Once:
        def rollout(self, gamma, gae_lambda):
            return r

    algo.learn(64, Once())
    stats = algo.last_train_stats.step_stats
    print("gridnet pi_loss", stats["pi_loss"], pi_ref, "v_loss", stats["v_loss"], v_ref)
    assert all(np.isfinite(stats[k]) for k in ("loss", "pi_loss", "v_loss"))
    np.testing.assert_allclose(stats["pi_loss"], pi_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(stats["v_loss"], v_ref, rtol=1e-4, atol=1e-6)
    after = algo.flat.flat.detach()
    assert torch.isfinite(after).all() and not torch.equal(before, after)


def test_data_parallel_is_refused(dev):
    from rl_algo_impls_amd.ppo import PPO

    _, pol, gen = make(dev, grid=False, include_logp=True)
    algo = PPO(pol, dev, None, batch_size=30, n_epochs=1)
    algo.world = 2  # as after enable_data_parallel on a second rank
    with pytest.raises(NotImplementedError, match="ReferenceAIRolloutGenerator under data parallel"):
        algo.learn_epoch(0, 30, gen)
    assert gen.rng_offset == 0, "refused before the rollout"
