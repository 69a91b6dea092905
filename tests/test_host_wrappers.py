"""Host-side rows of the path against the reference's own outputs (tests/golden/make_golden_host.py):
A16 HyperparamTransitions, A17 RunningMeanStd / Normalize* wrappers (incl. the world-2 gloo
cross-rank merge), A18 EpisodeStatsWriter.  CPU only."""
import json
import multiprocessing as mp
from types import SimpleNamespace

import numpy as np
import pytest

from rl_algo_impls_amd import callbacks, wrappers
from rl_algo_impls_amd.envs import Box

from conftest import GOLDEN


@pytest.fixture(scope="module")
def host():
    return np.load(GOLDEN / "host_wrappers.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def sched():
    return json.loads((GOLDEN / "host_schedule.json").read_text())


class FixtureEnv:
    """Replays the scripted env of make_golden_host.py (optionally a slice of its envs)."""

    def __init__(self, z, envs=slice(None)):
        self.obs, self.rew = z["env_obs"][:, envs], z["env_rew"][:, envs]
        self.term, self.trunc = z["env_term"][:, envs], z["env_trunc"][:, envs]
        self.num_envs = self.obs.shape[1]
        self.single_observation_space = Box(-np.inf, np.inf, (self.obs.shape[2],), np.float32)
        self.single_action_space = None
        self.t = 0

    @property
    def unwrapped(self):
        return self

    def reset(self, **kw):
        self.t = 0
        return self.obs[0].copy(), {}

    def step(self, actions):
        t = self.t
        self.t += 1
        return self.obs[t + 1].copy(), self.rew[t].copy(), self.term[t].copy(), self.trunc[t].copy(), {}


def test_running_mean_std_matches_reference(host):
    rms = wrappers.RunningMeanStd(shape=(3,))
    hmv = wrappers.HybridMovingMeanVar(window_size=40, shape=(3,))
    i = 0
    while f"rms_in_{i}" in host.files:
        rms.update(host[f"rms_in_{i}"])
        hmv.update(host[f"rms_in_{i}"])
        np.testing.assert_array_equal(rms.mean, host[f"rms_mean_{i}"])
        np.testing.assert_array_equal(rms.var, host[f"rms_var_{i}"])
        assert rms.count == host[f"rms_count_{i}"]
        np.testing.assert_array_equal(hmv.mean, host[f"hmv_mean_{i}"])
        np.testing.assert_array_equal(hmv.var, host[f"hmv_var_{i}"])
        i += 1
    assert i == 5


@pytest.mark.parametrize("name,kw", [("nr", {}), ("nr_emv", dict(exponential_moving_mean_var=True,
                                                                 emv_window_size=50))])
def test_normalize_wrappers_match_reference(host, name, kw):
    env = wrappers.NormalizeReward(wrappers.NormalizeObservation(FixtureEnv(host)), gamma=0.97, **kw)
    o, _ = env.reset()
    obs, rew = [o], []
    for _ in range(host["env_rew"].shape[0]):
        o, r, *_ = env.step(None)
        obs.append(o)
        rew.append(r)
    np.testing.assert_array_equal(np.stack(obs), host[f"{name}_obs"])
    np.testing.assert_array_equal(np.stack(rew), host[f"{name}_rew"])


def test_normalize_save_load_roundtrip(tmp_path, host):
    env = wrappers.NormalizeObservation(FixtureEnv(host))
    env.reset()
    env.step(None)
    env.save(str(tmp_path / "norm_obs.npz"))
    other = wrappers.NormalizeObservation(FixtureEnv(host), training=False)
    other.load(str(tmp_path / "norm_obs.npz"))
    np.testing.assert_array_equal(other.rms.mean, env.rms.mean)
    np.testing.assert_array_equal(other.rms.var, env.rms.var)
    assert float(other.rms.count) == env.rms.count


def test_hyperparam_transitions_match_reference(sched):
    for case in sched["hyperparam_transitions"]:
        c = case["case"]
        algo = SimpleNamespace(learning_rate=None, clip_range=None, ent_coef=None, multi_reward_weights=None)
        ht = callbacks.HyperparamTransitions(SimpleNamespace(n_timesteps=case["n_timesteps"]), None, algo, None,
                                             c["phases"], c["durations"], interpolate_method=c["interpolate_method"])
        for want in case["trace"]:
            for k, v in want.items():
                got = getattr(algo, k)
                np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.asarray(v, dtype=np.float64),
                                           rtol=0, atol=0, err_msg=k)
            ht.on_step(timesteps_elapsed=case["step"])


def test_hyperparam_transitions_rejects_unknown_key():
    algo = SimpleNamespace(learning_rate=1.0)
    with pytest.raises(ValueError):
        callbacks.HyperparamTransitions(SimpleNamespace(n_timesteps=10), None, algo, None,
                                        [{"reward_weights": 1}], [1.0])


def test_episode_stats_writer_matches_reference(sched):
    es = sched["episode_stats"]

    class Rec:
        def __init__(self):
            self.scalars = []

        def add_scalar(self, tag, value, global_step=None):
            self.scalars.append((tag, float(np.asarray(value))))

    class InfoEnv:
        num_envs = 4
        single_observation_space = single_action_space = None

        def __init__(self):
            self.t = 0

        @property
        def unwrapped(self):
            return self

        def reset(self, **kw):
            return None, {}

        def step(self, a):
            s = es["script"][self.t]
            self.t += 1
            if s["kind"] == "episode":
                info = {"episode": {"r": np.array(s["r"]), "l": np.array(s["l"])}, "_episode": np.array(s["mask"])}
            elif s["kind"] == "final_info":
                fi = np.array([{"episode": {"r": np.array([r]), "l": np.array([l])}} if m else None
                               for r, l, m in zip(s["r"], s["l"], s["mask"])], dtype=object)
                info = {"final_info": fi, "_final_info": np.array(s["mask"])}
            else:
                info = {}
            return None, None, None, None, info

    rec = Rec()
    w = wrappers.EpisodeStatsWriter(InfoEnv(), rec, rolling_length=es["rolling_length"])
    w.reset()
    for _ in es["script"]:
        w.step(None)
    assert [t for t, _ in rec.scalars] == [t for t, _ in es["scalars"]]
    np.testing.assert_allclose([v for _, v in rec.scalars], [v for _, v in es["scalars"]], rtol=1e-12)


def test_normalize_cross_rank_merge_world2(host):
    """Two ranks holding 3 + 5 of the 8 envs normalise like one process holding all 8."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    import dp_worker

    port = dp_worker.rendezvous()
    procs = [ctx.Process(target=dp_worker.rms_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    np.testing.assert_array_equal(res[0][2], res[1][2])  # identical statistics on every rank
    np.testing.assert_array_equal(res[0][3], res[1][3])
    obs = np.concatenate([res[0][0], res[1][0]], axis=1)
    rew = np.concatenate([res[0][1], res[1][1]], axis=1)
    np.testing.assert_allclose(obs, host["nr_obs"], rtol=1e-5, atol=1e-5)  # fp64 merge order vs f32 storage
    np.testing.assert_allclose(rew, host["nr_rew"], rtol=1e-5, atol=1e-6)
