"""Diagnostic: where one env step of a bench config's rollout spends its wall time (host timers with
a device synchronize after every phase), next to the unsynchronised rollout, plus the host->device
staging alternatives for the step's observation batch.  The phases are the generic step loop's own
methods (SyncStepRolloutGenerator._slot_copies ... _stage_next), so every policy kind is timed as it
runs; forward and sample are one "policy step" row (the earlier "forward graph" and "sample" rows,
merged).  A CartPole-class config is timed in this generic form, not its mapped loop.  Not part of the
product or the tests.

    python tools/rollout_timing.py --config pong --steps 64
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _pkgload  # noqa: E402

_pkgload.load()
import bench  # noqa: E402
from rl_algo_impls_amd.envs import SyntheticVecEnv  # noqa: E402
from rl_algo_impls_amd.policy import ActorCritic  # noqa: E402
from rl_algo_impls_amd.rollout import SyncStepRolloutGenerator  # noqa: E402
from rl_algo_impls_amd.running_utils import set_device_optimizations  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--config", default="pong")
p.add_argument("--num-envs", type=int, default=None)
p.add_argument("--steps", type=int, default=64)
args = p.parse_args()
cfg = bench.CONFIGS[args.config]
N, T = args.num_envs or cfg["num_envs"], cfg["n_steps"]
dev = torch.device("cuda", 0)
set_device_optimizations(dev, use_deterministic_algorithms=False)
torch.backends.cudnn.benchmark = True
torch.manual_seed(1)
env = SyntheticVecEnv(N, cfg["env"], seed=1)
policy = ActorCritic(env, **cfg["policy"]).to(dev)
gen = SyncStepRolloutGenerator(policy, env, n_steps=T, seed=1234)
sync = torch.cuda.synchronize

for _ in range(2):
    gen.rollout(0.99, 0.95)
sync()
t0 = time.perf_counter()
gen.rollout(0.99, 0.95)
sync()
whole = time.perf_counter() - t0
print(f"whole rollout {T} steps x {N} envs: {whole * 1e3:.1f} ms = {whole * 1e3 / T:.3f} ms/step", flush=True)

# the generic step's phases, the generator's own methods, synchronising after every phase
h_rew, h_done = gen.h_rew.numpy(), gen.h_done.numpy()
ph = {k: [] for k in ("slot copies", "policy step", "D2H act + sync", "env.step + results", "reward/done H2D",
                      "stage obs (+ masks)")}


def lap(name, t0):
    sync()
    t1 = time.perf_counter()
    ph[name].append(t1 - t0)
    return t1


policy.eval()
with torch.no_grad():
    for s in range(args.steps):
        s_ = s % T
        t = time.perf_counter()
        gen._slot_copies(s_)
        t = lap("slot copies", t)
        gen._policy_step(s_)
        t = lap("policy step", t)
        acts = gen._actions_to_host(s_)
        t = lap("D2H act + sync", t)
        obs = gen._env_step(acts, h_rew, h_done)
        t = lap("env.step + results", t)
        gen._results_to_device(s_)
        t = lap("reward/done H2D", t)
        gen._stage_next(obs)
        t = lap("stage obs (+ masks)", t)
tot = 0.0
for k, v in ph.items():
    m = float(np.median(v)) * 1e3
    tot += m
    print(f"  {k:24s} median {m:7.3f} ms", flush=True)
print(f"  {'sum of medians':24s}        {tot:7.3f} ms", flush=True)

# staging alternatives for one observation batch (median of 20)
obs = env._obs()
h = gen.h_obs
d = gen.next_obs_dev


def med(fn, n=20):
    xs = []
    for i in range(n):
        o = env._pool[i % len(env._pool)]
        sync()
        a = time.perf_counter()
        fn(o)
        sync()
        xs.append(time.perf_counter() - a)
    return float(np.median(xs)) * 1e3


print(f"obs batch {obs.nbytes / 1e6:.1f} MB, torch threads {torch.get_num_threads()}", flush=True)
print(f"  np.copyto -> pinned                 {med(lambda o: np.copyto(h.numpy(), o)):7.3f} ms", flush=True)
print(f"  torch copy_ -> pinned               {med(lambda o: h.copy_(torch.from_numpy(o))):7.3f} ms", flush=True)
print(f"  pinned -> device (H2D)              {med(lambda o: d.copy_(h, non_blocking=True)):7.3f} ms", flush=True)
print(f"  np.copyto + H2D                     "
      f"{med(lambda o: (np.copyto(h.numpy(), o), d.copy_(h, non_blocking=True))):7.3f} ms", flush=True)
print(f"  torch copy_ + H2D                   "
      f"{med(lambda o: (h.copy_(torch.from_numpy(o)), d.copy_(h, non_blocking=True))):7.3f} ms", flush=True)
print(f"  pageable -> device (direct)         {med(lambda o: d.copy_(torch.from_numpy(o))):7.3f} ms", flush=True)
H = N // 2


def halves(o):
    ot = torch.from_numpy(o)
    h[:H].copy_(ot[:H])
    d[:H].copy_(h[:H], non_blocking=True)
    h[H:].copy_(ot[H:])
    d[H:].copy_(h[H:], non_blocking=True)


print(f"  torch copy_ + H2D in two halves      {med(halves):7.3f} ms", flush=True)
