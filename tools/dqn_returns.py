"""DQN training returns on CartPoleVecEnv with the reference's dqn.yml CartPole-v1 hyperparameters, N seeds,
on the device path (replay ring, graph-replayed gradient steps).

Writes profiles/dqn_returns_cartpole_mi355x.json in the layout of tests/golden/dqn_returns_cartpole.json (the
reference's own DQN on the same env and seeds, from tests/golden/make_golden_dqn.py returns): per seed, the
mean return of the last 50 training episodes every 5,000 timesteps.  Return parity is not claimed: DQN on
CartPole is seed-noisy, and the two samplers draw different random streams; DESIGN reports both side by side.

    python tools/dqn_returns.py [--seeds 1 2 3] [--device cuda:0]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import _pkgload  # noqa: E402

_pkgload.load()
from make_golden_dqn import EpisodeLog  # noqa: E402  (numpy-only helper; no reference import)
from rl_algo_impls_amd.dqn import DQN, DQNPolicy  # noqa: E402
from rl_algo_impls_amd.envs import CartPoleVecEnv  # noqa: E402
from rl_algo_impls_amd.replay import ReplayBufferRolloutGenerator  # noqa: E402
from rl_algo_impls_amd.running_utils import set_seeds  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--timesteps", type=int, default=50000)
    args = ap.parse_args()
    dev = torch.device(args.device)
    out = dict(env="CartPoleVecEnv (CartPole-v1 dynamics)", n_timesteps=args.timesteps, every=5000, window=50,
               device=str(dev), seeds={}, seconds={})
    for seed in args.seeds:
        set_seeds(seed)
        env = EpisodeLog(CartPoleVecEnv(1, seed=seed))
        policy = DQNPolicy(env, hidden_sizes=[256, 256]).to(dev)
        algo = DQN(policy, dev, None, learning_rate=2.3e-3, batch_size=64, gamma=0.99, target_update_interval=10,
                   gradient_steps=128, exploration_fraction=0.16, exploration_final_eps=0.04)
        gen = ReplayBufferRolloutGenerator(policy, env, buffer_size=100000, learning_starts=1000, train_freq=256,
                                           seed=seed)
        t0 = time.perf_counter()
        algo.learn(args.timesteps, gen)
        if dev.type == "cuda":
            torch.cuda.synchronize()
            assert gen.buffer.device_state()["err"] == 0
        out["seconds"][str(seed)] = round(time.perf_counter() - t0, 2)
        out["seeds"][str(seed)] = env.curve(out["every"], out["window"])
        assert np.isfinite(algo.flat.flat.cpu().numpy()).all() if dev.type == "cuda" else True
        print(seed, out["seconds"][str(seed)], "s", out["seeds"][str(seed)], flush=True)
    dst = ROOT / "profiles" / "dqn_returns_cartpole_mi355x.json"
    dst.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", dst)


if __name__ == "__main__":
    main()
