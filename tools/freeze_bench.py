"""Same-process timing of the run-wise clip + optimizer step (rai_clip_optim_step_runs) next to the flat one
(rai_clip_optim_step, the yardstick: unchanged code), and of the graph-replayed per-minibatch PPO step of the
IMPALA policy (3x64x64 uint8, B = 256) and the NatureCNN policy (4x84x84, B = 256) with nothing frozen, a
frozen backbone, and a frozen backbone + policy head.

Optimizer forms, at P = 1,687,719 (the C3 policy) and P = 9,155 (C2), Adam, clipping on:
    flat        rai_clip_optim_step
    runs1       one active run [0, P)
    runs3       three active runs (cuts off every multiple of 4), lags 0 / 2 / 0
    runs_frozen the same three runs with the largest one frozen
Device events around --calls calls (default 500) per form, the forms alternated within each of 5 repeats; per
form the median and the min..max over the repeats, and the bytes the algorithm needs (28 B per element of an
active Adam run: g, p, m, v read, p, m, v written, g zeroed = 32 B with the zero store; 4 B per element of a
frozen run).

Every part runs in a child process of its own under its own time limit (the parent never touches the GPU),
with at most 16 CPU threads.  One JSON line per figure, also written to profiles/freeze_bench_mi355x.txt.

    python tools/freeze_bench.py [--calls 500] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
REPEATS = 5


def _setup():
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    import _pkgload

    _pkgload.load()
    assert torch.cuda.is_available(), "freeze_bench needs a HIP device"
    return torch, torch.device("cuda:0")


def child_optim(calls):
    import numpy as np

    torch, dev = _setup()
    from rl_algo_impls_amd import _lib
    from rl_algo_impls_amd.optim import struct_to_device

    L = _lib.lib()
    for P in (1_687_719, 9_155):
        g = torch.Generator().manual_seed(P)
        p, m = (torch.randn(P, generator=g).to(dev) for _ in range(2))
        v = torch.rand(P, generator=g).to(dev)
        grad_src = torch.randn(P, generator=g).to(dev)
        grad = grad_src.clone()
        hp = struct_to_device(_lib.OptimHparams(lr=1e-6, beta1=0.9, beta2=0.999, eps=1e-7, alpha=0.99,
                                                max_grad_norm=0.5, kind=0, beta1_d=0.9, beta2_d=0.999), dev)
        state = struct_to_device(_lib.TrainState(opt_step=10), dev)
        ws = torch.zeros(int(L.rai_optim_workspace_bytes(P)), dtype=torch.uint8, device=dev)
        c1, c2 = P // 5 + 1, P // 5 + 1 + (3 * P) // 5 + 1  # run 2 is the largest; cuts off the multiples of 4
        tables = {"runs1": [(0, P, 0, 1)], "runs3": [(0, c1, 0, 1), (c1, c2, 2, 1), (c2, P, 0, 1)],
                  "runs_frozen": [(0, c1, 0, 1), (c1, c2, 2, 0), (c2, P, 0, 1)]}
        dev_tables = {}
        for name, runs in tables.items():
            arr = (_lib.OptimRun * _lib.RAI_OPTIM_MAX_RUNS)()
            for k, (b, e, lag, act) in enumerate(runs):
                arr[k] = _lib.OptimRun(begin=b, end=e, lag=lag, active=act)
            dev_tables[name] = (struct_to_device(arr, dev), len(runs))
        st = _lib.stream_handle(dev)
        head = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), P, hp.data_ptr(), state.data_ptr())
        tail = (None, 0, ws.data_ptr(), ws.numel(), st)

        def call(form):
            if form == "flat":
                rc = L.rai_clip_optim_step(*head, *tail)
            else:
                t, n = dev_tables[form]
                rc = L.rai_clip_optim_step_runs(*head, t.data_ptr(), n, *tail)
            assert rc == 0, rc

        forms = ["flat", "runs1", "runs3", "runs_frozen"]
        times = {f: [] for f in forms}
        for f in forms:  # warm-up
            for _ in range(20):
                call(f)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            for f in forms:
                # (the step zeroes the gradient; a zero gradient takes the same loads, stores and arithmetic)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call(f)
                e1.record()
                torch.cuda.synchronize()
                times[f].append(e0.elapsed_time(e1) * 1e3 / calls)
        for f in forms:
            runs = tables.get(f, [(0, P, 0, 1)])
            nbytes = sum((e - b) * (32 if act else 4) for b, e, _, act in runs)
            t = np.array(times[f])
            print(json.dumps(dict(part="optim", P=P, form=f, us_per_call_median=round(float(np.median(t)), 3),
                                  us_min=round(float(t.min()), 3), us_max=round(float(t.max()), 3), repeats=REPEATS,
                                  calls=calls, algorithm_bytes=int(nbytes),
                                  GBps_at_median=round(nbytes / float(np.median(t)) / 1e3, 1))), flush=True)


SETTINGS = {"none": {}, "backbone": dict(freeze_backbone=True),
            "backbone+policy_head": dict(freeze_backbone=True, freeze_policy_head=True)}


def child_step(kind):
    import numpy as np

    torch, dev = _setup()
    from rl_algo_impls_amd.envs import Box, Discrete
    from rl_algo_impls_amd.policy import ActorCritic
    from rl_algo_impls_amd.ppo import PPO
    from rl_algo_impls_amd.rollout import DeviceRollout

    class Env:
        def __init__(self, obs, act):
            self.num_envs, self.single_observation_space, self.single_action_space = 1, obs, act
            self.unwrapped = self

    B, NMB = 256, 8
    if kind == "impala":
        shape, n_act, kw = (3, 64, 64), 15, dict(activation_fn="relu", cnn_style="impala", cnn_flatten_dim=256)
    else:
        shape, n_act, kw = (4, 84, 84), 6, dict(activation_fn="relu")
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(0, 256, (NMB, B) + shape, dtype=torch.uint8, generator=g).to(dev)
    for name, flags in SETTINGS.items():
        torch.manual_seed(3)
        pol = ActorCritic(Env(Box(0, 255, shape, np.uint8), Discrete(n_act)), **kw).to(dev)
        algo = PPO(pol, dev, None, batch_size=B, n_epochs=1, learning_rate=1e-5, **flags)
        with torch.no_grad():
            actions = torch.randint(0, n_act, (NMB * B,), generator=g).to(dev)
            logp, v = [], []
            for i in range(NMB):
                lp, _, vv = pol(obs[i], actions[i * B:(i + 1) * B])
                logp.append(lp)
                v.append(vv)
        values = torch.stack(v)
        adv = torch.randn(NMB, B, generator=g).to(dev)
        r = DeviceRollout.from_fields(dev, obs, actions.reshape(NMB, B), values, adv, values + adv, torch.stack(logp),
                                      perm_keys=lambda: 5)
        for _ in range(2):  # capture, then one replayed update
            algo.update(r)
        assert algo._graphed is not None
        t = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            algo.update(r)
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / NMB)
        t = np.array(t)
        print(json.dumps(dict(part="step", policy=kind, B=B, frozen=name, minibatches_per_update=NMB,
                              us_per_step_median=round(float(np.median(t)), 1), us_min=round(float(t.min()), 1),
                              us_max=round(float(t.max()), 1), repeats=REPEATS,
                              note="one update of 8 replayed minibatch steps incl. the epoch gather, / 8")),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "optim":
        return child_optim(a.calls)
    if a.child:
        return child_step(a.child)
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "16"))
    lines = []
    for part in ("optim", "impala", "nature"):
        try:
            out = subprocess.run([sys.executable, __file__, "--child", part, "--calls", str(a.calls)], env=env,
                                 capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"{part}: time limit of {a.timeout} s; stopping", file=sys.stderr)
            sys.exit(124)
        got = [l for l in out.stdout.splitlines() if l.startswith("{")]
        print("\n".join(got), flush=True)
        lines += got
        if out.returncode != 0:  # nothing more is started on the GPU after a failed part
            sys.stderr.write(out.stderr[-4000:])
            sys.exit(out.returncode if out.returncode > 0 else 1)
    prof = ROOT / "profiles"
    prof.mkdir(exist_ok=True)
    (prof / "freeze_bench_mi355x.txt").write_text("\n".join(lines) + "\n")
    print(f"wrote profiles/freeze_bench_mi355x.txt ({len(lines)} lines)")


if __name__ == "__main__":
    main()
