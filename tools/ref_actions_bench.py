"""Same-box timing of rai_ref_actions_store (csrc/ref_actions.hip) against the torch composition that does the
same work on the same stream: cast to int64, range test, mask gather, per-group any, masked write, per-env sum.

Shapes: GridNet planes [6, 4, 4, 4, 4, 7, 49] at (N, cells) = (28, 256) and (512, 256), the MicroRTS env counts;
Discrete(6) at (4096, 1).  int32 sources (what the env hands over), with a mask.  The child process checks the
two results equal before it times them.  One JSON line per shape: device microseconds per call from events
around `reps` calls after warm-up, ours and torch alternating in the same run, and the bytes the launch must
move (source + mask + destination + counts) over its time.  The lines are also written to
profiles/ref_actions_bench_mi355x.txt.  The measuring runs in a child process under its own time limit (the
parent never touches the GPU).

    python tools/ref_actions_bench.py [--reps 200] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
GRID = [6, 4, 4, 4, 4, 7, 49]
SHAPES = [("gridnet", GRID, 28, 256), ("gridnet", GRID, 512, 256), ("discrete", [6], 4096, 1)]


def child(reps):
    import numpy as np
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd.reference_rollout import store

    dev = torch.device("cuda:0")

    def timeit(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for name, nvec, N, cells in SHAPES:
        rng = np.random.default_rng(1)
        G, A, R = len(nvec), sum(nvec), N * cells
        nv = torch.tensor(nvec, device=dev)
        off = torch.tensor(np.concatenate([[0], np.cumsum(nvec)[:-1]]), device=dev)
        group_of = torch.repeat_interleave(torch.arange(G, device=dev), nv)
        src = torch.from_numpy(rng.integers(-1, np.asarray(nvec) + 1, size=(R, G)).astype(np.int32)).to(dev)
        mask = torch.from_numpy(rng.random((R, A)) < 0.5).to(dev)
        dst, bad = torch.empty((R, G), dtype=torch.int64, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        t_dst, t_bad = torch.empty_like(dst), torch.empty_like(bad)

        def ours():
            store(src, nvec, mask, cells, dst, bad)

        def composed():
            a = src.to(torch.int64)
            oor = (a < 0) | (a >= nv)
            safe = torch.where(oor, 0, a)
            picked = torch.gather(mask, 1, safe + off)
            anyg = torch.zeros((R, G), dtype=torch.int32, device=dev).index_add_(1, group_of, mask.to(torch.int32)) > 0
            counted = oor | (anyg & ~picked)
            t_dst.copy_(safe)
            t_bad.copy_(counted.view(N, cells * G).sum(1))

        ours()
        composed()
        torch.cuda.synchronize()
        assert torch.equal(dst, t_dst) and torch.equal(bad, t_bad), "the composition and the kernel disagree"
        for _ in range(10):
            ours()
            composed()
        rounds = [(timeit(ours, reps), timeit(composed, reps)) for _ in range(5)]
        o, t = sorted(r[0] for r in rounds), sorted(r[1] for r in rounds)
        nbytes = R * G * 4 + R * A + R * G * 8 + N * 4
        print(json.dumps(dict(head=name, N=N, cells=cells, nvec=nvec, src="int32", ours_us=round(o[2], 2),
                              ours_us_min_max=[round(o[0], 2), round(o[-1], 2)], torch_us=round(t[2], 2),
                              torch_us_min_max=[round(t[0], 2), round(t[-1], 2)], must_move_bytes=nbytes,
                              ours_GBps=round(nbytes / o[2] / 1e3, 1),
                              note="median of 5 alternating rounds; torch: 10 launches")), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.reps)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--reps", str(args.reps), "--child"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0:
        lines.append(json.dumps(dict(error=f"exit status {p.returncode}")))
        print(lines[-1], flush=True)
    out = ROOT / "profiles" / "ref_actions_bench_mi355x.txt"
    out.write_text("# tools/ref_actions_bench.py: device microseconds per call, rai_ref_actions_store and the torch "
                   "composition in the same run\n" + "\n".join(lines) + "\n")
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
