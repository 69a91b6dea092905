"""Same-box timing of the DQN kernels (csrc/dqn.hip) against the torch ops they replace, and of the whole
replayed gradient step against the same step run eagerly with torch sampling, at the CartPole shape (batch 64,
4 floats, hidden [256, 256], capacity 1e5) and the Atari shape (batch 32, 4x84x84 uint8, IMPALA encoder,
capacity 1e5).

Every shape runs in a child process of its own under its own time limit (the parent never touches the GPU),
with at most 16 CPU threads.  One JSON line per kernel: device microseconds per call of ours and of torch, in
the same run.  The lines are also written to profiles/dqn_bench_mi355x.txt.

    python tools/dqn_bench.py [--reps 50] [--timeout 300]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SHAPES = {
    "cartpole": dict(B=64, obs=(4,), u8=False, A=2, N=1, policy=dict(hidden_sizes=[256, 256])),
    "atari": dict(B=32, obs=(4, 84, 84), u8=True, A=6, N=8, policy=dict(cnn_style="impala", cnn_flatten_dim=256)),
}
CAPACITY = 100_000


def child(shape, reps):
    import ctypes as C

    import numpy as np
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd import _lib
    from rl_algo_impls_amd.dqn import DQN, DQNPolicy, argmax_rows, head_bwd, head_fwd, polyak_update, td_loss
    from rl_algo_impls_amd.envs import Box, Discrete
    from rl_algo_impls_amd.replay import Batch, ReplayRing
    from rl_algo_impls_amd.rollout import gather_rows

    s = SHAPES[shape]
    B, A, N = s["B"], s["A"], s["N"]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    rng = np.random.default_rng(1)

    def timeit(fn, n=reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def emit(kernel, ours, ref, note=""):
        print(json.dumps(dict(shape=shape, kernel=kernel, B=B, ours_us=round(ours, 1), torch_us=round(ref, 1),
                              note=note)), flush=True)

    # -- ring: filled to capacity so that the sampler's domain is the full 1e5 ------------------------------
    dtype = np.uint8 if s["u8"] else np.float32
    ring = ReplayRing(CAPACITY, s["obs"], dtype, dev, seed=3)
    chunk = 1000
    mk = lambda n: (rng.integers(0, 256, size=(n,) + s["obs"], dtype=np.uint8) if s["u8"]
                    else rng.standard_normal((n,) + s["obs"]).astype(np.float32))
    o, no = mk(chunk), mk(chunk)
    for i in range(CAPACITY // chunk):
        ring.push(o, no, rng.integers(0, A, chunk), rng.standard_normal(chunk).astype(np.float32),
                  rng.random(chunk) < 0.1)
    torch.cuda.synchronize()
    L, st = _lib.lib(), _lib.stream_handle(dev)

    # push of one env step's N transitions (device staging -> ring) vs torch index_copy_ of the five fields
    stage = ring._stage(N)[2]
    slots = torch.arange(N, device=dev)
    fields = (ring.obs, ring.next_obs, ring.actions, ring.rewards, ring.dones)

    def push_ours():
        _lib.check(L.rai_replay_push(C.byref(ring.c_ring), *[d.data_ptr() for d in stage], N, st), "push")

    def push_torch():
        for f, d in zip(fields, stage):
            f.index_copy_(0, slots, d)

    emit("replay_push", timeit(push_ours), timeit(push_torch), f"N={N} transitions per call")

    # sample + gather: one launch; indices + rai_gather_rows; torch randperm + index_select
    bufs = ring.batch_buffers(B)

    def sample_two_launch():
        _lib.check(L.rai_replay_sample(C.byref(ring.c_ring), ring.seed, B, None, bufs[5].data_ptr(), None, None, None,
                                       None, None, st), "sample")
        gather_rows(list(fields), list(bufs[:5]), bufs[5])

    def sample_torch():
        idx = torch.randperm(CAPACITY, device=dev)[:B]
        return [f.index_select(0, idx) for f in fields]

    t_torch = timeit(sample_torch)
    emit("replay_sample (draw + gather, one launch)", timeit(lambda: ring.launch_sample(B)), t_torch,
         "torch: randperm(len)[:B] + 5 index_select")
    emit("replay_sample (draw) + rai_gather_rows", timeit(sample_two_launch), t_torch, "two launches")

    # TD loss, argmax
    q, qn = torch.randn(B, A, generator=g).to(dev), torch.randn(B, A, generator=g).to(dev)
    a = torch.randint(0, A, (B,), generator=g).to(dev)
    r = torch.randn(B, generator=g).to(dev)
    d = (torch.rand(B, generator=g) < 0.2).to(dev)

    def td_torch():
        qq = q.clone().requires_grad_(True)
        t = r + ~d * 0.99 * qn.max(1).values
        loss = torch.nn.functional.smooth_l1_loss(qq.gather(1, a.unsqueeze(1)).squeeze(1), t)
        loss.backward()
        return qq.grad

    emit("dqn_td_loss", timeit(lambda: td_loss(q, qn, a, r, d, 0.99)), timeit(td_torch),
         "torch: target, gather, smooth_l1_loss, backward to q")
    emit("argmax_rows", timeit(lambda: argmax_rows(q)), timeit(lambda: q.argmax(1)))

    # the trainer: fused head, polyak, whole step
    class Env:
        num_envs = 1
        single_observation_space = Box(0, 255, s["obs"], np.uint8) if s["u8"] else Box(-np.inf, np.inf, s["obs"],
                                                                                     np.float32)
        single_action_space = Discrete(A)

    env = Env()
    env.unwrapped = env
    torch.manual_seed(0)
    policy = DQNPolicy(env, **s["policy"]).to(dev)
    algo = DQN(policy, dev, None, batch_size=B)
    head, t_head = policy.q_net.head, algo.target_q_net.head
    H = head.in_features
    h, hn = torch.randn(B, H, generator=g).to(dev).relu(), torch.randn(B, H, generator=g).to(dev).relu()

    def head_ours():
        _, _, gb = head_fwd(h, hn, head.weight, head.bias, t_head.weight, t_head.bias, a, r, d, 0.99)
        head_bwd(h, head.weight, a, gb, head.weight.grad, head.bias.grad)

    def head_unfused():
        hh = h.clone().requires_grad_(True)
        with torch.no_grad():
            qn_ = t_head(hn)
        q_ = head(hh)
        _, _, dq = td_loss(q_.detach(), qn_, a, r, d, 0.99)
        q_.backward(dq)

    emit(f"dqn_head_fwd + _bwd (H={H}, A={A})", timeit(head_ours), timeit(head_unfused),
         "torch column: linear x2 + rai_dqn_td_loss + autograd (the unfused path)")
    algo.flat.grad.zero_()

    def polyak_torch():
        for tp, p in zip(algo.target_q_net.parameters(), policy.q_net.parameters()):
            tp.data.copy_(0.25 * p.data + (1 - 0.25) * tp.data)

    emit(f"polyak_update (P={algo.flat.P})", timeit(lambda: polyak_update(algo.target_flat.flat, algo.flat.flat, 0.25)),
         timeit(polyak_torch), "torch: the reference's per-parameter loop")

    def step_eager():
        idx = torch.randperm(CAPACITY, device=dev)[:B]
        o_, no_, a_, r_, d_ = [f.index_select(0, idx) for f in fields]
        algo.train(Batch(o_, a_, r_, d_.view(torch.bool), no_))

    n = max(10, reps // 2)
    t_eager = timeit(step_eager, n)
    algo.train_sampled(ring, algo.WARMUP + 1)  # warm-up + capture
    t_graph = timeit(lambda: algo.train_sampled(ring, 1), n)
    emit("gradient step (replayed hipGraph)", t_graph, t_eager,
         "torch column: the same step un-captured with torch.randperm + index_select sampling")
    assert ring.device_state()["err"] == 0 and bool(torch.isfinite(algo.flat.flat).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", metavar="SHAPE")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k, "16"))))
    lines = []
    rc = 0
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--reps", str(args.reps),
               "--child", shape]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        rc = p.returncode
        if rc != 0:  # a failed or timed-out step ends the run: nothing more is started on the GPU
            lines.append(json.dumps(dict(shape=shape, error=f"exit status {rc}")))
            print(lines[-1], flush=True)
            break
    out = ROOT / "profiles" / "dqn_bench_mi355x.txt"
    out.write_text("# tools/dqn_bench.py: device microseconds per call, ours and torch in the same run\n"
                   + "\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
