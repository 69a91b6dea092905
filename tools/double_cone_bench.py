"""Same-box timing of the DoubleCone network's new kernels (csrc/se_gate.hip) against the torch
compositions they replace.

  gate     rai_se_gate_fwd / _bwd at (B, HW, C) in {(768, 16, 128), (768, 256, 128), (768, 16, 512)} (the
           default network's cone at pooled_channels 128 and 512 on a 16x16 map, and its full-resolution
           blocks) against AdaptiveAvgPool2d + Linear + GELU + Linear + sigmoid on the same NHWC activation
           and autograd's backward of it.  The fused backward also does the add into dr that autograd does in
           a launch of its own (counted on torch's side as part of its backward).
  add      rai_bias_gelu_add_fwd against rai_bias_gelu_fwd followed by torch's add, at the cone's last
           up-convolution (768 * 256 rows, C = 128).
  network  one forward + backward of the full DoubleCone network at B = 768 on a 16x16 map, the fused gate on
           and off, with the YAML's pooled_channels 128 and the default 512.

Every section runs in a child process of its own under its own time limit (the parent never touches the
GPU), with at most 16 CPU threads.  One JSON line per measurement, device microseconds from events around
`reps` calls after warm-up; ours and torch in the same run.  The lines are also written to --out
(default profiles/double_cone_bench_mi355x.txt).

    python tools/double_cone_bench.py [--reps 50] [--timeout 600] [--sections gate,add,network] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SECTIONS = ("gate", "add", "network")
NVEC = [6, 4, 4, 4, 4, 7, 49]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def child(section, reps):
    import numpy as np
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd import _lib, backbone, running_utils

    dev = torch.device("cuda:0")
    ptr = lambda t: t.data_ptr()

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

    if section == "gate":
        L, st = _lib.lib(), _lib.stream_handle(dev)
        for B, HW, C in ((768, 16, 128), (768, 256, 128), (768, 16, 512)):
            side, M = int(HW ** 0.5), C // 16
            torch.manual_seed(C + HW)
            se = backbone.SqueezeExcitation(C).to(dev)
            w1, w2 = se.fc[0].weight.detach(), se.fc[2].weight.detach()
            r = torch.randn(B, C, side, side, device=dev).contiguous(memory_format=torch.channels_last)
            ds = torch.randn(B, C, device=dev)
            s, pooled, hidden = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev), torch.empty(B, M, device=dev)
            dr = torch.randn_like(r)
            dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
            nb = int(L.rai_se_gate_workspace_bytes(C))
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)

            def fwd():
                _lib.check(L.rai_se_gate_fwd(ptr(r), ptr(w1), ptr(w2), B, C, HW, M, ptr(s), ptr(pooled), ptr(hidden),
                                             st), "fwd")

            def bwd():
                _lib.check(L.rai_se_gate_bwd(ptr(ds), ptr(s), ptr(pooled), ptr(hidden), ptr(w1), ptr(w2), B, C, HW, M,
                                             ptr(dr), ptr(dw1), ptr(dw2), ptr(ws), nb, st), "bwd")

            rr = r.detach().clone().requires_grad_()
            t_fwd = lambda: se.fc(se.avg_pool(rr).view(B, C))
            s_saved = t_fwd()
            dr0 = torch.randn_like(r)

            def t_bwd():  # autograd's backward of the gate, and the add of its dr into the epilogue's
                g = torch.autograd.grad(s_saved, (rr, se.fc[0].weight, se.fc[2].weight), ds, retain_graph=True)
                return dr0 + g[0]

            with torch.no_grad():
                t_f = timeit(t_fwd)
            o_f, o_b, t_b = timeit(fwd), timeit(bwd), timeit(t_bwd)
            np.testing.assert_allclose(s.cpu().numpy(), s_saved.detach().cpu().numpy(), rtol=1e-4, atol=1e-6)
            emit(section=section, kernel="rai_se_gate_fwd (1 launch)", B=B, HW=HW, C=C, ours_us=round(o_f, 1),
                 torch_us=round(t_f, 1), speedup=round(t_f / o_f, 2), note="torch: avg_pool, Linear, GELU, Linear, sigmoid")
            emit(section=section, kernel="rai_se_gate_bwd (2 launches)", B=B, HW=HW, C=C, ours_us=round(o_b, 1),
                 torch_us=round(t_b, 1), speedup=round(t_b / o_b, 2), workspace_bytes=nb,
                 note="torch: autograd's backward of the composition + the add into dr")
        return

    if section == "add":
        L, st = _lib.lib(), _lib.stream_handle(dev)
        rows, C = 768 * 256, 128
        x, skip = torch.randn(rows, C, device=dev), torch.randn(rows, C, device=dev)
        b = torch.randn(C, device=dev)
        out, tmp = torch.empty_like(x), torch.empty_like(x)

        def fused():
            _lib.check(L.rai_bias_gelu_add_fwd(ptr(x), ptr(b), ptr(skip), rows, C, ptr(out), st), "add")

        def two():
            _lib.check(L.rai_bias_gelu_fwd(ptr(x), ptr(b), rows, C, ptr(tmp), st), "fwd")
            return skip + tmp

        o, t = timeit(fused), timeit(two)
        act = rows * C * 4
        emit(section=section, kernel="rai_bias_gelu_add_fwd", rows=rows, C=C, ours_us=round(o, 1),
             bias_gelu_then_add_us=round(t, 1), speedup=round(t / o, 2), must_move_bytes=3 * act,
             ours_GBps=round(3 * act / o / 1e3, 1))
        return

    # network: the full DoubleCone network, forward + backward, the fused gate on and off
    running_utils.seed_miopen_find_db(tempfile.mkdtemp(prefix="rai-miopen-bench-"))
    from rl_algo_impls_amd.envs import Box, MultiDiscrete

    B = 768
    rng = np.random.default_rng(1)
    obs = torch.from_numpy((rng.random((B, 74, 16, 16)) < 0.2).astype(np.float32)).to(dev)
    for pooled_channels in (128, 512):
        torch.manual_seed(1)
        net = backbone.DoubleConeActorCritic(
            Box(0.0, 1.0, (74, 16, 16), np.float32), MultiDiscrete(np.tile(NVEC, 256)), MultiDiscrete(NVEC),
            pooled_channels=pooled_channels, additional_critic_activation_functions=["tanh", "identity"]).to(dev)

        def step():
            net.zero_grad(set_to_none=True)
            logits, v = net.logits_and_value(obs)
            (logits.square().mean() + v.square().mean()).backward()

        n = max(3, reps // 10)
        t = {}
        for on in (True, False):
            backbone.set_fused_gate(net, on)
            t[on] = timeit(step, n)
        emit(section=section, what="DoubleCone network forward + backward", B=B, pooled_channels=pooled_channels,
             se_blocks=sum(isinstance(m, backbone.SEResidualBlock) for m in net.modules()),
             fused_gate_us=round(t[True], 1), torch_gate_us=round(t[False], 1), speedup=round(t[False] / t[True], 3))
        del net
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "double_cone_bench_mi355x.txt"))
    ap.add_argument("--child", metavar="SECTION")
    args = ap.parse_args()
    if args.child:
        child(args.child, args.reps)
        return 0
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k, "16"))))
    lines, rc = [], 0
    for section in args.sections.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--reps", str(args.reps),
               "--child", section]
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        lines += [l for l in p.stdout.splitlines() if l.startswith("{")]
        rc = p.returncode
        if rc != 0:  # a failed or timed-out step ends the run: nothing more is started on the GPU
            lines.append(json.dumps(dict(section=section, error=f"exit status {rc}")))
            print(lines[-1], flush=True)
            break
    Path(args.out).write_text("# tools/double_cone_bench.py: device microseconds per call, ours and torch in the "
                              "same run\n" + "\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
