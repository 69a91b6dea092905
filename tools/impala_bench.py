"""Same-box timing of the IMPALA CNN kernels (csrc/conv3x3.hip) against the torch ops they replace
(F.conv2d / aten.convolution_backward on MIOpen, F.max_pool2d), layer by layer at the procgen shape
(3x64x64, channels 16/32/32, update minibatch 2,048) and the Atari shape (4x84x84, minibatch 256).

Every layer runs in a child process of its own under its own time limit (the parent never touches the
GPU), with at most 16 CPU threads.  Prints one JSON line per kernel: device microseconds of ours and of
torch, the FLOPs and the fraction of the 157.3 TF/s f32 MFMA peak.

    python tools/impala_bench.py [--reps 20] [--timeout 180]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PEAK = 157.3e12
SHAPES = {"procgen": (2048, 3, 64, 64), "atari": (256, 4, 84, 84)}
CHANNELS = (16, 32, 32)


def layers(shape):
    """(name, kind, Ci, Co, H, W) for one block of every distinct layer shape."""
    _, C, H, W = SHAPES[shape]
    out = []
    ci = C
    for s, co in enumerate(CHANNELS):
        out.append((f"seq{s}.conv", "first" if s == 0 else "conv", ci, co, H, W))
        out.append((f"seq{s}.pool", "pool", co, co, H, W))
        H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out.append((f"seq{s}.block_conv", "conv", co, co, H, W))
        ci = co
    return out


def child(shape, name, reps):
    import torch
    import torch.nn.functional as F

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd import _lib, impala_ops as io

    B = SHAPES[shape][0]
    _, kind, Ci, Co, H, W = next(l for l in layers(shape) if l[0] == name)
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = True
    g = torch.Generator().manual_seed(1)
    cl = torch.channels_last

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    def emit(kernel, ours, ref, flops, nbytes):
        print(json.dumps(dict(shape=shape, layer=name, kernel=kernel, B=B, Ci=Ci, Co=Co, H=H, W=W,
                              ours_us=round(ours, 1), torch_us=round(ref, 1), flops=flops, bytes=nbytes,
                              peak_fraction=round(flops / (ours * 1e-6) / PEAK, 4) if flops else None)), flush=True)

    M = B * H * W
    if kind == "pool":
        x = torch.randn(B, Co, H, W, generator=g).to(dev).contiguous(memory_format=cl)
        y, am = io._pool_fwd(x)
        dy = torch.randn(y.shape, generator=g).to(dev).contiguous(memory_format=cl)
        _, idx = F.max_pool2d(x, 3, 2, 1, return_indices=True)
        nb = 4 * (x.numel() + y.numel())
        emit("maxpool_fwd", timeit(lambda: io._pool_fwd(x)), timeit(lambda: F.max_pool2d(x, 3, 2, 1)), 0,
             nb + y.numel())
        emit("maxpool_bwd", timeit(lambda: io._pool_bwd(dy, am, H, W)),
             timeit(lambda: torch.ops.aten.max_pool2d_with_indices_backward(dy, x, [3, 3], [2, 2], [1, 1], [1, 1],
                                                                            False, idx)), 0, nb + y.numel())
        return
    flops = 2 * M * 9 * Ci * Co
    w = (torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5).to(dev).contiguous(memory_format=cl)
    b = (torch.randn(Co, generator=g) * 0.1).to(dev)
    dz = torch.randn(B, Co, H, W, generator=g).to(dev).contiguous(memory_format=cl)
    wbytes = 4 * w.numel()
    if kind == "first":
        xu = torch.randint(0, 256, (B, Ci, H, W), generator=g, dtype=torch.uint8).to(dev).contiguous(memory_format=cl)
        xf = (xu.float() / 255.0).contiguous(memory_format=cl)
        emit("conv3x3_fwd_first(u8)", timeit(lambda: io._conv_fwd(xu, w, b, x_div=255.0)),
             timeit(lambda: F.conv2d(xf, w, b, padding=1)), flops, xu.numel() + 4 * dz.numel() + wbytes)
        key = torch.nn.Identity()
        emit("conv3x3_wgrad_first(u8)", timeit(lambda: io._conv_wgrad(key, xu, dz, w, b, False, False, 255.0)),
             timeit(lambda: torch.ops.aten.convolution_backward(dz, xf, w, [Co], [1, 1], [1, 1], [1, 1], False,
                                                                [0, 0], 1, [False, True, True])), flops,
             xu.numel() + 4 * dz.numel() + wbytes)
        return
    x = torch.randn(B, Ci, H, W, generator=g).to(dev).contiguous(memory_format=cl)
    res = torch.randn(B, Co, H, W, generator=g).to(dev).contiguous(memory_format=cl)
    act = 4 * (x.numel() + dz.numel())
    emit("conv3x3_fwd(pre,res)", timeit(lambda: io._conv_fwd(x, w, b, res=res, pre=True)),
         timeit(lambda: res + F.conv2d(F.relu(x), w, b, padding=1)), flops, act + 4 * res.numel() + wbytes)
    emit("conv3x3_dgrad(mask,res)", timeit(lambda: io._conv_dgrad(dz, w, m=x, res=x)),
         timeit(lambda: x + torch.ops.aten.threshold_backward(
             torch.ops.aten.convolution_backward(dz, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                 [True, False, False])[0], x, 0)), flops, act + 8 * x.numel() + wbytes)
    key = torch.nn.Identity()
    emit("conv3x3_wgrad(pre)", timeit(lambda: io._conv_wgrad(key, x, dz, w, b, True, False)),
         timeit(lambda: torch.ops.aten.convolution_backward(dz, F.relu(x), w, [Co], [1, 1], [1, 1], [1, 1], False,
                                                            [0, 0], 1, [False, True, True])), flops, act + wbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "LAYER"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k, "16"))))
    for shape in SHAPES:
        for name, *_ in layers(shape):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--reps", str(args.reps),
                   "--child", shape, name]
            rc = subprocess.run(cmd, env=env).returncode
            if rc != 0:  # a failed or timed-out step ends the run: nothing more is started on the GPU
                print(json.dumps(dict(shape=shape, layer=name, error=f"exit status {rc}")), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
