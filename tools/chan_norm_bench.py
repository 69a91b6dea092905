"""Same-box timing and accuracy of the channel layer norm kernels (csrc/chan_norm.hip) against the torch
composition they replace.

  kernels  rai_chan_ln_fwd / _bwd against bias add + the reference module's formula + GELU and autograd's
           backward, on NHWC (channels_last) activations at the C5 shapes with `normalization: layer`:
           B = 512, C = 128, H = W = 16, 4, 1 (rows = 512 * 256, 512 * 16, 512 * 1).  Each kernel's achieved
           bytes/s against the traffic it must move (forward: read + write rows * C * 4; backward: three reads
           and one write).
  network  one forward + backward of the full-width C5 network with normalization="layer" at its per-GPU
           minibatch (B = 768), the fused path against the modules' torch path on the same NHWC activations.
  errors   the kernels' and torch's float32 maximum errors against float64 (tests/chan_norm_ref.py) per
           shape of tests/test_gpu_chan_norm_kernels.py.

Every section runs in a child process of its own under its own time limit (the parent never touches the
GPU), with at most 16 CPU threads.  One JSON line per measurement, device microseconds from events around
`reps` calls after warm-up; ours and torch in the same run.  The lines are also written to
profiles/chan_norm_bench_mi355x.txt.

    python tools/chan_norm_bench.py [--reps 50] [--timeout 600] [--sections kernels,network,errors]
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
SECTIONS = ("kernels", "errors", "network")
NVEC = [6, 4, 4, 4, 4, 7, 49]
C5_KW = dict(strides_per_level=[[2, 2], [2, 2]], deconv_strides_per_level=[[2, 2], [2, 2]],
             encoder_residual_blocks_per_level=[3, 2, 4], decoder_residual_blocks_per_level=[2, 3],
             increment_kernel_size_on_down_conv=True, additional_critic_activation_functions=["tanh", "identity"],
             subaction_mask={0: {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 5}}, init_layers_orthogonal=True)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def child(section, reps):
    import numpy as np
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd import _lib, backbone, running_utils

    dev = torch.device("cuda:0")

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

    if section == "kernels":
        L, st = _lib.lib(), _lib.stream_handle(dev)
        B, C = 512, 128
        g = torch.Generator().manual_seed(1)
        for hw in (16, 4, 1):
            rows = B * hw * hw
            mk = lambda: torch.randn(B, C, hw, hw, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            x, dout = mk(), mk()
            norm = backbone.ChannelLayerNorm2d(C).to(dev)
            bias = torch.randn(C, generator=g).to(dev).requires_grad_()
            with torch.no_grad():
                norm.gamma.copy_(1 + 0.5 * torch.randn(1, C, 1, 1, generator=g))
                norm.beta.copy_(0.5 * torch.randn(1, C, 1, 1, generator=g))
            for gelu in (1, 0):
                out, dx = torch.empty_like(x), torch.empty_like(x)
                stats = torch.empty(rows, 2, device=dev)
                dpar = torch.empty(3, C, device=dev)
                nb = int(L.rai_chan_ln_workspace_bytes(C))
                ws = torch.empty(nb, dtype=torch.uint8, device=dev)
                ptr = lambda t: t.data_ptr()

                def fwd():
                    _lib.check(L.rai_chan_ln_fwd(ptr(x), ptr(bias), ptr(norm.gamma), ptr(norm.beta), rows, C, 1e-5,
                                                 gelu, ptr(out), ptr(stats), st), "fwd")

                def bwd():
                    _lib.check(L.rai_chan_ln_bwd(ptr(dout), ptr(x), ptr(bias), ptr(norm.gamma), ptr(norm.beta),
                                                 ptr(stats), rows, C, gelu, ptr(dx), ptr(dpar[0]), ptr(dpar[1]),
                                                 ptr(dpar[2]), ptr(ws), nb, st), "bwd")

                xr = x.detach().clone().requires_grad_()

                def t_fwd():
                    y = norm(xr + bias.view(1, -1, 1, 1))
                    return torch.nn.functional.gelu(y) if gelu else y

                y_saved = t_fwd()

                def t_bwd():
                    torch.autograd.grad(y_saved, (xr, bias, norm.gamma, norm.beta), dout, retain_graph=True)

                with torch.no_grad():
                    t_f = timeit(t_fwd)
                o_f, o_b, t_b = timeit(fwd), timeit(bwd), timeit(t_bwd)
                act = rows * C * 4
                emit(section=section, kernel="rai_chan_ln_fwd", rows=rows, C=C, gelu=gelu, ours_us=round(o_f, 1),
                     torch_us=round(t_f, 1), must_move_bytes=2 * act, ours_GBps=round(2 * act / o_f / 1e3, 1),
                     note="torch: bias add, mean, var, 5 elementwise passes" + (", GELU" if gelu else ""))
                emit(section=section, kernel="rai_chan_ln_bwd (2 launches)", rows=rows, C=C, gelu=gelu,
                     ours_us=round(o_b, 1), torch_us=round(t_b, 1), must_move_bytes=4 * act,
                     ours_GBps=round(4 * act / o_b / 1e3, 1), note="torch: autograd's backward of the composition")
        return

    if section == "errors":
        import chan_norm_ref as R

        per = lambda C: _lib.CLN_ROWS_PER_LANE * (_lib.CLN_THREADS // (C // 4))
        for C in (16, 32, 64, 128, 256):
            for rows in [1, 37, 3 * per(C) + 5] + ([35 * per(C) + 3] if C >= 64 else []):
                for gelu in (0, 1):
                    inp = R.make_inputs(rows, C, seed=1000 * C + rows)
                    got = R.run_kernels(*inp, gelu, dev)[0]
                    e = R.errors(got, R.torch32(*inp, gelu), R.ref64(*inp, gelu))
                    emit(section=section, C=C, rows=rows, gelu=gelu,
                         **{k: dict(kernel=float(f"{v[0]:.3e}"), torch_f32=float(f"{v[1]:.3e}"),
                                    bound=float(f"{v[2]:.3e}")) for k, v in e.items()})
        return

    # network: the full-width C5 network with normalization="layer", forward + backward
    running_utils.seed_miopen_find_db(tempfile.mkdtemp(prefix="rai-miopen-bench-"))
    from rl_algo_impls_amd.envs import Box, MultiDiscrete

    B = 768
    torch.manual_seed(1)
    net = backbone.SqueezeUnetActorCriticNetwork(
        Box(0.0, 1.0, (74, 16, 16), np.float32), MultiDiscrete(np.tile(NVEC, 256)), MultiDiscrete(NVEC),
        channels_per_level=[128] * 3, normalization="layer", **C5_KW).to(dev)
    rng = np.random.default_rng(1)
    obs = torch.from_numpy((rng.random((B, 74, 16, 16)) < 0.2).astype(np.float32)).to(dev)

    def step():
        net.zero_grad(set_to_none=True)
        logits, v = net.logits_and_value(obs)
        (logits.square().mean() + v.square().mean()).backward()

    n = max(3, reps // 10)
    fused = timeit(step, n)
    real = backbone._chan_ln_fusable
    backbone._chan_ln_fusable = lambda C: False  # the modules' torch path on the same NHWC activations
    try:
        plain = timeit(step, n)
    finally:
        backbone._chan_ln_fusable = real
    emit(section=section, what="C5 network (normalization=layer) forward + backward", B=B,
         norms_per_forward=sum(isinstance(m, backbone.ChannelLayerNorm2d) for m in net.modules()),
         fused_us=round(fused, 1), torch_path_us=round(plain, 1), speedup=round(plain / fused, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--sections", default=",".join(SECTIONS))
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
    out = ROOT / "profiles" / "chan_norm_bench_mi355x.txt"
    out.write_text("# tools/chan_norm_bench.py: device microseconds per call, ours and torch in the same run; "
                   "errors: max |x - float64|\n" + "\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
