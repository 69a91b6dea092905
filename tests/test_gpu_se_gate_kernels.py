"""rai_se_gate_fwd / _bwd and rai_bias_gelu_add_fwd (csrc/se_gate.hip) called raw through _lib against a
float64 numpy evaluation of the formulas (tests/se_gate_ref.py).

Tolerance, per checked array (pooled, hidden, s, dr, dw1, dw2; out): the same formula run in float32 by
torch on the CPU on the same inputs has some maximum error against float64; the kernel's may be at most
4 x that plus one float32 ulp of the array's largest magnitude (the rule of test_gpu_chan_norm_kernels.py:
the kernels' fixed summation orders differ from torch's; both are O(eps log n)).  The measured errors are
printed, and kept in profiles/double_cone_bench_mi355x.txt.

Shapes: C in {16 (M = 1), 64, 128, 512} x HW in {1, 16, 37, 256} x B in {1, 3}, and one B taken from the
kernel's constants, 2 * RAI_SEG_MAX_BLOCKS + 5: the backward's workgroups then own 3 samples each, write
more workspace slots than the second launch sums side by side (RAI_SEG_FIN_LANES), and the last one's run
is a single sample; that B runs at HW = 1 (and HW = 9 for C = 64), every case under 5,000 rows.
Inputs (seeded): unit normal r, every third sample with a common offset of 100; W1 / W2 pointers one float
into a larger buffer; dr pre-filled with a known pattern (the result must be pattern + dpool / HW: the add
is in place and touches each element once); outputs and workspace NaN-filled."""
import numpy as np
import pytest
import torch

import se_gate_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CS = [16, 64, 128, 512]
HWS = [1, 16, 37, 256]


def big_b():
    from rl_algo_impls_amd import _lib

    B = 2 * _lib.RAI_SEG_MAX_BLOCKS + 5
    run = -(-B // _lib.RAI_SEG_MAX_BLOCKS)
    slots = -(-B // run)
    assert run == 3 and slots > _lib.RAI_SEG_FIN_LANES and B - (slots - 1) * run < run  # ragged last run
    return B


def cases(C):
    out = [(B, HW) for HW in HWS for B in (1, 3)] + [(big_b(), 1)]
    if C == 64:
        out.append((big_b(), 9))
    assert all(B * HW < 5000 for B, HW in out)
    return out


@pytest.mark.parametrize("C", CS)
def test_gate_kernels_vs_float64(C):
    for B, HW in cases(C):
        inp = R.make_inputs(B, HW, C, seed=100000 * C + 100 * HW + B)
        r64, t32 = R.ref64(*inp), R.torch32(*inp)
        a, b = R.run_kernels(*inp, DEV, repeat_bwd=2)
        errs = R.errors(a, t32, r64)
        for k, (e_k, e_t, bound) in errs.items():
            print(f"se_gate C={C} HW={HW} B={B} {k}: kernel {e_k:.3e} torch_f32 {e_t:.3e} bound {bound:.3e}")
        for k, (e_k, e_t, bound) in errs.items():
            assert np.isfinite(a[k]).all(), (C, HW, B, k)
            assert e_k <= bound, (C, HW, B, k, e_k, e_t, bound)
        for k in ("dr", "dw1", "dw2"):  # two calls on the same inputs: the same bits
            assert np.array_equal(a[k], b[k]), (C, HW, B, k)


def test_shape_null_and_workspace_errors():
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(DEV)
    t = torch.zeros(1 << 16, device=DEV)
    p, q = t.data_ptr(), t.data_ptr() + 4
    big = 1 << 40
    for C, M, HW in ((24, 1, 4), (48, 3, 4), (2048, 128, 4), (8, 0, 4), (64, 8, 4), (64, 4, 0)):
        assert L.rai_se_gate_fwd(p, p, p, 2, C, HW, M, p, p, p, st) == _lib.RAI_E_SHAPE, (C, M, HW)
        assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, p, p, p, p, big, st) == _lib.RAI_E_SHAPE, (C, M, HW)
    assert L.rai_se_gate_fwd(p, p, p, -1, 64, 4, 4, p, p, p, st) == _lib.RAI_E_SHAPE
    C, M, HW = 64, 4, 4
    nb = int(L.rai_se_gate_workspace_bytes(C))
    assert nb == _lib.RAI_SEG_MAX_BLOCKS * 2 * M * C * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    w = ws.data_ptr()
    assert L.rai_se_gate_fwd(None, p, p, 2, C, HW, M, p, p, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_gate_fwd(p, p, None, 2, C, HW, M, p, p, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_gate_fwd(q, p, p, 2, C, HW, M, p, p, p, st) == _lib.RAI_E_WORKSPACE  # r 4-byte aligned
    assert L.rai_se_gate_fwd(p, q, q, 2, C, HW, M, p, q, p, st) == _lib.RAI_E_WORKSPACE  # pooled
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, None, p, p, w, nb, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, p, None, p, w, nb, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, p, p, p, None, nb, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, p, p, p, w, nb - 1, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, q, p, p, w, nb, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_se_gate_bwd(p, p, p, p, p, p, 2, C, HW, M, p, p, p, w + 4, nb, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_bias_gelu_add_fwd(p, p, p, 4, 6, p, st) == _lib.RAI_E_SHAPE
    assert L.rai_bias_gelu_add_fwd(p, p, None, 4, 8, p, st) == _lib.RAI_E_NULLPTR
    torch.cuda.synchronize()
    assert bool((t == 0).all())  # nothing was launched


def test_zero_batch():
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(DEV)
    C, M = 64, 4
    dw = torch.full((2, M * C), float("nan"), device=DEV)
    assert L.rai_se_gate_fwd(None, None, None, 0, C, 4, M, None, None, None, st) == 0
    assert L.rai_se_gate_bwd(None, None, None, None, None, None, 0, C, 4, M, None, dw[0].data_ptr(), dw[1].data_ptr(),
                             None, 0, st) == 0
    assert bool((dw == 0).all())


@pytest.mark.parametrize("rows,C", [(1, 4), (37, 32), (1029, 128), (300, 96)])
def test_bias_gelu_add(rows, C):
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(DEV)
    g = torch.Generator().manual_seed(rows * 1000 + C)
    x, skip, b = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g), torch.randn(C, generator=g)
    r64 = R.bias_gelu_add_ref64(x, b, skip)
    t32 = (skip + torch.nn.functional.gelu(x + b)).numpy()
    xd, sd = x.to(DEV), skip.to(DEV)
    bbuf, bp = R._offset(b, DEV)
    out = torch.full((rows, C), float("nan"), device=DEV)
    _lib.check(L.rai_bias_gelu_add_fwd(xd.data_ptr(), bp, sd.data_ptr(), rows, C, out.data_ptr(), st), "add")
    e_k = float(np.abs(out.cpu().numpy().astype(np.float64) - r64).max())
    e_t = float(np.abs(t32.astype(np.float64) - r64).max())
    bound = 4 * e_t + float(np.spacing(np.float32(np.abs(r64).max())))
    print(f"bias_gelu_add rows={rows} C={C}: kernel {e_k:.3e} torch_f32 {e_t:.3e} bound {bound:.3e}")
    assert e_k <= bound
    # a skip of zeros reproduces rai_bias_gelu_fwd bit for bit
    z, o0, o1 = torch.zeros_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    _lib.check(L.rai_bias_gelu_add_fwd(xd.data_ptr(), bp, z.data_ptr(), rows, C, o0.data_ptr(), st), "add")
    _lib.check(L.rai_bias_gelu_fwd(xd.data_ptr(), bp, rows, C, o1.data_ptr(), st), "fwd")
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32))
