"""rai_chan_ln_fwd / _bwd (csrc/chan_norm.hip) called raw through _lib against a float64 numpy
evaluation of the formula (tests/chan_norm_ref.py).

Tolerance, per checked array (out, mean, rstd, dx, dgamma, dbeta, dbias): the reference formula run in
float32 by torch on the CPU on the same inputs has some maximum error against float64; the kernel's may
be at most 4 x that plus one float32 ulp of the array's largest magnitude (the kernel's lane-tree and
cross-workgroup summation orders differ from torch's; both are O(eps log n)).  The measured errors per
shape are in profiles/chan_norm_bench_mi355x.txt.

Inputs (seeded): unit normal rows, every third with a common offset of 100 (an E[z^2] - mean^2 variance
fails there), one row constant after the bias (var = 0: rstd = eps^-1/2, y = beta), bias / gamma / beta
pointers one float into a larger buffer.  Row counts: 1; 37 (no multiple of the rows per wave); three full
row-pass workgroups plus a ragged tail; and, for C >= 64, 35 workgroups plus a tail (more partials than the
second launch has row lanes)."""
import numpy as np
import pytest
import torch

import chan_norm_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CS = [16, 32, 64, 128, 256]


def row_counts(C):
    from rl_algo_impls_amd import _lib

    per_wg = _lib.CLN_ROWS_PER_LANE * (_lib.CLN_THREADS // (C // 4))  # rows before another workgroup is added
    counts = [1, 37, 3 * per_wg + 5]
    if C >= 64:
        counts.append(35 * per_wg + 3)
    assert max(counts) < 5000
    return counts


@pytest.fixture(scope="module")
def refs():
    """(C, rows, gelu) -> (inputs, float64 reference, torch float32), computed once and left unchanged."""
    cache = {}

    def get(C, rows, gelu):
        k = (C, rows, gelu)
        if k not in cache:
            inp = R.make_inputs(rows, C, seed=1000 * C + rows)
            cache[k] = (inp, R.ref64(*inp, gelu), R.torch32(*inp, gelu))
        return cache[k]

    return get


@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("C", CS)
def test_kernels_vs_float64(refs, C, gelu):
    for rows in row_counts(C):
        inp, r64, t32 = refs(C, rows, gelu)
        a, b = R.run_kernels(*inp, gelu, DEV, repeat_bwd=2)
        errs = R.errors(a, t32, r64)
        for k, (e_k, e_t, bound) in errs.items():
            print(f"chan_ln C={C} rows={rows} gelu={gelu} {k}: kernel {e_k:.3e} torch_f32 {e_t:.3e} bound {bound:.3e}")
        for k, (e_k, e_t, bound) in errs.items():
            assert np.isfinite(a[k]).all(), (C, rows, k)
            assert e_k <= bound, (C, rows, gelu, k, e_k, e_t, bound)
        for k in ("dx", "dgamma", "dbeta", "dbias"):  # two launches, the same bits
            assert np.array_equal(a[k], b[k]), (C, rows, k)
        if rows > 2:  # the constant row: var = 0 exactly
            r = rows // 2
            assert a["mean"][r] == 3.0
            np.testing.assert_allclose(a["rstd"][r], 1 / np.sqrt(np.float64(np.float32(R.EPS))), rtol=2e-7)
            if not gelu:
                np.testing.assert_array_equal(a["out"][r], inp[3].numpy())


def test_shape_and_alignment_errors():
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(DEV)
    for C in (12, 48, 512):
        t = torch.zeros(8 * C + 8, device=DEV)
        p = t.data_ptr()
        assert L.rai_chan_ln_fwd(p, p, p, p, 8, C, R.EPS, 1, p, p, st) == _lib.RAI_E_SHAPE
        assert L.rai_chan_ln_bwd(p, p, p, p, p, p, 8, C, 1, p, p, p, p, p, 1 << 30, st) == _lib.RAI_E_SHAPE
    assert _lib.RAI_CLN_MAX_C == 256
    C = 32
    t = torch.zeros(8 * C + 8, device=DEV)
    ws = torch.empty(int(L.rai_chan_ln_workspace_bytes(C)), dtype=torch.uint8, device=DEV)
    p, q = t.data_ptr(), t.data_ptr() + 4
    assert L.rai_chan_ln_fwd(q, p, p, p, 8, C, R.EPS, 0, p, p, st) == _lib.RAI_E_WORKSPACE  # x 4-byte aligned
    assert L.rai_chan_ln_fwd(p, p, p, p, 8, C, R.EPS, 0, q, p, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_chan_ln_bwd(p, p, p, p, p, p, 8, C, 0, q, p, p, p, ws.data_ptr(), ws.numel(), st) \
        == _lib.RAI_E_WORKSPACE
    assert L.rai_chan_ln_bwd(p, p, p, p, p, p, 8, C, 0, p, p, p, p, ws.data_ptr(), ws.numel() - 1, st) \
        == _lib.RAI_E_WORKSPACE
    assert L.rai_chan_ln_fwd(None, p, p, p, 8, C, R.EPS, 0, p, p, st) == _lib.RAI_E_NULLPTR
    torch.cuda.synchronize()


def test_zero_rows():
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(DEV)
    C = 64
    dpar = torch.full((3, C), float("nan"), device=DEV)
    assert L.rai_chan_ln_fwd(None, None, None, None, 0, C, R.EPS, 1, None, None, st) == 0
    assert L.rai_chan_ln_bwd(None, None, None, None, None, None, 0, C, 1, None, dpar[0].data_ptr(), dpar[1].data_ptr(),
                             dpar[2].data_ptr(), None, 0, st) == 0
    assert bool((dpar == 0).all())
