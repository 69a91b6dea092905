"""rai_ref_actions_store (csrc/ref_actions.hip) called raw through _lib, in exact integer equality with the
oracle of tests/ref_actions_ref.py: both source dtypes, mask and no mask, GridNet / Discrete / MultiDiscrete
shapes on both sides of the 64-row tile and the 256-env workgroup, the injected out-of-range and masked-out
values, dst as a slot inside a sentinel-filled buffer, bad between guard elements, an odd mask address, bit
repeatability, and the error codes (nothing launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_actions_ref as R

pytestmark = pytest.mark.gpu

SENT64 = -0x5A5A5A5A5A5A5A5B
SENT32 = -0x5A5A5A5B


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def nvec_arr(nvec):
    return (C.c_int32 * len(nvec))(*[int(n) for n in nvec])


def call(src, code, nvec, G, mask, N, cells, dst, bad):
    from rl_algo_impls_amd import _lib

    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return _lib.lib().rai_ref_actions_store(p(src), code, nvec, G, p(mask), N, cells, p(dst), p(bad),
                                            _lib.stream_handle(torch.device("cuda", 0)))


def run_case(dev, nvec, cells, N, dtype, with_mask, seed, mask_shift=0):
    from rl_algo_impls_amd import _lib

    src, mask = R.make_case(nvec, cells, N, dtype, with_mask, seed)
    G, Rows = len(nvec), N * cells
    want_dst, want_bad = R.oracle(src, nvec, mask, cells)
    src_d = torch.from_numpy(src).to(dev)
    pad = 3 * G + 1  # the slot starts at a non-zero, 8-byte aligned offset of a larger buffer
    buf = torch.full((pad + Rows * G + pad,), SENT64, dtype=torch.int64, device=dev)
    dst = buf[pad:pad + Rows * G]
    badbuf = torch.full((N + 2,), SENT32, dtype=torch.int32, device=dev)
    bad = badbuf[1:N + 1]
    mptr = None
    if mask is not None:
        mbuf = torch.zeros(Rows * sum(nvec) + 64, dtype=torch.uint8, device=dev)
        mview = mbuf[mask_shift:mask_shift + mask.size]
        mview.copy_(torch.from_numpy(mask.reshape(-1).view(np.uint8)).to(dev))
        mptr = mview.data_ptr()
        assert mptr % 16 == mask_shift % 16
    code = _lib.RAI_REF_ACT_I32 if np.dtype(dtype) == np.int32 else _lib.RAI_REF_ACT_I64
    assert call(src_d, code, nvec_arr(nvec), G, mptr, N, cells, dst, bad) == 0
    got, got_bad = buf.cpu().numpy(), badbuf.cpu().numpy()
    np.testing.assert_array_equal(got[pad:pad + Rows * G].reshape(Rows, G), want_dst)
    np.testing.assert_array_equal(got_bad[1:N + 1], want_bad)
    assert (got[:pad] == SENT64).all() and (got[pad + Rows * G:] == SENT64).all(), "wrote outside the slot"
    assert got_bad[0] == SENT32 and got_bad[-1] == SENT32, "wrote outside bad"
    assert want_bad[0] == 0, "env 0 has nothing wrong"
    if N > 1:
        assert want_bad[-1] == cells * G, "every component of the last env is wrong"
    # two calls give the same bits
    buf2 = torch.full_like(buf, SENT64)
    bad2 = torch.full_like(badbuf, SENT32)
    assert call(src_d, code, nvec_arr(nvec), G, mptr, N, cells, buf2[pad:pad + Rows * G], bad2[1:N + 1]) == 0
    assert torch.equal(buf, buf2) and torch.equal(badbuf, bad2)


@pytest.mark.parametrize("name,nvec,cells,N,dtype,with_mask,seed", R.cases(), ids=[c[0] for c in R.cases()])
def test_matches_oracle(dev, name, nvec, cells, N, dtype, with_mask, seed):
    run_case(dev, nvec, cells, N, dtype, with_mask, seed)


@pytest.mark.parametrize("shift", [1, 7, 15])
@pytest.mark.parametrize("nvec,cells,N", [(R.GRID_NVEC, 37, 3), ((6,), 1, 67)])
def test_mask_at_an_odd_address(dev, nvec, cells, N, shift):
    """The mask pointer off 16-byte (and 2-byte) alignment: the staged tile's single-byte head and tail."""
    run_case(dev, nvec, cells, N, np.int32, True, 7, mask_shift=shift)


def test_error_codes_launch_nothing(dev):
    from rl_algo_impls_amd import _lib

    nv = nvec_arr(R.GRID_NVEC)
    G, N, cells = 7, 2, 4
    src = torch.zeros(N * cells * G, dtype=torch.int32, device=dev)
    dst = torch.zeros(N * cells * G, dtype=torch.int64, device=dev)
    bad = torch.zeros(N, dtype=torch.int32, device=dev)
    src.fill_(99)  # out of range everywhere: any launch would count it
    i32 = _lib.RAI_REF_ACT_I32
    assert call(None, i32, nv, G, None, N, cells, dst, bad) == _lib.RAI_E_NULLPTR
    assert call(src, i32, nv, G, None, N, cells, None, bad) == _lib.RAI_E_NULLPTR
    assert call(src, i32, nv, G, None, N, cells, dst, None) == _lib.RAI_E_NULLPTR
    assert call(src, i32, nv, 0, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    big = nvec_arr([1] * (_lib.RAI_MD_MAX_G + 1))
    assert call(src, i32, big, _lib.RAI_MD_MAX_G + 1, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, i32, nvec_arr([6, 0, 4]), 3, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, i32, nvec_arr([6, -2, 4]), 3, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, i32, nv, G, None, N, 0, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, 2, nv, G, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, -1, nv, G, None, N, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, i32, nv, G, None, -1, cells, dst, bad) == _lib.RAI_E_SHAPE
    assert call(src, i32, nv, G, None, 0, cells, dst, bad) == 0  # RAI_OK
    torch.cuda.synchronize()
    assert not bad.any() and not dst.any(), "an error return launched the kernel"
