"""csrc/conv3x3.hip kernel by kernel against float64 oracles computed in-test with torch on the CPU.

The error rule is the one test_gpu_conv.py:66-72 derives: any f32 summation order of K products obeys
|y - ref64| <= (K + 3) * 2^-24 * sum|terms| (the +3: the bias, the residual and the final rounding), with
sum|terms| from the same convolution of absolute values plus |res|.  K = 9 * Ci for the forward, the pixel
count B * H * W for the weight gradient.  The input gradient sums 9 * Co products, so its derived bound has
K = 9 * Co; the test holds it to K = 9 * Ci, which is never larger in the cases here (Ci <= Co in every
pair, asserted below), i.e. a tighter bound than the derived one.  An indexing or padding error is O(1)
relative, far outside either.  Every output is pre-filled with NaN, so an unwritten element shows."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rl_algo_impls_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS = 2.0 ** -24
HWS = [(1, 1), (2, 3), (5, 3), (11, 11), (16, 16)]
BS = [1, 7]
CHANS = [(16, 16), (16, 32), (32, 32), (64, 128)]


def _rng(*key):
    return np.random.default_rng([20261019, *key])


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _st():
    return _lib.stream_handle(DEV)


def _nchw64(x):  # (B, H, W, C) -> (B, C, H, W) float64
    return x.double().permute(0, 3, 1, 2)


def _w64(w):  # (Co, 3, 3, Ci) -> (Co, Ci, 3, 3) float64
    return w.double().permute(0, 3, 1, 2)


def _case(B, H, W, Ci, Co, key):
    r = _rng(B, H, W, Ci, Co, key)
    x = _t(r.standard_normal((B, H, W, Ci)))
    w = _t(r.standard_normal((Co, 3, 3, Ci)) / np.sqrt(9 * Ci))
    b = _t(r.standard_normal(Co) * 0.1)
    return x, w, b, r


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("hw", HWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv3x3_fwd(hw, B):
    H, W = hw
    L = _lib.lib()
    for Ci, Co in CHANS:
        x, w, b, r = _case(B, H, W, Ci, Co, 0)
        res = _t(r.standard_normal((B, H, W, Co)))
        xd, wd, bd, resd = (t.to(DEV) for t in (x, w, b, res))
        ref = {p: F.conv2d(_nchw64(x.clamp_min(0) if p else x), _w64(w), b.double(), padding=1) for p in (0, 1)}
        mag = {p: F.conv2d(_nchw64((x.clamp_min(0) if p else x).abs()), _w64(w).abs(), b.double().abs(), padding=1)
               for p in (0, 1)}
        for pre, use_res, post, nchw in itertools.product((0, 1), repeat=4):
            y = _nan(B, Co * H * W) if nchw else _nan(B, H, W, Co)
            rc = L.rai_conv3x3_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), resd.data_ptr() if use_res else None,
                                   B, H, W, Ci, Co, pre, post, nchw, y.data_ptr(), _st())
            assert rc == 0, (rc, Ci, Co)
            want, m = ref[pre], mag[pre]
            if use_res:
                want, m = want + _nchw64(res), m + _nchw64(res).abs()
            if post:
                want = want.clamp_min(0)
            got = y.cpu().double()
            got = got.view(B, Co, H, W) if nchw else got.permute(0, 3, 1, 2)
            assert torch.isfinite(got).all(), (Ci, Co, pre, use_res, post, nchw)
            bound = (9 * Ci + 3) * EPS * m
            err = (got - want).abs()
            assert (err <= bound).all(), (Ci, Co, pre, use_res, post, nchw, float((err / bound.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("hw", HWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv3x3_dgrad(hw, B):
    H, W = hw
    L = _lib.lib()
    for Ci, Co in CHANS:
        assert Ci <= Co  # K = 9 * Ci below is then at most the reduction length 9 * Co of the derived bound
        _, w, _, r = _case(B, H, W, Ci, Co, 1)
        dz = _t(r.standard_normal((B, H, W, Co)))
        m = _t(r.standard_normal((B, H, W, Ci)))
        m[..., 0] = 0.0  # a zero counts as masked (threshold_backward: m <= 0)
        res = _t(r.standard_normal((B, H, W, Ci)))
        dzd, wd, md, resd = (t.to(DEV) for t in (dz, w, m, res))
        ref = F.conv_transpose2d(_nchw64(dz), _w64(w), padding=1)
        mag = F.conv_transpose2d(_nchw64(dz).abs(), _w64(w).abs(), padding=1)
        for use_m, use_res in itertools.product((0, 1), repeat=2):
            dx = _nan(B, H, W, Ci)
            rc = L.rai_conv3x3_dgrad(dzd.data_ptr(), wd.data_ptr(), md.data_ptr() if use_m else None,
                                     resd.data_ptr() if use_res else None, B, H, W, Ci, Co, dx.data_ptr(), _st())
            assert rc == 0, (rc, Ci, Co)
            want, mg = ref, mag
            if use_m:
                keep = (_nchw64(m) > 0).double()
                want, mg = want * keep, mg * keep
            if use_res:
                want, mg = want + _nchw64(res), mg + _nchw64(res).abs()
            got = dx.cpu().double().permute(0, 3, 1, 2)
            assert torch.isfinite(got).all(), (Ci, Co, use_m, use_res)
            bound = (9 * Ci + 3) * EPS * mg
            err = (got - want).abs()
            assert (err <= bound).all(), (Ci, Co, use_m, use_res, float((err / bound.clamp_min(1e-30)).max()))


def _wgrad_ref(x64, dz64):
    """dw (Co, 3, 3, Ci) and db (Co) in float64 from NHWC x (zero padded here) and dz."""
    xp = F.pad(x64, (0, 0, 1, 1, 1, 1))
    H, W = x64.shape[1], x64.shape[2]
    dw = torch.stack([torch.stack([torch.einsum("nhwo,nhwi->oi", dz64, xp[:, kh:kh + H, kw:kw + W])
                                   for kw in range(3)], 1) for kh in range(3)], 1)
    return dw, dz64.sum((0, 1, 2))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("hw", HWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv3x3_wgrad(hw, B):
    H, W = hw
    L = _lib.lib()
    K = B * H * W
    for Ci, Co in CHANS:
        x, _, _, r = _case(B, H, W, Ci, Co, 2)
        dz = _t(r.standard_normal((B, H, W, Co)))
        base_w = _t(r.standard_normal((Co, 3, 3, Ci)))
        base_b = _t(r.standard_normal(Co))
        xd, dzd = x.to(DEV), dz.to(DEV)
        nb = int(L.rai_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co))
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        for pre, acc in itertools.product((0, 1), repeat=2):
            xin = x.clamp_min(0) if pre else x
            want_w, want_b = _wgrad_ref(xin.double(), dz.double())
            mag_w, mag_b = _wgrad_ref(xin.double().abs(), dz.double().abs())
            if acc:
                want_w, want_b = want_w + base_w.double(), want_b + base_b.double()
                mag_w, mag_b = mag_w + base_w.double().abs(), mag_b + base_b.double().abs()
            runs = []
            for _ in range(2):
                dw = base_w.to(DEV) if acc else _nan(Co, 3, 3, Ci)
                db = base_b.to(DEV) if acc else _nan(Co)
                rc = L.rai_conv3x3_wgrad(xd.data_ptr(), dzd.data_ptr(), B, H, W, Ci, Co, pre, dw.data_ptr(),
                                         db.data_ptr(), acc, ws.data_ptr(), nb, _st())
                assert rc == 0, (rc, Ci, Co)
                runs.append((dw.cpu(), db.cpu()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
            gw, gb = runs[0][0].double(), runs[0][1].double()
            assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
            for got, want, mag, what in ((gw, want_w, mag_w, "dw"), (gb, want_b, mag_b, "db")):
                bound = (K + 3) * EPS * mag
                err = (got - want).abs()
                assert (err <= bound).all(), (what, Ci, Co, pre, acc, float((err / bound.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("hw", [(5, 3), (20, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("Co", [16, 32])
@pytest.mark.parametrize("Ci", [3, 4])
def test_first_layer(Ci, Co, hw):
    """uint8 input (x / divisor in-kernel) == the fp32 kernel on x.float() / divisor formed with a device
    scalar divisor (as cnn_ops._u8_to_f32), bit for bit, forward and weight gradient; and the fp32 result
    against the float64 oracle."""
    H, W = hw
    B, div = 7, 255.0
    L = _lib.lib()
    r = _rng(Ci, Co, H, W, 3)
    xu = torch.from_numpy(r.integers(0, 256, size=(B, H, W, Ci), dtype=np.uint8))
    w = _t(r.standard_normal((Co, 3, 3, Ci)) / np.sqrt(9 * Ci))
    b = _t(r.standard_normal(Co) * 0.1)
    dz = _t(r.standard_normal((B, H, W, Co)))
    xud, wd, bd, dzd = (t.to(DEV) for t in (xu, w, b, dz))
    xfd = (xud.float() / torch.full((), div, dtype=torch.float32, device=DEV)).contiguous()
    np.testing.assert_array_equal(xfd.cpu().numpy(), xu.numpy().astype(np.float32) / np.float32(div))
    ys = []
    for x, u8 in ((xud, 1), (xfd, 0)):
        y = _nan(B, H, W, Co)
        assert L.rai_conv3x3_fwd_first(x.data_ptr(), u8, div, wd.data_ptr(), bd.data_ptr(), B, H, W, Ci, Co,
                                       y.data_ptr(), _st()) == 0
        ys.append(y.cpu())
    assert torch.isfinite(ys[0]).all() and torch.equal(ys[0], ys[1])
    x64 = xfd.cpu().double()
    want = F.conv2d(_nchw64(x64), _w64(w), b.double(), padding=1)
    mag = F.conv2d(_nchw64(x64).abs(), _w64(w).abs(), b.double().abs(), padding=1)
    err = (ys[1].double().permute(0, 3, 1, 2) - want).abs()
    assert (err <= (9 * Ci + 3) * EPS * mag).all()

    nb = int(L.rai_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    gs = []
    for x, u8 in ((xud, 1), (xfd, 0)):
        dw, db = _nan(Co, 3, 3, Ci), _nan(Co)
        assert L.rai_conv3x3_wgrad_first(x.data_ptr(), u8, div, dzd.data_ptr(), B, H, W, Ci, Co, dw.data_ptr(),
                                         db.data_ptr(), 0, ws.data_ptr(), nb, _st()) == 0
        gs.append((dw.cpu(), db.cpu()))
    assert torch.equal(gs[0][0], gs[1][0]) and torch.equal(gs[0][1], gs[1][1])
    want_w, want_b = _wgrad_ref(x64, dz.double())
    mag_w, mag_b = _wgrad_ref(x64.abs(), dz.double().abs())
    K = B * H * W
    assert ((gs[1][0].double() - want_w).abs() <= (K + 3) * EPS * mag_w).all()
    assert ((gs[1][1].double() - want_b).abs() <= (K + 3) * EPS * mag_b).all()
    # accumulate adds onto what is there
    dw, db = gs[1][0].to(DEV), gs[1][1].to(DEV)
    assert L.rai_conv3x3_wgrad_first(xfd.data_ptr(), 0, div, dzd.data_ptr(), B, H, W, Ci, Co, dw.data_ptr(),
                                     db.data_ptr(), 1, ws.data_ptr(), nb, _st()) == 0
    assert torch.equal(dw.cpu(), gs[1][0] + gs[1][0]) and torch.equal(db.cpu(), gs[1][1] + gs[1][1])


def _pool(x):
    """rai_maxpool3x3s2_fwd on an NHWC CPU tensor -> (y, argmax) on the CPU."""
    B, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = _nan(B, OH, OW, C)
    am = torch.full((B, OH, OW, C), 255, dtype=torch.uint8, device=DEV)
    xd = x.to(DEV)
    assert _lib.lib().rai_maxpool3x3s2_fwd(xd.data_ptr(), B, H, W, C, y.data_ptr(), am.data_ptr(), _st()) == 0
    return y, am


def _pool_bwd(dy, am, H, W):
    B, _, _, C = dy.shape
    dx = _nan(B, H, W, C)
    dyd = dy.to(DEV)
    assert _lib.lib().rai_maxpool3x3s2_bwd(dyd.data_ptr(), am.data_ptr(), B, H, W, C, dx.data_ptr(), _st()) == 0
    return dx.cpu()


def _torch_pool(x, dy):
    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(xc, 3, stride=2, padding=1)
    y.backward(dy.permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), xc.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 3), (21, 21), (12, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxpool(hw, C, B):
    H, W = hw
    r = _rng(B, H, W, C, 4)
    n = B * H * W * C
    x = _t(r.permutation(n).reshape(B, H, W, C) - n // 2)  # distinct integers: no ties
    y, am = _pool(x)
    OH, OW = y.shape[1], y.shape[2]
    assert (OH, OW) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    dy = _t(r.integers(-3, 4, size=(B, OH, OW, C)))  # small integers: the sums are exact
    want_y, want_dx = _torch_pool(x, dy)
    assert torch.equal(y.cpu(), want_y)
    assert int(am.max()) <= 8
    assert torch.equal(_pool_bwd(dy, am, H, W), want_dx)


def test_maxpool_ties_and_nan():
    B, H, W, C = 2, 5, 6, 16
    x = torch.full((B, H, W, C), 1.5)
    y, am = _pool(x)
    OH, OW = y.shape[1], y.shape[2]
    dy = _t(_rng(5).integers(1, 4, size=(B, OH, OW, C)))
    want_y, want_dx = _torch_pool(x, dy)
    assert torch.equal(y.cpu(), want_y)
    assert torch.equal(_pool_bwd(dy, am, H, W), want_dx)  # the first in-bounds position of each window wins
    x = _t(_rng(6).standard_normal((B, H, W, C)))
    x[0, 2, 3, 5] = float("nan")
    y, _ = _pool(x)
    want_y, _ = _torch_pool(x, torch.zeros(B, OH, OW, C))
    got = y.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want_y)) and torch.isnan(got).sum() >= 1
    assert torch.equal(got[~torch.isnan(got)], want_y[~torch.isnan(want_y)])


def test_unsupported_shapes_launch_nothing():
    L = _lib.lib()
    B, H, W = 2, 4, 4
    buf = torch.zeros(B * H * W * 144 + 8, dtype=torch.float32, device=DEV)
    wbuf = torch.zeros(144 * 9 * 144, dtype=torch.float32, device=DEV)
    bias = torch.zeros(144, dtype=torch.float32, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for Ci, Co, off in ((24, 16, 0), (16, 144, 0), (16, 16, 4)):
        y = _nan(B * H * W * 144)
        xp = buf.data_ptr() + off  # off = 4: a pointer that is only 4-B aligned
        assert L.rai_conv3x3_fwd(xp, wbuf.data_ptr(), bias.data_ptr(), None, B, H, W, Ci, Co, 0, 0, 0, y.data_ptr(),
                                 _st()) == _lib.RAI_E_UNSUPPORTED
        assert L.rai_conv3x3_dgrad(xp, wbuf.data_ptr(), None, None, B, H, W, Ci, Co, y.data_ptr(),
                                   _st()) == _lib.RAI_E_UNSUPPORTED
        assert L.rai_conv3x3_wgrad(xp, buf.data_ptr(), B, H, W, Ci, Co, 0, y.data_ptr(), None, 0, ws.data_ptr(),
                                   ws.numel(), _st()) == _lib.RAI_E_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.isnan(y).all()  # nothing was launched
    assert L.rai_conv3x3_wgrad_workspace_bytes(B, H, W, 24, 16) == 0
    y = _nan(64)
    assert L.rai_conv3x3_fwd_first(buf.data_ptr(), 0, 1.0, wbuf.data_ptr(), bias.data_ptr(), B, H, W, 5, 16,
                                   y.data_ptr(), _st()) == _lib.RAI_E_UNSUPPORTED
    assert L.rai_maxpool3x3s2_fwd(buf.data_ptr(), B, H, W, 6, y.data_ptr(), ws.data_ptr(), _st()) \
        == _lib.RAI_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


def test_shape_gate_sends_other_widths_to_the_fallback():
    """impala_channels outside the kernels' range: the gate, evaluated before any launch, picks the
    module path (F.conv2d / F.max_pool2d, still on the GPU); nothing raises."""
    from rl_algo_impls_amd import impala_ops
    from rl_algo_impls_amd.envs import Box
    from rl_algo_impls_amd.policy import ImpalaCnnEncoder

    torch.manual_seed(3)
    space = Box(0, 255, (3, 20, 12), np.uint8)
    obs = torch.from_numpy(_rng(7).integers(0, 256, size=(5, 3, 20, 12), dtype=np.uint8))
    for chans, want in (((24, 32, 32), False), ((16, 144, 32), False), ((16, 32, 32), True)):
        enc = ImpalaCnnEncoder(space, torch.nn.ReLU, None, True, 64, chans)
        ref = enc(obs)
        enc = enc.to(DEV)
        assert impala_ops.fusable(enc, obs.to(DEV)) is want
        assert enc.obs_transform(obs.to(DEV)) is not None if want else enc.obs_transform(obs.to(DEV)) is None
        out = enc(obs.to(DEV))
        assert tuple(out.shape) == tuple(ref.shape) and bool(torch.isfinite(out).all())
    # an input that wants a gradient: the first layer has no input-gradient kernel, so the gate takes the
    # module path and its backward runs (nothing fails mid-graph)
    xg = (obs.to(DEV).float() / 255).requires_grad_()
    assert impala_ops.fusable(enc, xg) is False
    enc(xg, prepared=True).sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
