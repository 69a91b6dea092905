"""Raw outputs of the MultiDiscrete head kernels (csrc/multidiscrete.hip: rai_md_head_fwd / _bwd, rai_md_sample)
against a float64 torch recomputation of rl_algo_impls/shared/actor/multi_discrete.py over MaskedCategorical.

Tolerance (not fixed in advance), the rule of tests/test_gpu_sde_kernels.py and test_gpu_wide_kernels.py: the
same quantities are computed by the plain-torch float32 head on the CPU (torch Linear + md_ops.logp_entropy_torch
under autograd); a kernel may be off by 4 x that implementation's own max |f32 - f64| per quantity, floored at
1e-6 relative.  Each test prints its worst error / bound ratio."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.md_ops import logp_entropy_torch, nvec_array

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# one row and one logit pair; an odd B with an H that is no multiple of a wave; more than one row block with a
# width-1 group; the H and A limits with the last group ending at A = 256; the G limit
SHAPES = [(1, 1, [2]), (7, 20, [3, 5, 2]), (130, 64, [3, 1, 4]), (65, 512, [32] * 8), (9, 33, [2] * 32)]
QUANTITIES = ("logits", "logp", "entropy", "dx", "dW", "db")


def make_masks(g, B, nvec):
    """Entries valid with probability 0.6, every group repaired to one valid entry at least, then (B >= 3) row 0
    fully valid, row 1 with one valid entry in its widest group and row 2 with an all-false first group."""
    A, off = sum(nvec), np.concatenate([[0], np.cumsum(nvec)])
    mask = torch.rand(B, A, generator=g) < 0.6
    for j, w in enumerate(nvec):
        keep = torch.randint(0, w, (B,), generator=g)
        empty = ~mask[:, off[j]:off[j + 1]].any(dim=1)
        mask[torch.nonzero(empty)[:, 0], off[j] + keep[empty]] = True
    if B >= 3:
        wide = int(np.argmax(nvec))
        mask[0] = True
        mask[1, off[wide]:off[wide + 1]] = False
        mask[1, off[wide] + nvec[wide] // 2] = True
        mask[2, off[0]:off[1]] = False
    return mask


def make_inputs(B, H, nvec, masked, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * len(nvec) + int(masked))
    A, off = sum(nvec), np.concatenate([[0], np.cumsum(nvec)])
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=torch.tanh(r(B, H)), W=r(A, H) * (2.0 / np.sqrt(H)), b=0.1 * r(A), d_logp=r(B), d_entropy=r(B))
    mask = make_masks(g, B, nvec) if masked else None
    valid = mask if masked else torch.ones(B, A, dtype=torch.bool)
    act = torch.zeros(B, len(nvec), dtype=torch.int64)
    for j, w in enumerate(nvec):  # a valid entry of each group (any entry of an all-false group)
        vg = valid[:, off[j]:off[j + 1]].float()
        vg = torch.where(vg.sum(1, keepdim=True) > 0, vg, torch.ones_like(vg))
        act[:, j] = torch.multinomial(vg, 1, generator=g)[:, 0]
    d["actions"], d["mask"] = act, mask
    return d


def torch_head(d, nvec, dtype):
    """The quantities by torch's Linear and the plain-torch head in `dtype` on the CPU."""
    f = lambda k: d[k].to(dtype)
    x, W, b = f("x").requires_grad_(), f("W").requires_grad_(), f("b").requires_grad_()
    logits = torch.nn.functional.linear(x, W, b)
    lp, ent = logp_entropy_torch(logits, nvec, d["actions"], d["mask"])
    dx, dW, db = torch.autograd.grad((f("d_logp") * lp + f("d_entropy") * ent).sum(), [x, W, b])
    return dict(logits=logits.detach(), logp=lp.detach(), entropy=ent.detach(), dx=dx, dW=dW, db=db)


def kernel_head(d, nvec, accumulate=0, pre=None):
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    t = {k: v.to(DEV).contiguous() for k, v in d.items() if v is not None and k != "mask"}
    m = d["mask"].to(DEV).contiguous().view(torch.uint8) if d["mask"] is not None else None
    B, H, A, G = t["x"].shape[0], t["x"].shape[1], sum(nvec), len(nvec)
    nan = lambda *s: torch.full(s, np.nan, device=DEV)
    logits, logp, ent, dq, dx = nan(B, A), nan(B), nan(B), nan(B, A), nan(B, H)
    dW, db = (nan(A, H), nan(A)) if pre is None else pre
    p = lambda k: t[k].data_ptr()
    nv = nvec_array(nvec)
    _lib.check(L.rai_md_head_fwd(p("x"), p("W"), p("b"), _lib.ptr(m), p("actions"), nv, G, B, H, logits.data_ptr(),
                                 logp.data_ptr(), ent.data_ptr(), st), "rai_md_head_fwd")
    _lib.check(L.rai_md_head_bwd(p("x"), p("W"), logits.data_ptr(), _lib.ptr(m), p("actions"), nv, G, p("d_logp"),
                                 p("d_entropy"), B, H, dq.data_ptr(), dx.data_ptr(), dW.data_ptr(), db.data_ptr(),
                                 accumulate, st), "rai_md_head_bwd")
    return dict(logits=logits, logp=logp, entropy=ent, dx=dx, dW=dW, db=db, d_logits=dq)


def bound(ref64, f32):
    """4 x the torch float32 head's own max error, floored at 1e-6 relative (elementwise)."""
    own = float((f32.double() - ref64).abs().max())
    return torch.clamp(1e-6 * ref64.abs(), min=4 * own)


def worst_ratio(got, ref64, f32):
    b = bound(ref64, f32)
    d = (got.double().cpu() - ref64).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / b).max())


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("B,H,nvec", SHAPES, ids=[f"B{B}-H{H}-G{len(n)}-A{sum(n)}" for B, H, n in SHAPES])
def test_head_forward_backward_against_float64(B, H, nvec, masked):
    d = make_inputs(B, H, nvec, masked)
    ref, f32, got = torch_head(d, nvec, torch.float64), torch_head(d, nvec, torch.float32), kernel_head(d, nvec)
    ratios = {q: worst_ratio(got[q], ref[q], f32[q]) for q in QUANTITIES}
    print(f"md head ({B},{H},G={len(nvec)},A={sum(nvec)}) masked={masked}: worst error / bound "
          + " ".join(f"{q}={r:.3f}" for q, r in ratios.items()))
    for q in QUANTITIES:
        assert tuple(got[q].shape) == tuple(ref[q].shape), q
        assert torch.isfinite(got[q]).all(), q
        assert ratios[q] <= 1.0, (q, ratios[q])
    if masked and B >= 3:  # the all-false first group of row 2: no gradient, whatever its action
        a0 = nvec[0]
        ls = got["d_logits"]
        assert torch.equal(ls[2, :a0], torch.zeros(a0, device=DEV))
        assert torch.equal(ls[~d["mask"].to(DEV)], torch.zeros(int((~d["mask"]).sum()), device=DEV))


def test_logits_only_mode_and_out_of_group_action():
    B, H, nvec = 7, 20, [3, 5, 2]
    d = make_inputs(B, H, nvec, True, seed=4)
    full = kernel_head(d, nvec)
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    x, W, b = (d[k].to(DEV).contiguous() for k in ("x", "W", "b"))
    logits = torch.full((B, 10), np.nan, device=DEV)
    _lib.check(L.rai_md_head_fwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), None, None, nvec_array(nvec), 3, B, H,
                                 logits.data_ptr(), None, None, st), "rai_md_head_fwd")
    assert torch.equal(logits, full["logits"])
    bad = dict(d, actions=d["actions"].clone())
    bad["actions"][3, 1] = 5  # group 1 has entries 0..4
    bad["actions"][5, 0] = -1
    got = kernel_head(bad, nvec)
    assert torch.isnan(got["logp"][[3, 5]]).all() and torch.isfinite(got["logp"][[0, 1, 2, 4, 6]]).all()
    assert torch.equal(got["entropy"], full["entropy"]) and torch.isfinite(got["dW"]).all()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_backward_is_deterministic_and_accumulates(masked):
    B, H, nvec = 130, 64, [3, 1, 4]
    d = make_inputs(B, H, nvec, masked, seed=1)
    a, b = kernel_head(d, nvec), kernel_head(d, nvec)
    for q in ("dW", "db", "dx"):
        assert torch.equal(a[q], b[q]), q
    g = torch.Generator().manual_seed(5)
    pre_W, pre_b = torch.randn(8, H, generator=g).to(DEV), torch.randn(8, generator=g).to(DEV)
    acc = kernel_head(d, nvec, accumulate=1, pre=(pre_W.clone(), pre_b.clone()))
    assert torch.equal(acc["dW"], pre_W + a["dW"]) and torch.equal(acc["db"], pre_b + a["db"])


def test_limits_are_reported():
    L = _lib.lib()
    U, nv = _lib.RAI_E_UNSUPPORTED, nvec_array
    fwd = lambda nvec, H: L.rai_md_head_fwd(None, None, None, None, None, nv(nvec), len(nvec), 4, H, None, None, None,
                                            None)
    bwd = lambda nvec, H: L.rai_md_head_bwd(None, None, None, None, None, nv(nvec), len(nvec), None, None, 4, H, None,
                                            None, None, None, 0, None)
    smp = lambda nvec: L.rai_md_sample(None, None, nv(nvec), len(nvec), 4, 1, 0, None, None, None, None, 1, None)
    assert fwd([3, 5, 2], _lib.RAI_MD_MAX_H + 1) == U and bwd([3, 5, 2], _lib.RAI_MD_MAX_H + 1) == U
    assert fwd([32] * 8 + [1], 64) == U and bwd([32] * 8 + [1], 64) == U and smp([32] * 8 + [1]) == U  # A = 257
    assert fwd([2] * 33, 64) == U and bwd([2] * 33, 64) == U and smp([2] * 33) == U  # G = 33
    # at the limits the arguments are looked at: null pointers
    assert fwd([32] * 8, _lib.RAI_MD_MAX_H) == _lib.RAI_E_NULLPTR and smp([2] * 32) == _lib.RAI_E_NULLPTR
    assert fwd([3, 0, 2], 64) == _lib.RAI_E_SHAPE and smp([3, -1]) == _lib.RAI_E_SHAPE


def run_sample(logits, mask, nvec, seed, offset, K=2):
    N, G = logits.shape[0], len(nvec)
    act = torch.full((N, G), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((N,), np.nan, device=DEV)
    v_in = torch.randn(N, K, generator=torch.Generator().manual_seed(4)).to(DEV)
    v_out = torch.full((N, K), np.nan, device=DEV)
    m = mask.contiguous().view(torch.uint8) if mask is not None else None
    _lib.check(_lib.lib().rai_md_sample(logits.data_ptr(), _lib.ptr(m), nvec_array(nvec), G, N, seed, offset,
                                        act.data_ptr(), logp.data_ptr(), v_in.data_ptr(), v_out.data_ptr(), K,
                                        _lib.stream_handle(DEV)), "rai_md_sample")
    assert torch.equal(v_out, v_in)
    return act, logp


def head_logp_of(logits, mask, nvec, act):
    """rai_md_head_fwd's logp at given logits: x = logits, W = I, b = 0 reproduces them exactly."""
    N, A = logits.shape
    W, b = torch.eye(A, device=DEV), torch.zeros(A, device=DEV)
    out, logp, ent = torch.empty(N, A, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    m = mask.contiguous().view(torch.uint8) if mask is not None else None
    _lib.check(_lib.lib().rai_md_head_fwd(logits.data_ptr(), W.data_ptr(), b.data_ptr(), _lib.ptr(m), act.data_ptr(),
                                          nvec_array(nvec), len(nvec), N, A, out.data_ptr(), logp.data_ptr(),
                                          ent.data_ptr(), _lib.stream_handle(DEV)), "rai_md_head_fwd")
    assert torch.equal(out, logits)
    return logp


def test_sampler_frequencies_masks_keys_and_logp():
    N, nvec = 4096, [3, 5, 2]
    row = torch.tensor([0.3, -0.5, 0.1, 1.0, -2.0, 0.4, 0.0, -0.3, 0.6, -0.6])
    mrow = torch.tensor([1, 1, 1, 1, 0, 1, 0, 1, 1, 1], dtype=torch.bool)  # two entries of group 1 masked
    off = [0, 3, 8, 10]
    # the true probabilities (float64, CPU) and the distance of the 5-sigma bound from a false alarm
    probs = []
    for lo, hi in zip(off[:-1], off[1:]):
        z = torch.where(mrow[lo:hi], row[lo:hi].double(), torch.tensor(-float("inf"), dtype=torch.float64))
        probs.append(torch.softmax(z, 0))
    p = torch.cat(probs)
    assert float((N * p[mrow]).min()) >= 50, "the smallest expected count keeps the normal bound meaningful"
    logits = row.repeat(N, 1).to(DEV).contiguous()
    mask = mrow.repeat(N, 1).to(DEV).contiguous()
    act, logp = run_sample(logits, mask, nvec, 1234, 7)
    a = act.cpu()
    for g, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        assert ((a[:, g] >= 0) & (a[:, g] < hi - lo)).all()
        counts = torch.bincount(a[:, g], minlength=hi - lo).double()
        assert (counts[~mrow[lo:hi]] == 0).all(), "a masked action was drawn"
        pg = p[lo:hi]
        dev = (counts - N * pg).abs() / torch.sqrt(N * pg * (1 - pg)).clamp(min=1e-12)
        print(f"md sampler group {g}: counts {counts.tolist()} expected {(N * pg).tolist()} worst sigma "
              f"{float(dev[mrow[lo:hi]].max()):.2f}")
        assert (dev[mrow[lo:hi]] <= 5).all()
    # logp of the stored actions: rai_md_head_fwd's, bit for bit
    assert torch.equal(logp, head_logp_of(logits, mask, nvec, act))
    ref = sum(torch.log(p[off[g] + a[:, g]]) for g in range(3))
    np.testing.assert_allclose(logp.cpu().double().numpy(), ref.numpy(), rtol=1e-6, atol=1e-6)
    act2, logp2 = run_sample(logits, mask, nvec, 1234, 7)
    assert torch.equal(act, act2) and torch.equal(logp, logp2)
    act3, _ = run_sample(logits, mask, nvec, 1234, 8)
    assert not torch.equal(act, act3)
    # no mask: every entry is drawn, and the logp still matches the head's
    act4, logp4 = run_sample(logits, None, nvec, 99, 0)
    assert all(torch.unique(act4[:, g]).numel() == n for g, n in enumerate(nvec))
    assert torch.equal(logp4, head_logp_of(logits, None, nvec, act4))


@pytest.mark.parametrize("N,nvec", [(7, [3, 1, 4]), (65, [32] * 8), (9, [2] * 32)], ids=["w1", "A256", "G32"])
def test_sampler_edge_shapes_stay_valid_and_match_the_head(N, nvec):
    g = torch.Generator().manual_seed(N)
    A, off = sum(nvec), np.concatenate([[0], np.cumsum(nvec)])
    logits = (2.0 * torch.randn(N, A, generator=g)).to(DEV)
    mask = make_masks(g, N, nvec).to(DEV)
    act, logp = run_sample(logits, mask, nvec, 5, 11)
    a, m = act.cpu(), mask.cpu()
    for j, w in enumerate(nvec):
        assert ((a[:, j] >= 0) & (a[:, j] < w)).all()
        any_valid = m[:, off[j]:off[j + 1]].any(1)
        picked = m[torch.arange(N), off[j] + a[:, j]]
        assert picked[any_valid].all(), "a masked action was drawn"
    assert torch.isfinite(logp).all()
    assert torch.equal(logp, head_logp_of(logits, mask, nvec, act))
