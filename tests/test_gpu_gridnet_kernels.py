"""Raw outputs of the GridNet head kernels (csrc/gridnet.hip: rai_gridnet_logp_entropy / _backward / _sample /
_num_actions) against float64, at the shapes where the tile loop, the sampler's two code paths, the group table and
the LDS request change.

References.  The float64 reference is oracle.gridnet_logp_entropy_grad (checked against the reference project's
golden cases in test_gridnet.py).  `torch_head` below restates the same head in plain torch (torch.where(mask, z,
finfo(float32).min), logsumexp, gather, the masked entropy and the ValueDependentMask gate, autograd for the gradient
of sum_b wl[b] logp[b] + we[b] H[b]); test_torch_restatement_matches_the_oracle holds its float64 outputs to the
oracle's within 1e-12 of each quantity's scale (rtol 1e-12, atol 1e-12 max |ref|) without a GPU, so the two guard
each other.

Tolerance (not fixed in advance), the rule of test_gpu_multidiscrete_kernels.py: per quantity (logp, entropy,
d_logits) a kernel may be off by 4 x the float32 torch_head's own max |f32 - f64| on the same inputs, floored at
1e-6 relative.  Each test prints its worst error / bound ratio.  Masked entries of d_logits and whole all-masked
groups are exactly 0.0.

Inputs.  Masks by tests/golden/make_golden_gridnet.py's recipe over any nvec (density 0.5, 30 % empty cells, 10 %
killed groups), with three cells forced where there are three: one fully valid, one whose widest group has exactly
one valid entry, one whose widest group is all masked under a nonzero action.  Logits once as 2 N(0,1) and once as
30 N(0,1) plus +-60 per (cell, group): the float32 torch_head stays finite at that scale (asserted on the CPU), and a
kernel without the max-subtraction would overflow there.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle as O
from rl_algo_impls_amd import _lib

gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F32_MIN = float(torch.finfo(torch.float32).min)
RTS = [6, 4, 4, 4, 4, 7, 49]
RTS_GATE = {1: (0, 1), 2: (0, 2), 3: (0, 3), 4: (0, 4), 5: (0, 4), 6: (0, 5)}  # group: (reference plane, value)
W70 = ([1, 3, 1, 70], {3: (1, 2)})
A256 = ([64] * 4, {1: (0, 3), 2: (0, 5)})
# name: (B, C, nvec, gate table); each the smallest shape that reaches its path
CASES = {
    "min": (1, 1, [2], None),
    "rts-C63": (3, 63, RTS, RTS_GATE),  # one short tile
    "rts-C64": (3, 64, RTS, RTS_GATE),  # one full tile
    "rts-C65": (3, 65, RTS, RTS_GATE),  # a full tile and one cell
    "w1-w70-C130": (2, 130) + W70,  # width-1 groups, a 70-wide plane, a gate on plane 1, two tiles and a remainder
    "G8-A256": (5, 3, [32] * 8, None),  # the G and A limits with few cells
    "A256-C70": (2, 70) + A256,  # A = 256 across a tile boundary
    "flat-A256": (300, 1, [256], None),  # the flat Categorical fallback as policy.py calls it
    "A204": (2, 2, [51] * 4, None),  # the last A whose tile fits a kernel's default dynamic-LDS limit
    "A205": (2, 2, [41] * 5, None),  # the first A whose tile does not
}
SCALES = {"unit": (2.0, 0.0), "large": (30.0, 60.0)}
QUANTITIES = ("logp", "entropy", "d_logits")


def offsets(nvec):
    return np.concatenate([[0], np.cumsum(nvec)]).astype(np.int64)


def gate_arrays(nvec, gates):
    ref, val = np.full(len(nvec), -1, dtype=np.int32), np.zeros(len(nvec), dtype=np.int32)
    for g, (r, v) in (gates or {}).items():
        ref[g], val[g] = r, v
    return ref, val


@functools.lru_cache(maxsize=None)
def make_case(name, scale):
    """The inputs of one case as numpy arrays (never modified: the tests copy what they change)."""
    B, Cc, nvec, gates = CASES[name]
    std, shift = SCALES[scale]
    rng = np.random.default_rng(1000 * list(CASES).index(name) + list(SCALES).index(scale))
    G, A, off, R = len(nvec), sum(nvec), offsets(nvec), B * Cc
    z = rng.standard_normal((R, A)) * std
    for g in range(G):
        z[:, off[g]:off[g + 1]] += shift * rng.choice([-1.0, 1.0], size=(R, 1))
    m = rng.random((R, A)) < 0.5
    m[rng.random(R) < 0.3] = False  # empty cells
    for g in range(G):
        m[rng.random(R) < 0.1, off[g]:off[g + 1]] = False  # killed groups
    wide = int(np.argmax(nvec))
    ws = slice(off[wide], off[wide + 1])
    forced = None
    if R >= 3:
        full, single, dead = (int(r) for r in rng.choice(R, 3, replace=False))
        m[full] = True
        m[single, ws] = False
        m[single, off[wide] + nvec[wide] // 2] = True
        m[dead, ws] = False
        forced = dict(full=full, single=single, dead=dead, wide=wide)
    else:
        m[0] = True
    a = np.zeros((R, G), dtype=np.int64)
    for r in range(R):
        for g in range(G):
            valid = np.flatnonzero(m[r, off[g]:off[g + 1]])
            a[r, g] = rng.choice(valid) if len(valid) else 0
    for g, (ref, val) in (gates or {}).items():  # open every gate on a share of the cells where its value is valid
        rows = (rng.random(R) < 0.3) & m[:, off[ref] + val]
        a[rows, ref] = val
    if forced:
        a[dead, wide] = nvec[wide] - 1  # an all-masked group under a nonzero action
    d = dict(logits=z.astype(np.float32).reshape(B, Cc, A), masks=m.reshape(B, Cc, A), actions=a.reshape(B, Cc, G),
             w_logp=rng.standard_normal(B).astype(np.float32), w_ent=rng.standard_normal(B).astype(np.float32),
             forced=forced)
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def torch_head(d, nvec, gates, dtype):
    """logp (B,), entropy (B,) and d(sum_b wl logp + we H)/dlogits in `dtype` on the CPU: plain torch + autograd."""
    z = torch.tensor(d["logits"]).to(dtype).requires_grad_()
    m, a = torch.tensor(d["masks"]), torch.tensor(d["actions"])
    neg, zero, off = torch.tensor(F32_MIN, dtype=dtype), torch.zeros((), dtype=dtype), offsets(nvec)
    logp, ent = 0, 0
    for g in range(len(nvec)):
        mg = m[..., off[g]:off[g + 1]]
        zm = torch.where(mg, z[..., off[g]:off[g + 1]], neg)
        l = zm - torch.logsumexp(zm, -1, keepdim=True)
        ent = ent - torch.where(mg, l * l.exp(), zero).sum(-1)
        la = l.gather(-1, a[..., g:g + 1])[..., 0]
        if gates and g in gates:
            la = torch.where(a[..., gates[g][0]] == gates[g][1], la, zero)
        logp = logp + la
    logp, ent = logp.sum(-1), ent.sum(-1)
    wl, we = torch.tensor(d["w_logp"]).to(dtype), torch.tensor(d["w_ent"]).to(dtype)
    (grad,) = torch.autograd.grad((wl * logp + we * ent).sum(), [z])
    return dict(logp=logp.detach(), entropy=ent.detach(), d_logits=grad)


def oracle_head(d, nvec, gates):
    ref, val = gate_arrays(nvec, gates)
    lp, en, gr = O.gridnet_logp_entropy_grad(d["logits"], d["masks"], d["actions"], np.asarray(nvec),
                                             ref if gates else None, val, d["w_logp"].astype(np.float64),
                                             d["w_ent"].astype(np.float64))
    return dict(logp=torch.tensor(lp), entropy=torch.tensor(en), d_logits=torch.tensor(gr))


@functools.lru_cache(maxsize=None)
def references(name, scale):
    """(float64 oracle, float32 torch_head) of a case, computed once."""
    _, _, nvec, gates = CASES[name]
    d = make_case(name, scale)
    return oracle_head(d, nvec, gates), torch_head(d, nvec, gates, torch.float32)


def bound(ref64, f32):
    """4 x the float32 torch_head's own max error, floored at 1e-6 relative (elementwise)."""
    own = float((f32.double() - ref64).abs().max())
    return torch.clamp(1e-6 * ref64.abs(), min=4 * own)


def worst_ratio(got, ref64, f32):
    b = bound(ref64, f32)
    d = (got.double().cpu() - ref64).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / b).max())


def check_ratios(what, got, ref, f32, quantities=QUANTITIES):
    ratios = {q: worst_ratio(got[q], ref[q], f32[q]) for q in quantities}
    print(f"gridnet {what}: worst error / bound " + " ".join(f"{q}={r:.3f}" for q, r in ratios.items()))
    for q in quantities:
        assert tuple(got[q].shape) == tuple(ref[q].shape), q
        assert torch.isfinite(got[q]).all(), q
        assert ratios[q] <= 1.0, (q, ratios[q])
    return ratios


# ---- the two references against each other (no GPU) ----------------------------------------------------------------

def test_torch_restatement_matches_the_oracle():
    for name, (B, Cc, nvec, gates) in CASES.items():
        for scale in SCALES:
            d = make_case(name, scale)
            ref, _ = references(name, scale)
            t64 = torch_head(d, nvec, gates, torch.float64)
            for q in QUANTITIES:
                np.testing.assert_allclose(t64[q].numpy(), ref[q].numpy(), rtol=1e-12,
                                           atol=1e-12 * float(ref[q].abs().max()), err_msg=f"{name} {scale} {q}")


def test_inputs_hold_the_forced_edges_and_float32_torch_stays_finite():
    for name, (B, Cc, nvec, gates) in CASES.items():
        off = offsets(nvec)
        for scale in SCALES:
            d = make_case(name, scale)
            _, f32 = references(name, scale)
            for q in QUANTITIES:
                assert torch.isfinite(f32[q]).all(), (name, scale, q)
            m, a, f = d["masks"].reshape(B * Cc, -1), d["actions"].reshape(B * Cc, -1), d["forced"]
            assert 0.2 < m.mean() < 0.6 or B * Cc < 3
            if f is None:
                assert B * Cc < 3 and m[0].all()
                continue
            ws = slice(off[f["wide"]], off[f["wide"] + 1])
            assert m[f["full"]].all() and m[f["single"], ws].sum() == 1
            assert not m[f["dead"], ws].any() and a[f["dead"], f["wide"]] > 0
            for g, (r, v) in (gates or {}).items():  # every gate open somewhere and closed somewhere
                assert 0 < (a[:, r] == v).sum() < B * Cc, (name, g)


# ---- kernel launches -----------------------------------------------------------------------------------------------

def spec_ptrs(nvec, gates):
    """Host arrays of a launch; sub_ref / sub_val are NULL without a gate table."""
    nv = (C.c_int32 * len(nvec))(*nvec)
    if not gates:
        return nv, None, None
    ref, val = gate_arrays(nvec, gates)
    return nv, (C.c_int32 * len(nvec))(*ref.tolist()), (C.c_int32 * len(nvec))(*val.tolist())


def device_inputs(d):
    z = torch.tensor(d["logits"]).to(DEV).contiguous()
    m = torch.tensor(d["masks"]).to(DEV).contiguous().view(torch.uint8)
    a = torch.tensor(d["actions"]).to(DEV).contiguous()
    return z, m, a


def kernel_forward(z, m, a, nvec, gates, want_logp=True):
    B, Cc = z.shape[0], z.shape[1]
    nv, sr, sv = spec_ptrs(nvec, gates)
    logp, ent = torch.full((B,), np.nan, device=DEV), torch.full((B,), np.nan, device=DEV)
    _lib.check(_lib.lib().rai_gridnet_logp_entropy(z.data_ptr(), m.data_ptr(), _lib.ptr(a), B, Cc, len(nvec), nv, sr,
                                                   sv, logp.data_ptr() if want_logp else None, ent.data_ptr(),
                                                   _lib.stream_handle(DEV)), "rai_gridnet_logp_entropy")
    return logp, ent


def kernel_backward(z, m, a, nvec, gates, wl, we):
    B, Cc = z.shape[0], z.shape[1]
    nv, sr, sv = spec_ptrs(nvec, gates)
    dz = torch.full_like(z, np.nan)
    _lib.check(_lib.lib().rai_gridnet_backward(z.data_ptr(), m.data_ptr(), a.data_ptr(), B, Cc, len(nvec), nv, sr, sv,
                                               wl.data_ptr(), we.data_ptr(), dz.data_ptr(), _lib.stream_handle(DEV)),
               "rai_gridnet_backward")
    return dz


def kernel_head(d, nvec, gates):
    z, m, a = device_inputs(d)
    z0 = z.clone()
    logp, ent = kernel_forward(z, m, a, nvec, gates)
    dz = kernel_backward(z, m, a, nvec, gates, torch.tensor(d["w_logp"]).to(DEV), torch.tensor(d["w_ent"]).to(DEV))
    assert torch.equal(z, z0), "the kernels leave their logits alone"
    return dict(logp=logp, entropy=ent, d_logits=dz)


def kernel_sample(z, m, nvec, gates, seed, offset):
    B, Cc = z.shape[0], z.shape[1]
    nv, sr, sv = spec_ptrs(nvec, gates)
    act = torch.full((B, Cc, len(nvec)), -1, dtype=torch.int64, device=DEV)
    logp = torch.full((B,), np.nan, device=DEV)
    _lib.check(_lib.lib().rai_gridnet_sample(z.data_ptr(), m.data_ptr(), B, Cc, len(nvec), nv, sr, sv, seed, offset,
                                             act.data_ptr(), logp.data_ptr(), _lib.stream_handle(DEV)),
               "rai_gridnet_sample")
    return act, logp


def assert_masked_gradients_are_zero(d, nvec, dz):
    """Masked entries (all-masked groups among them, whatever their action) carry exactly 0.0."""
    dead = ~torch.tensor(d["masks"])
    assert torch.equal(dz.cpu()[dead], torch.zeros(int(dead.sum())))
    f = d["forced"]
    if f is not None:
        off = offsets(nvec)
        cell = dz.cpu().reshape(-1, dz.shape[-1])[f["dead"], off[f["wide"]]:off[f["wide"] + 1]]
        assert torch.equal(cell, torch.zeros(nvec[f["wide"]]))


# ---- forward and backward ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_against_float64(name, scale):
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, scale)
    ref, f32 = references(name, scale)
    got = kernel_head(d, nvec, gates)
    check_ratios(f"{name} (B={B}, C={Cc}, G={len(nvec)}, A={sum(nvec)}) {scale}", got, ref, f32)
    assert_masked_gradients_are_zero(d, nvec, got["d_logits"])
    off = offsets(nvec)
    for g, n in enumerate(nvec):  # a width-1 group: l = 0, p = 1, H = 0, no gradient
        if n == 1:
            assert torch.equal(got["d_logits"][..., off[g]], torch.zeros(B, Cc, device=DEV))


@gpu
@pytest.mark.parametrize("scale", list(SCALES))
def test_entropy_only_mode(scale):
    name = "rts-C65"
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, scale)
    z, m, a = device_inputs(d)
    _, ent_full = kernel_forward(z, m, a, nvec, gates)
    logp_none, ent_only = kernel_forward(z, m, None, nvec, gates, want_logp=False)
    assert torch.equal(ent_only, ent_full) and torch.isnan(logp_none).all()  # no actions: logp_out is not written
    # the backward of the entropy term alone: d_logp = 0 over placeholder actions, as GridnetLogpEntropy calls it
    d0 = dict(d, actions=np.zeros_like(d["actions"]), w_logp=np.zeros_like(d["w_logp"]))
    ref, f32 = oracle_head(d0, nvec, gates), torch_head(d0, nvec, gates, torch.float32)
    dz = kernel_backward(z, m, torch.zeros_like(a), nvec, gates, torch.zeros(B, device=DEV),
                         torch.tensor(d["w_ent"]).to(DEV))
    check_ratios(f"{name} {scale} entropy only", dict(entropy=ent_only, d_logits=dz), ref, f32,
                 ("entropy", "d_logits"))
    assert_masked_gradients_are_zero(d0, nvec, dz)


@gpu
def test_masked_action_in_a_live_group():
    name = "flat-A256"
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, "unit")
    m = d["masks"].reshape(B, -1)
    b = int(np.flatnonzero(m.any(1) & ~m.all(1))[0])  # a sample whose group is live and has a masked entry
    act = d["actions"].copy()
    act[b, 0, 0] = int(np.flatnonzero(~m[b])[0])
    d = dict(d, actions=act)
    ref, f32 = oracle_head(d, nvec, gates), torch_head(d, nvec, gates, torch.float32)
    got = kernel_head(d, nvec, gates)
    assert float(got["logp"][b]) <= -3e38 and float(ref["logp"][b]) <= -3e38 and float(f32["logp"][b]) <= -3e38
    assert torch.isfinite(got["logp"]).all() and torch.isfinite(got["d_logits"]).all()
    keep = torch.arange(B) != b  # sample b's log-prob is finfo.min in every implementation: compare the others
    sub = lambda t: {q: (v[keep] if q == "logp" else v) for q, v in t.items()}
    got_cpu = {q: v.cpu() for q, v in got.items()}
    check_ratios(f"{name} masked action of sample {b}", sub(got_cpu), sub(ref), sub(f32))
    assert_masked_gradients_are_zero(d, nvec, got["d_logits"])


@gpu
def test_kernels_are_deterministic():
    name = "w1-w70-C130"
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, "unit")
    one, two = kernel_head(d, nvec, gates), kernel_head(d, nvec, gates)
    for q in QUANTITIES:
        assert torch.equal(one[q], two[q]), q
    z, m, _ = device_inputs(d)
    (a1, l1), (a2, l2) = kernel_sample(z, m, nvec, gates, 11, 3), kernel_sample(z, m, nvec, gates, 11, 3)
    assert torch.equal(a1, a2) and torch.equal(l1, l2)


@gpu
def test_limits_are_reported():
    L, U = _lib.lib(), _lib.RAI_E_UNSUPPORTED
    nv = lambda nvec: (C.c_int32 * len(nvec))(*nvec)
    fwd = lambda n: L.rai_gridnet_logp_entropy(None, None, None, 4, 1, len(n), nv(n), None, None, None, None, None)
    bwd = lambda n: L.rai_gridnet_backward(None, None, None, 4, 1, len(n), nv(n), None, None, None, None, None, None)
    smp = lambda n: L.rai_gridnet_sample(None, None, 4, 1, len(n), nv(n), None, None, 1, 0, None, None, None)
    for f in (fwd, bwd, smp):
        assert f([64] * 4 + [1]) == U  # A = 257
        assert f([2] * 9) == U  # G = 9
        assert f([3, 0]) == _lib.RAI_E_SHAPE
        assert f([64] * 4) == _lib.RAI_E_NULLPTR and f([32] * 8) == _lib.RAI_E_NULLPTR  # at the limits: looked at


# ---- sampler -------------------------------------------------------------------------------------------------------

def sampler_rows(nvec, gates, R=4000, Cc=3):
    """R rows of the same 3 cells: plane 0 always live, the widest plane of cell 1 all masked, cell 0's gate
    reference planes fully valid."""
    rng = np.random.default_rng(7 + len(nvec))
    A, off, wide = sum(nvec), offsets(nvec), int(np.argmax(nvec[1:])) + 1
    logits = (1.5 * rng.standard_normal((Cc, A))).astype(np.float32)
    masks = rng.random((Cc, A)) < 0.6
    masks[:, off[0]] = True
    for r, _ in gates.values():
        masks[0, off[r]:off[r + 1]] = True
    masks[1, off[wide]:off[wide + 1]] = False
    d = dict(logits=np.broadcast_to(logits, (R, Cc, A)).copy(), masks=np.broadcast_to(masks, (R, Cc, A)).copy(),
             w_logp=np.ones(R, np.float32), w_ent=np.zeros(R, np.float32))
    return logits, masks, wide, d


@gpu
@pytest.mark.parametrize("nvec,gates", [W70, A256], ids=["w1-w70", "A256"])
def test_sampler_frequencies_masks_keys_and_logp(nvec, gates):
    R, Cc = 4000, 3
    logits, masks, wide, d = sampler_rows(nvec, gates, R, Cc)
    off = offsets(nvec)
    z, m = torch.tensor(d["logits"]).to(DEV), torch.tensor(d["masks"]).to(DEV).view(torch.uint8)
    act, logp = kernel_sample(z, m, nvec, gates, 1234, 7)
    a = act.cpu().numpy()
    worst = 0.0
    assert not masks[1, off[wide]:off[wide + 1]].any() and nvec[wide] == max(nvec)
    for c in range(Cc):
        for g, n in enumerate(nvec):
            assert ((a[:, c, g] >= 0) & (a[:, c, g] < n)).all()
            lg, mk = logits[c, off[g]:off[g + 1]].astype(np.float64), masks[c, off[g]:off[g + 1]]
            counts = np.bincount(a[:, c, g], minlength=n)
            if mk.any():
                p = np.where(mk, np.exp(lg - lg[mk].max()), 0.0)
                p /= p.sum()
                assert (counts[~mk] == 0).all(), f"a masked action was drawn (cell {c}, plane {g})"
            else:
                p = np.full(n, 1.0 / n)  # torch's equal finfo.min logits: uniform over all n
            tol = 5 * np.sqrt(p * (1 - p) / R) + 1.0 / R
            dev = np.abs(counts / R - p)
            worst = max(worst, float((dev / tol).max()))
            assert (dev <= tol).all(), (c, g, counts.tolist(), (R * p).tolist())
    print(f"gridnet sampler {nvec}: worst |freq - p| / (5 sigma + 1/R) = {worst:.3f}")
    # the log-prob of the drawn actions, gated by the drawn reference plane: both gate states occur
    for g, (r, v) in gates.items():
        assert 0 < (a[:, :, r] == v).sum() < R * Cc
    d = dict(d, actions=a)
    ref, f32 = torch_head(d, nvec, gates, torch.float64), torch_head(d, nvec, gates, torch.float32)
    lp_fwd, _ = kernel_forward(z, m, act, nvec, gates)
    check_ratios(f"sampler {nvec} returned logp", dict(logp=logp), ref, f32, ("logp",))
    check_ratios(f"sampler {nvec} rai_gridnet_logp_entropy of the draw", dict(logp=lp_fwd), ref, f32, ("logp",))
    act2, logp2 = kernel_sample(z, m, nvec, gates, 1234, 7)
    assert torch.equal(act, act2) and torch.equal(logp, logp2)
    act3, _ = kernel_sample(z, m, nvec, gates, 1234, 8)
    assert not torch.equal(act, act3)


@gpu
@pytest.mark.parametrize("name", ["rts-C65", "w1-w70-C130", "A256-C70", "flat-A256"])
def test_sampler_writes_every_action_in_range(name):
    """Tile remainders (C = 65, 130, 70): every (b, c, g) of the -1-filled buffer is written with a value in range,
    masked values only where a plane has none valid, and the log-prob is that of the draw."""
    B, Cc, nvec, gates = CASES[name]
    B = min(B, 2)
    d0 = make_case(name, "unit")
    d = {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in d0.items()}
    off = offsets(nvec)
    z, m, _ = device_inputs(d)
    act, logp = kernel_sample(z, m, nvec, gates, 5, 11)
    a, mk = act.cpu().numpy(), d["masks"]
    for g, n in enumerate(nvec):
        assert ((a[..., g] >= 0) & (a[..., g] < n)).all(), g
        mg = mk[..., off[g]:off[g + 1]]
        picked = np.take_along_axis(mg, a[..., g:g + 1], -1)[..., 0]
        assert picked[mg.any(-1)].all(), f"a masked action was drawn (plane {g})"
    d = dict(d, actions=a)
    ref, f32 = oracle_head(d, nvec, gates), torch_head(d, nvec, gates, torch.float32)
    check_ratios(f"sampler {name} logp", dict(logp=logp), ref, f32, ("logp",))


# ---- through the Python wrappers at A = 256 ------------------------------------------------------------------------

@gpu
def test_distribution_at_max_action_planes():
    from rl_algo_impls_amd.gridnet import GridnetDistribution, ValueDependentMask

    name = "A256-C70"
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, "unit")
    ref, f32 = references(name, "unit")
    sub = {g: ValueDependentMask(r, v) for g, (r, v) in gates.items()}
    lg = torch.tensor(d["logits"]).to(DEV).requires_grad_()
    masks = torch.tensor(d["masks"]).to(DEV)
    pi = GridnetDistribution(Cc, np.asarray(nvec), lg, masks, subaction_mask=sub)
    logp = pi.log_prob(torch.tensor(d["actions"]).to(DEV))
    ent = pi.entropy()
    (torch.tensor(d["w_logp"]).to(DEV) * logp + torch.tensor(d["w_ent"]).to(DEV) * ent).sum().backward()
    check_ratios(f"GridnetDistribution {name}", dict(logp=logp.detach(), entropy=ent.detach(), d_logits=lg.grad), ref,
                 f32)
    ent_only = GridnetDistribution(Cc, np.asarray(nvec), lg.detach(), masks, subaction_mask=sub).entropy()
    assert torch.equal(ent_only, ent.detach())
    a, lp = pi.sample_with_logp(seed=3, offset=1)
    assert tuple(a.shape) == (B, Cc, len(nvec)) and bool(((a >= 0) & (a < 64)).all())
    d2 = dict(d, actions=a.cpu().numpy())
    check_ratios(f"GridnetDistribution {name} sample_with_logp", dict(logp=lp), oracle_head(d2, nvec, gates),
                 torch_head(d2, nvec, gates, torch.float32), ("logp",))


@gpu
def test_flat_categorical_fallback_at_256_logits():
    """policy.py's call of the operator for a flat head the fused head does not take: one cell, one plane."""
    from rl_algo_impls_amd.gridnet import GridnetLogpEntropy, multidiscrete_spec

    name = "flat-A256"
    B, Cc, nvec, gates = CASES[name]
    d = make_case(name, "large")
    ref, f32 = references(name, "large")
    A, G = sum(nvec), len(nvec)
    logits = torch.tensor(d["logits"]).to(DEV).reshape(B, A).requires_grad_()
    masks = torch.tensor(d["masks"]).to(DEV).reshape(B, A)
    actions = torch.tensor(d["actions"]).to(DEV).reshape(B, G)
    logp, ent = GridnetLogpEntropy.apply(logits.reshape(B, 1, A), masks.reshape(B, 1, A),
                                         actions.long().reshape(B, 1, G), multidiscrete_spec(nvec))
    (torch.tensor(d["w_logp"]).to(DEV) * logp + torch.tensor(d["w_ent"]).to(DEV) * ent).sum().backward()
    got = dict(logp=logp.detach(), entropy=ent.detach(), d_logits=logits.grad.reshape(B, 1, A))
    check_ratios(f"GridnetLogpEntropy.apply {name}", got, ref, f32)


# ---- rai_gridnet_num_actions ---------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("out_bytes", [4, 8], ids=["int32", "int64"])
@pytest.mark.parametrize("mode", ["cells", "groups", "gated"])
@pytest.mark.parametrize("B,Cc,nvec,gates", [(5, 3, [3, 4], {1: (0, 1)}), (4, 257, RTS, RTS_GATE)],
                         ids=["odd-rows", "C257"])
def test_num_actions_on_unaligned_rows_and_past_the_tile(B, Cc, nvec, gates, mode, out_bytes):
    """C*A = 21: rows start at odd addresses (byte loads); C = 257: one cell past the 256-cell tile.  `cells`
    counts cells with any valid action, `groups` valid groups, `gated` valid groups whose gate is open."""
    rng = np.random.default_rng(B * Cc)
    A, G, off = sum(nvec), len(nvec), offsets(nvec)
    masks = rng.random((B, Cc, A)) < 0.3
    masks.reshape(B * Cc, A)[rng.random(B * Cc) < 0.3] = False
    actions = np.stack([rng.integers(0, n, (B, Cc)) for n in nvec], -1).astype(np.int64)
    ref_arr, val_arr = gate_arrays(nvec, gates)
    if mode == "cells":
        want = O.num_actions(None, masks)
        nv, sr, sv, g_launch = (C.c_int32 * 1)(A), None, None, 1
    else:
        want = O.num_actions(actions, masks, np.asarray(nvec), ref_arr if mode == "gated" else np.full(G, -1), val_arr)
        nv, sr, sv = spec_ptrs(nvec, gates if mode == "gated" else None)
        g_launch = G
    assert (A * Cc) % 4 != 0
    m = torch.tensor(masks).to(DEV).contiguous().view(torch.uint8)
    a = torch.tensor(actions).to(DEV) if mode == "gated" else None
    out = torch.full((B,), -1, dtype=torch.int32 if out_bytes == 4 else torch.int64, device=DEV)
    _lib.check(_lib.lib().rai_gridnet_num_actions(m.data_ptr(), _lib.ptr(a), B, Cc, g_launch, nv, sr, sv,
                                                  int(mode != "cells"), out_bytes, out.data_ptr(),
                                                  _lib.stream_handle(DEV)), "rai_gridnet_num_actions")
    assert np.array_equal(out.cpu().numpy().astype(np.int64), np.asarray(want).astype(np.int64)), (out, want)
    assert 0 < int(np.asarray(want).sum())
