"""The CNN policies' head and epilogue kernels against float64: csrc/heads.hip
(rai_categorical_critic_heads_fwd / _bwd / _bwd_relu) and the epilogues of csrc/se_block.hip
(rai_bias_relu_fwd / _bwd, rai_bias_relu_fwd_nchw / _bwd_nchw, rai_bias_gelu_fwd / _bwd,
rai_se_residual_fwd / _bwd).

The C entry points are called directly with raw pointers, on NaN-filled outputs.  The reference is
tests/cnn_epilogue_ref.py (plain torch, written from include/rai_amd.h), run in float64 on the CPU;
test_heads_reference_matches_the_modules validates it against CategoricalActorHead / CriticHead before it
judges a kernel.  The harness (check, shifted, carve, guarded_workspace / assert_guards, bits) is
test_gpu_wide_kernels.py's.

Tolerance, per tensor:

    bound = max(1e-5 * max|ref64|, 4 * max|torch_f32 - ref64|)

where torch_f32 is the same reference code run in float32 on the device, never the kernel.  An accumulate
call is judged on got - prefill (the prefill random, different per element) with 2^-23 * max|prefill|
added to the bound for the one rounding of the add.  Pure selections (rai_bias_relu_fwd, the dx of both
ReLU backwards, the NCHW forward) are held bit-exact against torch on the device.

The cases (the tables below; test_case_tables_cover_the_required_paths asserts what they must cover):

    heads       every A in {2..10, 12} at (B, D) = (37, 100); at A = 6 and 12: D in {5, 64, 100, 512, 516}
                at B = 37, B in {1, 3, 5, 257, 300} at D = 100, B in {1, 300} x D in {5, 516}; logits O(1)
                and, at (37, 100) and (300, 516), logits N(0, 40^2) (their largest exceed log(FLT_MAX), so
                exp without the max subtraction overflows); one case with parameters, gradients, enc and
                d_enc one float into their allocations.  Every case runs HEADS_RUNS: fwd, bwd and bwd_relu
                (enc a ReLU output with dead units) with accumulate 0 and 1, on an exactly sized workspace
                between guard bytes, twice (the same bits).
    bias_relu   C = 1024 (one row lane): rows 8 k for k = 1..9 (k workgroups), 4100 (the 512 cap's arm:
                456 workgroups of 9 rows) and 4603 (the cap's arm ending in 512 workgroups, a ragged last
                one); C = 16 (64 row lanes): rows 3 and 1000.  db written, accumulated, written again on
                one workspace zeroed once; db and b one float into their allocations.
    nchw        (B, HW, C) of NCHW_CASES, HW = 1 among them, each with aligned dy / y (the float4 form)
                and with dy / y one float into their allocations (the scalar form): the same bits.
    bias_gelu   (rows, C) in {(1, 4), (37, 32), (300, 96), (1029, 128)}, inputs 3 * randn with the first
                elements forced to +-12, +-8, +-5, +-1, +-0 before and after the bias; b one float off.
    se_residual (B, C, HW) of SE_CASES, the same inputs.
    grid-stride C = 16 and 1,048,580 rows (16 float4s past the 16,384 x 256 cap) for rai_bias_relu_fwd,
                rai_bias_gelu_fwd / _bwd and rai_se_residual_fwd, whole outputs compared.

Measured on an MI355X, worst err / bound per part (test_report_worst_ratios prints them):
heads fwd 0.244, heads bwd 0.297, heads bwd_relu 0.184, bias_relu db 0.018, nchw db 0.011, bias_gelu 0.030,
se_residual 0.250.  The selections are bit-exact, the float4 and scalar NCHW forms bit-equal (HW = 1 included),
and every repeated call gives the same bits.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import pytest
import torch

import cnn_epilogue_ref as R
from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.policy import CategoricalActorHead, CriticHead
from test_gpu_wide_kernels import (DEV, F32, F64, NAN, assert_guards, bits, carve, check, guarded_workspace,
                                   shifted)

WORST = {"heads_fwd": 0.0, "heads_bwd": 0.0, "heads_bwd_relu": 0.0, "bias_relu_db": 0.0, "nchw_db": 0.0,
         "bias_gelu": 0.0, "se_residual": 0.0}

# ---------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------
HEADS_AS = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12)  # the instantiations of heads.hip
O1, LARGE = 1.0, 40.0  # the standard deviation of the logits
LOG_FLT_MAX = 88.72
RAI_OK = 0
HCase = namedtuple("HCase", "A B D scale shift", defaults=(O1, 0))
# (entry point, accumulate) run by every heads case
HEADS_RUNS = (("fwd", None), ("bwd", 0), ("bwd", 1), ("bwd_relu", 0), ("bwd_relu", 1))
HEADS_CASES = [HCase(A, 37, 100) for A in HEADS_AS]
for _A in (6, 12):
    HEADS_CASES += [HCase(_A, 37, D) for D in (5, 64, 512, 516)]  # < 64 columns, one wave, the batched-load
    #                                      limit, the strided D > 512 branch with a ragged last column block
    HEADS_CASES += [HCase(_A, B, 100) for B in (1, 3, 5, 257, 300)]  # < 16 / 32 row lanes, a partial last
    #                                      workgroup, just past 8 rows per lane, a ragged tail
    HEADS_CASES += [HCase(_A, B, D) for B in (1, 300) for D in (5, 516)]
HEADS_CASES += [HCase(6, 37, 100, LARGE), HCase(12, 37, 100, LARGE), HCase(12, 300, 516, LARGE),
                HCase(6, 37, 100, O1, 1)]

BR_CASES = [(8 * k, 1024) for k in range(1, 10)] + [(4100, 1024), (4603, 1024), (3, 16), (1000, 16)]
BR_THREADS, BR_ROWS_PER_LANE, BR_MAX_BLOCKS, BR_CTR_BYTES = 256, 8, 512, 576  # se_block.hip's constants

NCHW_FORMS = (("float4", 0), ("scalar", 1))  # (form, floats dy / y start into their allocation)
NCHW_CASES = [(5, 1, 8), (3, 1, 64), (3, 1, 128), (700, 1, 32), (4, 2, 16), (5, 9, 8), (2, 63, 128), (600, 10, 32)]
BRT_MAX_ELEMS = 8192

GELU_CASES = [(1, 4), (37, 32), (300, 96), (1029, 128)]
# one channel group and one row on 64 row groups; an odd HW; 1024 channels; HW below the 8 row groups; many
# rows per group with a ragged tail; exactly one row per row group
SE_CASES = [(1, 4, 1), (3, 16, 70), (2, 1024, 3), (5, 128, 1), (4, 32, 257), (2, 64, 16)]
EW_CAP_F4 = 16384 * 256  # float4s one trip of the grid-stride kernels covers
BIG_ROWS, BIG_C, BIG_B = 1_048_580, 16, 5


def hid(c) -> str:
    return f"A{c.A}-B{c.B}-D{c.D}" + ("-large" if c.scale != O1 else "") + ("-shift" if c.shift else "")


def br_workgroups(rows, C):
    """(workgroups, whether the cap's arm was taken) of rai_bias_relu_bwd: about BR_ROWS_PER_LANE rows per
    row lane, at most BR_MAX_BLOCKS workgroups, equal runs of rows."""
    per = BR_ROWS_PER_LANE * (BR_THREADS // (C // 4))
    blocks = max(1, -(-rows // per))
    capped = blocks > BR_MAX_BLOCKS
    blocks = min(blocks, BR_MAX_BLOCKS)
    rpb = -(-rows // blocks)
    return -(-rows // rpb), capped


def heads_inputs(c):
    return R.make_heads_inputs(c.B, c.D, c.A, c.scale, seed=100000 * c.A + 100 * c.B + c.D)


# ---------------------------------------------------------------------------------------------------
# 0. CPU: the tables, the reference against the project's modules, the large logit scale
# ---------------------------------------------------------------------------------------------------
def test_case_tables_cover_the_required_paths():
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in HEADS_CASES)
    # every A instantiation for each of the three entry points, written and accumulated
    assert {c.A for c in HEADS_CASES} == set(HEADS_AS) and all(has(A=A, B=37, D=100) for A in HEADS_AS)
    assert {e for e, _ in HEADS_RUNS} == {"fwd", "bwd", "bwd_relu"}
    assert all((e, a) in HEADS_RUNS for e in ("bwd", "bwd_relu") for a in (0, 1))
    for A in (6, 12):
        assert all(has(A=A, B=37, D=D) for D in (5, 64, 100, 512, 516))  # both sides of 512
        assert all(has(A=A, B=B, D=100) for B in (1, 3, 5, 37, 257, 300))
        assert all(has(A=A, B=B, D=D) for B in (1, 300) for D in (5, 516))
        assert has(A=A, scale=LARGE)
    assert any(c.D % 8 and c.D > 512 for c in HEADS_CASES) and any(c.D % 8 and c.D < 512 for c in HEADS_CASES)
    assert has(shift=1)
    assert len({hid(c) for c in HEADS_CASES}) == len(HEADS_CASES)
    # rai_bias_relu_bwd: every workgroup count from 1 to 9, the cap's arm, 512 workgroups, 64 row lanes
    counts = [br_workgroups(r, C) for r, C in BR_CASES]
    assert set(range(1, 10)) <= {n for n, _ in counts}
    assert (BR_MAX_BLOCKS, True) in counts and any(capped and n < BR_MAX_BLOCKS for n, capped in counts)
    assert br_workgroups(3, 16) == (1, False) and br_workgroups(1000, 16) == (2, False)
    # the NCHW pair: HW = 1 in both forms, the LDS limit, several samples per workgroup
    assert {f for f, _ in NCHW_FORMS} == {"float4", "scalar"} and dict(NCHW_FORMS) == {"float4": 0, "scalar": 1}
    assert sum(HW == 1 for _, HW, _ in NCHW_CASES) == 4 and (3, 1, 128) in NCHW_CASES
    assert any(HW == 1 and B > BR_MAX_BLOCKS for B, HW, _ in NCHW_CASES)
    assert any(HW > 1 and B > BR_MAX_BLOCKS for B, HW, _ in NCHW_CASES)
    assert all((C + 1) * HW <= BRT_MAX_ELEMS for _, HW, C in NCHW_CASES)
    assert max((C + 1) * HW for _, HW, C in NCHW_CASES) == 129 * 63 and 129 * 64 > BRT_MAX_ELEMS
    # the SE backward's row groups (256 / (C / 4)) against HW
    groups = lambda C: 256 // (C // 4)
    assert any(HW < groups(C) for _, C, HW in SE_CASES) and any(HW == groups(C) for _, C, HW in SE_CASES)
    assert any(HW > 4 * groups(C) and HW % groups(C) for _, C, HW in SE_CASES)
    assert any(groups(C) == 1 for _, C, _ in SE_CASES)
    # the grid-stride loops take a second trip, for a few elements only
    assert 0 < BIG_ROWS * BIG_C // 4 - EW_CAP_F4 <= 256 and BIG_ROWS % BIG_B == 0


@pytest.mark.parametrize("A,B,D,scale", [(6, 9, 20, O1), (12, 7, 33, O1), (2, 5, 8, LARGE)])
def test_heads_reference_matches_the_modules(A, B, D, scale):
    """run_heads in float64 against CategoricalActorHead / CriticHead cast to .double() on the CPU, given the
    reference's parameters: outputs and autograd gradients to 1e-12 of each tensor's scale."""
    inp = R.make_heads_inputs(B, D, A, scale, seed=7 * A + B)
    pi, vf = CategoricalActorHead(A, D, (), torch.nn.ReLU).double(), CriticHead(D, (), torch.nn.ReLU).double()
    params = list(pi.parameters()) + list(vf.parameters())
    assert [tuple(p.shape) for p in params] == [(A, D), (A,), (1, D), (1,)]
    with torch.no_grad():
        for p, src in zip(params, (inp.wpi, inp.bpi, inp.wv, inp.bv)):
            p.copy_(src.double().reshape(p.shape))
    for relu in (False, True):
        ref = R.run_heads(inp, F64, relu=relu)
        enc = (torch.relu(inp.enc) if relu else inp.enc).double().requires_grad_(True)
        logits = pi.params(enc)
        logp, ent = pi.logp_entropy(logits, inp.actions)
        v = vf(enc)
        d_logp, d_ent, d_v = (t.double() for t in inp.cot)
        grads = torch.autograd.grad((d_logp * logp).sum() + (d_ent * ent).sum() + (d_v * v).sum(), [enc] + params)
        rel = lambda a, b: float((a.detach().reshape(-1) - b.reshape(-1)).abs().max()) / float(b.abs().max())
        for name, a in [("logits", logits), ("logp", logp), ("ent", ent), ("v", v)]:
            assert rel(a, getattr(ref, name)) <= 1e-12, name
        for name, a in zip(("d_enc", "g_wpi", "g_bpi", "g_wv", "g_bv"), grads):
            assert rel(a, getattr(ref, name)) <= 1e-12, name
        if relu:
            dz = torch.where(enc.detach() <= 0, torch.zeros((), dtype=F64), grads[0])
            assert torch.equal(dz == 0, ref.dz == 0) and rel(dz, ref.dz) <= 1e-12
            assert rel(dz.sum(0), ref.g_benc) <= 1e-12
            assert bool((enc == 0).any()) and bool((ref.dz == 0).any())


@pytest.mark.parametrize("c", [c for c in HEADS_CASES if c.scale == LARGE], ids=hid)
def test_float32_reference_stays_finite_at_the_large_logit_scale(c):
    """The large scale's logits pass log(FLT_MAX): exp(logit) overflows in float32, so a kernel without
    the max subtraction gives inf / NaN, while the float32 reference (logsumexp) stays finite."""
    inp = heads_inputs(c)
    ref = R.run_heads(inp, F64)
    assert float(ref.logits.max()) > LOG_FLT_MAX and float(ref.logits.abs().median()) > 10
    assert not bool(torch.isfinite(ref.logits.float().exp()).all())
    for relu in (False, True):
        assert R.run_heads(inp, F32, relu=relu).finite and R.run_heads(inp, F64, relu=relu).finite


# ---------------------------------------------------------------------------------------------------
# device harness
# ---------------------------------------------------------------------------------------------------
def nan(*shape, shift=0):
    return shifted(torch.full(shape, NAN, dtype=F32), shift)


def check_added(name, got, prefill, ref64, t32, part):
    """An accumulate call: got - prefill under the rule, plus 2^-23 * max|prefill| for the add's rounding."""
    got, prefill = got.double().cpu().reshape(-1), prefill.double().cpu().reshape(-1)
    ref64, t32 = ref64.reshape(-1), t32.reshape(-1)
    assert got.shape == ref64.shape == prefill.shape, (name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: not finite"
    bound = max(1e-5 * float(ref64.abs().max()), 4 * float((t32 - ref64).abs().max()))
    bound += 2.0 ** -23 * float(prefill.abs().max())
    err = float((got - prefill - ref64).abs().max())
    ratio = err / bound
    WORST[part] = max(WORST[part], ratio)
    assert err <= bound, f"{name} (accumulate): err {err:.3e} > bound {bound:.3e} (ratio {ratio:.2f})"
    return ratio


def heads_shapes(c, relu):
    return [(c.A, c.D), (c.A,), (c.D,), (1,)] + ([(c.D,)] if relu else [])


GRADS = ("g_wpi", "g_bpi", "g_wv", "g_bv", "g_benc")


class Heads:
    """One heads case on the device: parameters carved from a flat buffer, enc, an exactly sized workspace
    between guard bytes."""

    def __init__(self, c, inp, relu):
        self.c, self.relu = c, relu
        self.pbuf, self.p, _ = carve(heads_shapes(c, False), c.shift, NAN)
        for dst, src in zip(self.p, (inp.wpi, inp.bpi, inp.wv, inp.bv)):
            dst.copy_(src.reshape(dst.shape))
        self.enc = shifted(torch.relu(inp.enc) if relu else inp.enc, c.shift)
        self.act = inp.actions.to(DEV).contiguous()
        self.cot = [t.to(DEV).contiguous() for t in inp.cot]
        self.ws_bytes = int(_lib.lib().rai_categorical_critic_heads_workspace_bytes(c.B, c.A))
        assert self.ws_bytes == c.B * (c.A + 1) * 4
        self.big, self.ws = guarded_workspace(self.ws_bytes)
        self.st = _lib.stream_handle(DEV)

    def inputs(self):
        return [self.enc.data_ptr()] + [t.data_ptr() for t in self.p] + [self.act.data_ptr()]

    def fwd(self):
        c = self.c
        out = [nan(c.B, c.A), nan(c.B), nan(c.B), nan(c.B)]
        rc = _lib.lib().rai_categorical_critic_heads_fwd(*self.inputs(), c.B, c.D, c.A,
                                                         *[t.data_ptr() for t in out], self.st)
        _lib.check(rc, "rai_categorical_critic_heads_fwd")
        return out

    def bwd(self, logits, accumulate, base=None):
        """-> (the gradients' flat buffer, its views, d_enc / dz)."""
        c = self.c
        gbuf, g, P = carve(heads_shapes(c, self.relu), c.shift, NAN)
        if base is not None:
            for dst, src in zip(g, base):
                dst.copy_(src)
        d_enc = nan(c.B, c.D, shift=c.shift)
        args = self.inputs() + [logits.data_ptr(), c.B, c.D, c.A] + [t.data_ptr() for t in self.cot]
        args += [d_enc.data_ptr()] + [t.data_ptr() for t in g]
        args += [accumulate, self.ws.data_ptr(), self.ws_bytes, self.st]
        L = _lib.lib()
        fn = L.rai_categorical_critic_heads_bwd_relu if self.relu else L.rai_categorical_critic_heads_bwd
        _lib.check(fn(*args), "rai_categorical_critic_heads_bwd" + ("_relu" if self.relu else ""))
        torch.cuda.synchronize()
        assert_guards(self.big, self.ws_bytes)
        # nothing outside the views: the shift prefix and the tail keep their NaN
        assert bool(torch.isnan(gbuf[:c.shift]).all()) and bool(torch.isnan(gbuf[c.shift + P:]).all())
        return gbuf, g, d_enc


# ---------------------------------------------------------------------------------------------------
# 1. heads
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("c", HEADS_CASES, ids=hid)
def test_heads_vs_float64(c):
    """HEADS_RUNS of one case: the forward's four outputs (logits_out among them), then each backward
    written and accumulated onto a random prefill; every call repeated once for the same bits.  The
    accumulate call's d_enc / dz (always written) equals the accumulate = 0 call's bit for bit."""
    inp = heads_inputs(c)
    ratios = {}
    for entry in ("bwd", "bwd_relu"):
        relu = entry == "bwd_relu"
        ref, t32 = R.run_heads(inp, F64, relu=relu), R.run_heads(inp, F32, DEV, relu=relu)
        assert ref.finite and t32.finite
        if relu:
            assert bool((ref.dz == 0).any()) or c.B * c.D < 8  # dead units
        h = Heads(c, inp, relu)
        assert ("fwd", None) in HEADS_RUNS
        out = h.fwd()
        for name, got in zip(("logits", "logp", "ent", "v"), out):
            ratios[f"{entry}:{name}"] = check(name, got, getattr(ref, name), getattr(t32, name), "heads_fwd", WORST)
        for a, b in zip(out, h.fwd()):
            assert torch.equal(bits(a), bits(b)), "two forward calls differ"
        part = "heads_" + entry
        names = GRADS if relu else GRADS[:4]
        dname = "dz" if relu else "d_enc"
        first = None
        for acc in [a for e, a in HEADS_RUNS if e == entry]:
            base = None
            if acc:
                gen = torch.Generator().manual_seed(c.A + c.B + c.D)
                base = [torch.randn(s, generator=gen) for s in heads_shapes(c, relu)]
            gbuf, g, d_enc = h.bwd(out[0], acc, base)
            ratios[f"{entry}{acc}:{dname}"] = check(dname, d_enc, getattr(ref, dname), getattr(t32, dname), part, WORST)
            for i, (name, got) in enumerate(zip(names, g)):
                if acc:
                    r = check_added(name, got, base[i], getattr(ref, name), getattr(t32, name), part)
                else:
                    r = check(name, got, getattr(ref, name), getattr(t32, name), part, WORST)
                ratios[f"{entry}{acc}:{name}"] = r
            gbuf2, _, d_enc2 = h.bwd(out[0], acc, base)
            assert torch.equal(bits(gbuf[c.shift:]), bits(gbuf2[c.shift:])), "two backward calls differ"
            assert torch.equal(bits(d_enc), bits(d_enc2))
            if first is None:
                first = d_enc
            else:
                assert torch.equal(bits(d_enc), bits(first)), "accumulate changed d_enc"
    worst = max(ratios, key=ratios.get)
    print(f"\nheads {hid(c)}: worst err/bound {ratios[worst]:.3f} ({worst})")


@pytest.mark.gpu
def test_heads_return_codes_before_any_write():
    """A outside {2..10, 12} and D = 0: RAI_E_SHAPE; a workspace one byte short: RAI_E_WORKSPACE; a NULL
    argument: RAI_E_NULLPTR; each with the NaN-filled outputs untouched.  B = 0: RAI_OK, and what
    include/rai_amd.h says of the gradients: rai_categorical_critic_heads_bwd writes nothing (accumulate 0
    or 1), _bwd_relu zeroes g_benc alone when it does not accumulate."""
    L = _lib.lib()
    c = HCase(6, 4, 8)
    inp = heads_inputs(c)
    for relu in (False, True):
        h = Heads(c, inp, relu)
        logits = h.fwd()[0]
        fn = L.rai_categorical_critic_heads_bwd_relu if relu else L.rai_categorical_critic_heads_bwd
        outs = [nan(c.B, c.A), nan(c.B), nan(c.B), nan(c.B)]
        gbuf, g, _ = carve(heads_shapes(c, relu), 0, NAN)
        d_enc = nan(c.B, c.D)

        def fwd(B=c.B, D=c.D, A=c.A, null=None):
            a = h.inputs() + [B, D, A] + [t.data_ptr() for t in outs] + [h.st]
            if null is not None:
                a[null] = None
            return L.rai_categorical_critic_heads_fwd(*a)

        def bwd(B=c.B, D=c.D, A=c.A, acc=0, nbytes=h.ws_bytes, null=None):
            a = h.inputs() + [logits.data_ptr(), B, D, A] + [t.data_ptr() for t in h.cot] + [d_enc.data_ptr()]
            a += [t.data_ptr() for t in g] + [acc, h.ws.data_ptr(), nbytes, h.st]
            if null is not None:
                a[null] = None
            return fn(*a)

        n_ptr_bwd = 6 + 1 + 3 + 3 + 1 + len(g)  # positions of the pointer arguments before `accumulate`
        for A in (1, 11, 13):
            assert fwd(A=A) == _lib.RAI_E_SHAPE and bwd(A=A) == _lib.RAI_E_SHAPE, A
        assert fwd(D=0) == _lib.RAI_E_SHAPE and bwd(D=0) == _lib.RAI_E_SHAPE
        assert fwd(B=-1) == _lib.RAI_E_SHAPE and bwd(B=-1) == _lib.RAI_E_SHAPE
        assert bwd(nbytes=h.ws_bytes - 1) == _lib.RAI_E_WORKSPACE
        for i in (0, 1, 5, 9, 12):
            assert fwd(null=i) == _lib.RAI_E_NULLPTR, i
        for i in [j for j in range(n_ptr_bwd) if j not in (7, 8, 9)] + [n_ptr_bwd + 1]:
            assert bwd(null=i) == _lib.RAI_E_NULLPTR, i
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs + [gbuf, d_enc])
        # B = 0
        assert fwd(B=0) == RAI_OK
        for acc in (0, 1):
            assert bwd(B=0, acc=acc, nbytes=0) == RAI_OK
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in outs + g[:4] + [d_enc])
            if relu:
                assert bool((g[4] == 0).all()) if acc == 0 else bool(torch.isnan(g[4]).all())
                g[4].fill_(NAN)
        assert_guards(h.big, h.ws_bytes)


# ---------------------------------------------------------------------------------------------------
# 2. bias + ReLU
# ---------------------------------------------------------------------------------------------------
def one_off(C, src=None):
    """A (C) view one float into a NaN-filled allocation (4-byte aligned only) -> (allocation, view)."""
    buf = torch.full((C + 9,), NAN, dtype=F32, device=DEV)
    view = buf[1:1 + C]
    if src is not None:
        view.copy_(src)
    assert view.data_ptr() % 16 == 4
    return buf, view


def untouched_around(buf, C):
    return bool(torch.isnan(buf[:1]).all()) and bool(torch.isnan(buf[1 + C:]).all())


def br_workspace(C):
    n = int(_lib.lib().rai_bias_relu_workspace_bytes(C))
    assert n == BR_MAX_BLOCKS * C * 4 + BR_CTR_BYTES
    return (n,) + guarded_workspace(n, fill=0)


def counters_are_zero(ws):
    return bool((ws[-BR_CTR_BYTES:].view(torch.int32) == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", BR_CASES)
def test_bias_relu_vs_float64(rows, C):
    g = torch.Generator().manual_seed(rows * 31 + C)
    x, b, dy = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), torch.randn(rows, C, generator=g)
    base = torch.randn(C, generator=g)
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    _, bd = one_off(C, b)
    y = nan(rows, C)
    _lib.check(L.rai_bias_relu_fwd(xd.data_ptr(), bd.data_ptr(), rows, C, y.data_ptr(), st), "rai_bias_relu_fwd")
    assert torch.equal(y, R.bias_relu_fwd(xd, bd))
    dx32, db32 = R.bias_relu_bwd(dyd, y)
    _, db64 = R.bias_relu_bwd(dy.double(), y.cpu().double())
    nbytes, big, ws = br_workspace(C)
    dbs, ratios = [], []
    for acc in (0, 1, 0):  # written, accumulated, written again: one workspace, zeroed once
        dx = nan(rows, C)
        dbuf, db = one_off(C, base if acc else None)
        _lib.check(L.rai_bias_relu_bwd(dyd.data_ptr(), y.data_ptr(), rows, C, dx.data_ptr(), db.data_ptr(), acc,
                                       ws.data_ptr(), nbytes, st), "rai_bias_relu_bwd")
        assert torch.equal(dx, dx32)
        if acc:
            ratios.append(check_added("db", db, base, db64, db32.double().cpu(), "bias_relu_db"))
        else:
            ratios.append(check("db", db, db64, db32.double().cpu(), "bias_relu_db", WORST))
        assert untouched_around(dbuf, C)
        assert counters_are_zero(ws), "the arrival counters were not re-armed"
        dbs.append(db)
    assert torch.equal(bits(dbs[0]), bits(dbs[2]))
    assert_guards(big, nbytes)
    print(f"\nbias_relu rows={rows} C={C} ({br_workgroups(rows, C)[0]} workgroups): db err/bound {max(ratios):.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,HW,C", NCHW_CASES)
def test_bias_relu_nchw_vs_float64(B, HW, C):
    """Both forms of rai_bias_relu_bwd_nchw on the output of rai_bias_relu_fwd_nchw: dy and y aligned (the
    float4 form) and really one float into their allocations (the scalar form, no environment switch)."""
    g = torch.Generator().manual_seed(B * 131 + HW * 17 + C)
    x, b = torch.randn(B, HW, C, generator=g), torch.randn(C, generator=g)
    dy, base = torch.randn(B, C * HW, generator=g), torch.randn(C, generator=g)
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd = x.to(DEV)
    _, bd = one_off(C, b)
    nbytes, big, ws = br_workspace(C)
    res, ratios = {}, []
    for form, shift in NCHW_FORMS:
        y, dyd = nan(B, C * HW, shift=shift), shifted(dy, shift)
        assert all((t.data_ptr() % 16 == 0) == (form == "float4") for t in (y, dyd))
        _lib.check(L.rai_bias_relu_fwd_nchw(xd.data_ptr(), bd.data_ptr(), B, HW, C, y.data_ptr(), st), "fwd_nchw")
        assert torch.equal(y, R.bias_relu_fwd_nchw(xd, bd))
        dx32, db32 = R.bias_relu_bwd_nchw(dyd, y, HW, C)
        _, db64 = R.bias_relu_bwd_nchw(dy.double(), y.cpu().double(), HW, C)
        for acc in (0, 1):
            dx = nan(B, HW, C)
            dbuf, db = one_off(C, base if acc else None)
            _lib.check(L.rai_bias_relu_bwd_nchw(dyd.data_ptr(), y.data_ptr(), B, HW, C, dx.data_ptr(), db.data_ptr(),
                                                acc, ws.data_ptr(), nbytes, st), "rai_bias_relu_bwd_nchw")
            assert torch.equal(dx, dx32), f"{form}: dx is not threshold_backward in NHWC"
            if acc:
                ratios.append(check_added("db", db, base, db64, db32.double().cpu(), "nchw_db"))
            else:
                ratios.append(check("db", db, db64, db32.double().cpu(), "nchw_db", WORST))
            assert untouched_around(dbuf, C) and counters_are_zero(ws)
            res[form, acc] = (dx, db)
    for acc in (0, 1):
        for a, b_ in zip(res["float4", acc], res["scalar", acc]):
            assert torch.equal(bits(a), bits(b_)), "the float4 and the scalar form differ"
    assert_guards(big, nbytes)
    print(f"\nnchw B={B} HW={HW} C={C}: db err/bound {max(ratios):.3f}")


@pytest.mark.gpu
def test_bias_relu_return_codes():
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    t = torch.full((1 << 16,), NAN, dtype=F32, device=DEV)
    p = t.data_ptr()
    nbytes, big, ws = br_workspace(128)
    w = ws.data_ptr()
    for C in (6, 24, 2, 2048):
        assert L.rai_bias_relu_fwd(p, p, 4, C, p, st) == _lib.RAI_E_SHAPE, C
        assert L.rai_bias_relu_bwd(p, p, 4, C, p, p, 0, w, 1 << 30, st) == _lib.RAI_E_SHAPE, C
        assert L.rai_bias_relu_fwd_nchw(p, p, 4, 2, C, p, st) == _lib.RAI_E_SHAPE, C
        assert L.rai_bias_relu_bwd_nchw(p, p, 4, 2, C, p, p, 0, w, 1 << 30, st) == _lib.RAI_E_SHAPE, C
    # (C + 1) * HW = 129 * 64 floats do not fit the LDS plane
    assert L.rai_bias_relu_fwd_nchw(p, p, 1, 64, 128, p, st) == _lib.RAI_E_SHAPE
    assert L.rai_bias_relu_bwd_nchw(p, p, 1, 64, 128, p, p, 0, w, nbytes, st) == _lib.RAI_E_SHAPE
    assert L.rai_bias_relu_fwd(None, p, 4, 128, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_fwd(p, p, 4, 128, None, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_fwd_nchw(p, None, 4, 2, 128, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_bwd(p, None, 4, 128, p, p, 0, w, nbytes, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_bwd(p, p, 4, 128, p, None, 0, w, nbytes, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_bwd_nchw(None, p, 4, 2, 128, p, p, 0, w, nbytes, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_bwd_nchw(p, p, 4, 2, 128, p, p, 0, None, nbytes, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_relu_bwd(p, p, 4, 128, p, p, 0, w, nbytes - 1, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_bias_relu_bwd_nchw(p, p, 4, 2, 128, p, p, 0, w, nbytes - 1, st) == _lib.RAI_E_WORKSPACE
    assert L.rai_bias_relu_bwd_nchw(p, p, 4, 2, 128, p + 4, p, 0, w, nbytes, st) == _lib.RAI_E_WORKSPACE  # dx
    assert L.rai_bias_relu_fwd(p, p, 0, 128, p, st) == RAI_OK
    assert L.rai_bias_relu_fwd_nchw(p, p, 0, 2, 128, p, st) == RAI_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all()) and bool((ws == 0).all())  # nothing was launched
    assert_guards(big, nbytes)


# ---------------------------------------------------------------------------------------------------
# 3. bias + GELU, SE residual
# ---------------------------------------------------------------------------------------------------
def gelu_inputs(rows, C, seed):
    b = R.eighths(C, torch.Generator().manual_seed(seed + 1))
    x, g = R.tail_inputs((rows, C), b, seed)
    return x, b, torch.randn(rows, C, generator=g)


def run_bias_gelu_kernels(x, b, dy):
    rows, C = x.shape
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    bbuf, bd = one_off(C, b)
    y, dx = nan(rows, C), nan(rows, C)
    _lib.check(L.rai_bias_gelu_fwd(xd.data_ptr(), bd.data_ptr(), rows, C, y.data_ptr(), st), "rai_bias_gelu_fwd")
    _lib.check(L.rai_bias_gelu_bwd(dyd.data_ptr(), xd.data_ptr(), bd.data_ptr(), rows, C, dx.data_ptr(), st),
               "rai_bias_gelu_bwd")
    torch.cuda.synchronize()
    assert untouched_around(bbuf, C)
    return y, dx


@pytest.mark.gpu
@pytest.mark.parametrize("rows,C", GELU_CASES)
def test_bias_gelu_vs_float64(rows, C):
    x, b, dy = gelu_inputs(rows, C, seed=rows * 1000 + C)
    ref, t32 = R.run_bias_gelu(x, b, dy, F64), R.run_bias_gelu(x, b, dy, F32, DEV)
    y, dx = run_bias_gelu_kernels(x, b, dy)
    ry = check("y", y, ref.y, t32.y, "bias_gelu", WORST)
    rdx = check("dx", dx, ref.dx, t32.dx, "bias_gelu", WORST)
    print(f"\nbias_gelu rows={rows} C={C}: err/bound y {ry:.3f} dx {rdx:.3f}")


def se_inputs(B, C, HW, seed):
    """x with its first elements on the GELU's tails, r = 0 under the first few of them (the argument is
    then the tail value itself), s in (0, 1) as a sigmoid's output."""
    x, g = R.tail_inputs((B, HW, C), None, seed)
    r = 3.0 * torch.randn(B, HW, C, generator=g)
    r.view(-1)[:min(len(R.TAILS) // 2, r.numel() // 2)] = 0.0
    s = torch.sigmoid(torch.randn(B, C, generator=g))
    return x, r, s, torch.randn(B, HW, C, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,HW", SE_CASES)
def test_se_residual_vs_float64(B, C, HW):
    x, r, s, dout = se_inputs(B, C, HW, seed=B * 100000 + C * 300 + HW)
    ref, t32 = R.run_se_residual(x, r, s, dout, F64), R.run_se_residual(x, r, s, dout, F32, DEV)
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd, rd, sd, dd = (t.to(DEV) for t in (x, r, s, dout))
    out, dx, dr, ds = nan(B, HW, C), nan(B, HW, C), nan(B, HW, C), nan(B, C)
    _lib.check(L.rai_se_residual_fwd(xd.data_ptr(), rd.data_ptr(), sd.data_ptr(), B, C, HW, out.data_ptr(), st),
               "rai_se_residual_fwd")
    _lib.check(L.rai_se_residual_bwd(dd.data_ptr(), xd.data_ptr(), rd.data_ptr(), sd.data_ptr(), B, C, HW,
                                     dx.data_ptr(), dr.data_ptr(), ds.data_ptr(), st), "rai_se_residual_bwd")
    ratios = {k: check(k, got, getattr(ref, k), getattr(t32, k), "se_residual", WORST)
              for k, got in (("out", out), ("dx", dx), ("dr", dr), ("ds", ds))}
    assert torch.equal(bits(dr), bits(dx * sd.unsqueeze(1))), "dr is not dx * s"
    print(f"\nse_residual B={B} C={C} HW={HW}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@lru_cache(maxsize=1)
def big_inputs():
    """The inputs of the three tests above the grid-stride cap, made once: (BIG_ROWS, BIG_C)."""
    return gelu_inputs(BIG_ROWS, BIG_C, seed=99)


@pytest.mark.gpu
def test_bias_relu_fwd_above_the_grid_stride_cap():
    x, b, _ = big_inputs()
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd, (_, bd), y = x.to(DEV), one_off(BIG_C, b), nan(BIG_ROWS, BIG_C)
    _lib.check(L.rai_bias_relu_fwd(xd.data_ptr(), bd.data_ptr(), BIG_ROWS, BIG_C, y.data_ptr(), st),
               "rai_bias_relu_fwd")
    assert torch.equal(y, R.bias_relu_fwd(xd, bd))


@pytest.mark.gpu
def test_bias_gelu_above_the_grid_stride_cap():
    x, b, dy = big_inputs()
    ref, t32 = R.run_bias_gelu(x, b, dy, F64), R.run_bias_gelu(x, b, dy, F32, DEV)
    y, dx = run_bias_gelu_kernels(x, b, dy)
    ry = check("y", y, ref.y, t32.y, "bias_gelu", WORST)
    rdx = check("dx", dx, ref.dx, t32.dx, "bias_gelu", WORST)
    print(f"\nbias_gelu rows={BIG_ROWS} C={BIG_C}: err/bound y {ry:.3f} dx {rdx:.3f}")


@pytest.mark.gpu
def test_se_residual_fwd_above_the_grid_stride_cap():
    x, _, r = big_inputs()
    B, HW, C = BIG_B, BIG_ROWS // BIG_B, BIG_C
    x, r = x.view(B, HW, C), r.view(B, HW, C)
    s = torch.sigmoid(torch.randn(B, C, generator=torch.Generator().manual_seed(98)))
    ref = R.run_se_residual(x, r, s, None, F64, backward=False)
    t32 = R.run_se_residual(x, r, s, None, F32, DEV, backward=False)
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    xd, rd, sd, out = x.to(DEV), r.to(DEV), s.to(DEV), nan(B, HW, C)
    _lib.check(L.rai_se_residual_fwd(xd.data_ptr(), rd.data_ptr(), sd.data_ptr(), B, C, HW, out.data_ptr(), st),
               "rai_se_residual_fwd")
    ratio = check("out", out, ref.out, t32.out, "se_residual", WORST)
    print(f"\nse_residual_fwd B={B} C={C} HW={HW}: err/bound out {ratio:.3f}")


@pytest.mark.gpu
def test_gelu_and_se_return_codes():
    L, st = _lib.lib(), _lib.stream_handle(DEV)
    t = torch.full((1 << 14,), NAN, dtype=F32, device=DEV)
    p = t.data_ptr()
    for C in (6, 2):
        assert L.rai_bias_gelu_fwd(p, p, 4, C, p, st) == _lib.RAI_E_SHAPE
        assert L.rai_bias_gelu_bwd(p, p, p, 4, C, p, st) == _lib.RAI_E_SHAPE
    for C in (6, 24, 2048):  # 24 / 4 = 6 does not divide 256
        assert L.rai_se_residual_fwd(p, p, p, 2, C, 4, p, st) == _lib.RAI_E_SHAPE, C
        assert L.rai_se_residual_bwd(p, p, p, p, 2, C, 4, p, p, p, st) == _lib.RAI_E_SHAPE, C
    assert L.rai_se_residual_fwd(p, p, p, 2, 16, 0, p, st) == _lib.RAI_E_SHAPE
    assert L.rai_bias_gelu_fwd(None, p, 4, 8, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_gelu_fwd(p, None, 4, 8, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_gelu_bwd(p, p, p, 4, 8, None, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_residual_fwd(p, p, None, 2, 16, 4, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_residual_bwd(p, p, p, p, 2, 16, 4, p, p, None, st) == _lib.RAI_E_NULLPTR
    assert L.rai_se_residual_bwd(None, p, p, p, 2, 16, 4, p, p, p, st) == _lib.RAI_E_NULLPTR
    assert L.rai_bias_gelu_fwd(p, p, 0, 8, p, st) == RAI_OK
    assert L.rai_bias_gelu_bwd(p, p, p, 0, 8, p, st) == RAI_OK
    assert L.rai_se_residual_fwd(p, p, p, 0, 16, 4, p, st) == RAI_OK
    assert L.rai_se_residual_bwd(p, p, p, p, 0, 16, 4, p, p, p, st) == RAI_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(t).all())  # nothing was launched


@pytest.mark.gpu
def test_report_worst_ratios():
    """Runs last: the worst err / bound of every part over this module's cases (see the docstring)."""
    print("\nworst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    assert all(v <= 1.0 for v in WORST.values())
