"""The wide-MLP kernels (csrc/mlp_wide.hip, csrc/mlp_wide_epoch.hip) against a float64 reference.

The C entry points are called directly (no trainer): rai_mlp_wide_forward / _backward /
_dist_params / _forward_loss and rai_mlp_wide_epoch.  The reference is plain torch float64 on the
CPU, written here from include/rai_amd.h's description of the operation (two [in -> H -> H -> out]
MLPs, a Normal or Categorical head); test_reference_matches_actor_critic_module validates it
against the project's ActorCritic module before it judges a kernel.

Tolerance, per tensor (each output, each of the 12 gradient tensors and log_std's):

    bound = max(1e-5 * max|ref64|, 4 * max|torch_f32 - ref64|)

where torch_f32 is the same computation run by torch in float32 on the device (F.linear +
autograd): the margin is measured against the reference library's own float32 error, never
against the kernel under test.  An indexing error, a lost row or a wrong scale is 1e-2 relative
or more.

ReLU cases: act'(h) = h > 0 is discontinuous, so a pre-activation within float32 rounding of zero
may take either side.  Every ReLU case asserts, on the float64 reference alone, that no layer-1 or
layer-2 pre-activation z of either network has |z| < 2^-20 * max|z| of its layer; the seeds in the
case tables were searched on the CPU to satisfy it (with a 4x margin) and are hard-coded.

Measured on an MI355X, worst err / bound over all cases (test_report_worst_ratios prints them):
forward 0.090, backward 0.546, dist_params 0.090, epoch gradient 0.357, epoch stats 0.153.
accumulate = 1 and forward_loss vs forward + rai_ppo_loss are bit-equal.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.envs import Box, Discrete
from rl_algo_impls_amd.pg_common import DeviceBlocks, make_hparams
from rl_algo_impls_amd.policy import ActorCritic

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
NAN = float("nan")
GUARD = 256  # bytes of 0xFF on either side of an exactly-sized workspace
WORST = {"forward": 0.0, "backward": 0.0, "dist_params": 0.0, "epoch_grad": 0.0, "epoch_stats": 0.0}

# head: "g" Gaussian (rai head 1), "c" Categorical (head 0); act: "tanh" (0) / "relu" (1);
# acc: also run accumulate = 1; pshift / oshift: the parameter + gradient layout / the observations
# start one float into their buffers (4-byte but not 16-byte aligned)
Case = namedtuple("Case", "H in_dim out B head act acc pshift oshift seed", defaults=(0, 0, 0, 0))


def cid(c) -> str:
    s = f"H{c.H}-in{c.in_dim}-out{c.out}-B{c.B}-{c.head}-{c.act}"
    if getattr(c, "acc", 0):
        s += "-acc"
    if c.pshift:
        s += "-pshift"
    if getattr(c, "oshift", 0):
        s += "-oshift"
    if getattr(c, "vclip", None) is not None:
        s += f"-vclip{c.vclip}"
    if getattr(c, "ent_coef", None) is not None:
        s += f"-ent{c.ent_coef}"
    if getattr(c, "vf", "mse_loss") != "mse_loss":
        s += "-huber"
    return s


# ---------------------------------------------------------------------------------------------
# the float64 reference (dtype- and device-generic: the float32 device run uses the same code)
# ---------------------------------------------------------------------------------------------
def param_shapes(c):
    """ActorCritic.parameters() order (what FlatParams packs): the Gaussian head's log_std first,
    then the actor's and the critic's W1, b1, W2, b2, W3, b3."""
    net = lambda o: [(c.H, c.in_dim), (c.H,), (c.H, c.H), (c.H,), (o, c.H), (o,)]
    return ([(c.out,)] if c.head == "g" else []) + net(c.out) + net(1)


def split_params(params, c):
    if c.head == "g":
        return params[0], params[1:7], params[7:13]
    return None, params[0:6], params[6:12]


def make_inputs(c):
    """float32 CPU tensors from the case's seed: parameters, observations, actions, cotangents."""
    g = torch.Generator().manual_seed(c.seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    params = []
    if c.head == "g":
        params.append(-0.5 + 0.2 * rn(c.out))
    for o in (c.out, 1):
        params += [rn(c.H, c.in_dim) / math.sqrt(c.in_dim), 0.1 * rn(c.H), rn(c.H, c.H) / math.sqrt(c.H),
                   0.1 * rn(c.H), rn(o, c.H) / math.sqrt(c.H), 0.1 * rn(o)]
    obs = rn(c.B, c.in_dim)
    actions = rn(c.B, c.out) if c.head == "g" else torch.randint(0, c.out, (c.B,), generator=g)
    cot = (rn(c.B), rn(c.B, c.out) if c.head == "g" else rn(c.B), rn(c.B))
    return params, obs, actions, cot


def forward_ref(params, obs, actions, c):
    """h1 = act(x W1^T + b1), h2 = act(h1 W2^T + b2), o = h2 W3^T + b3 for both networks, then the
    head: Normal(mu, exp(log_std)) log-prob summed over dims and per-dimension entropy (B, out), or
    Categorical log_softmax gathered at the action and entropy (B,).  Returns logp, ent, v, the actor
    outputs o and the four layers' pre-activations."""
    log_std, pi, vn = split_params(params, c)
    act = torch.relu if c.act == "relu" else torch.tanh
    zs = []

    def mlp(p):
        z1 = F.linear(obs, p[0], p[1])
        z2 = F.linear(act(z1), p[2], p[3])
        zs.extend([z1, z2])
        return F.linear(act(z2), p[4], p[5])

    o, v = mlp(pi), mlp(vn).squeeze(-1)
    if c.head == "g":
        dist = torch.distributions.Normal(o, log_std.exp())
        logp, ent = dist.log_prob(actions).sum(-1), dist.entropy()
    else:
        ls = F.log_softmax(o, dim=-1)
        logp = ls.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
        ent = -(ls.exp() * ls).sum(-1)
    return logp, ent, v, o, zs


def cast(ts, dtype, device="cpu"):
    return [t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype) for t in ts]


def run_ref(c, params, obs, actions, cot, dtype, device="cpu"):
    """Forward and, by autograd of sum(d_logp logp) + sum(d_ent ent) + sum(d_v v), the gradients."""
    p = [t.requires_grad_(True) for t in cast(params, dtype, device)]
    obs, actions = cast([obs, actions], dtype, device)
    d_logp, d_ent, d_v = cast(cot, dtype, device)
    logp, ent, v, o, zs = forward_ref(p, obs, actions, c)
    grads = torch.autograd.grad((d_logp * logp).sum() + (d_ent * ent).sum() + (d_v * v).sum(), p)
    det = lambda t: t.detach().double().cpu()
    return SimpleNamespace(logp=det(logp), ent=det(ent), v=det(v), o=det(o), zs=[det(z) for z in zs],
                           grads=[det(g_) for g_ in grads])


def relu_margin(zs) -> float:
    """min over the layers of min|z| / max|z|; the ReLU condition is relu_margin >= 2^-20."""
    return min(float(z.abs().min() / z.abs().max()) for z in zs)


def assert_relu_condition(c, zs):
    if c.act == "relu":
        m = relu_margin(zs)
        assert m >= 2.0 ** -20, f"a pre-activation within 2^-20 of zero (margin {m:.3e}): pick another seed"


def check(name, got, ref64, t32, part, worst=None):
    """The tolerance rule; returns err / bound and records the part's worst (in `worst`: another
    module's table; this module's by default)."""
    worst = WORST if worst is None else worst
    got, ref64, t32 = got.double().cpu().reshape(-1), ref64.reshape(-1), t32.reshape(-1)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: an element was not written (NaN pre-fill) or is not finite"
    bound = max(1e-5 * float(ref64.abs().max()), 4 * float((t32 - ref64).abs().max()))
    err = float((got - ref64).abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
    worst[part] = max(worst[part], ratio)
    assert err <= bound, f"{name}: err {err:.3e} > bound {bound:.3e} (ratio {ratio:.2f})"
    return ratio


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------
# device harness
# ---------------------------------------------------------------------------------------------
def carve(shapes, shift, fill, tail=8):
    """One flat float32 buffer holding `shift` floats, the tensors packed back to back (as
    FlatParams does), then `tail` floats; returns (buffer, views, P)."""
    P = sum(int(np.prod(s)) for s in shapes)
    buf = torch.full((shift + P + tail,), fill, dtype=F32, device=DEV)
    views, off = [], shift
    for s in shapes:
        n = int(np.prod(s))
        views.append(buf[off:off + n].view(s))
        off += n
    return buf, views, P


def shifted(t, shift):
    """A contiguous device copy of t that starts `shift` floats into its allocation."""
    if not shift:
        return t.to(DEV).contiguous()
    buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=DEV)
    out = buf[shift:].view(t.shape)
    out.copy_(t)
    return out


def guarded_workspace(nbytes, fill=0xFF):
    big = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    ws = big[GUARD:GUARD + nbytes]
    if fill != 0xFF:
        ws.fill_(fill)
    return big, ws


def assert_guards(big, nbytes):
    assert bool((big[:GUARD] == 0xFF).all()) and bool((big[GUARD + nbytes:] == 0xFF).all()), \
        "bytes outside the workspace were written"


def make_desc(c, pviews, gviews, accumulate=0):
    d = _lib.MlpWideDesc()
    ls, pi, vn = split_params(pviews, c)
    for n, ts in enumerate((pi, vn)):
        for i, t in enumerate(ts):
            d.w[n][i] = t.data_ptr()
    if gviews is not None:
        gls, gpi, gvn = split_params(gviews, c)
        for n, ts in enumerate((gpi, gvn)):
            for i, t in enumerate(ts):
                d.g[n][i] = t.data_ptr()
        if c.head == "g":
            d.g_log_std = gls.data_ptr()
    if c.head == "g":
        d.log_std = ls.data_ptr()
    d.in_dim, d.hidden, d.out_pi = c.in_dim, c.H, c.out
    d.head, d.activation, d.accumulate = int(c.head == "g"), int(c.act == "relu"), accumulate
    return d


class Wide:
    """Parameters, inputs and an exactly-sized guarded workspace of one case on the device."""

    def __init__(self, c, params, obs, actions):
        self.c = c
        self.pbuf, self.p, self.P = carve(param_shapes(c), c.pshift, NAN)
        for dst, src in zip(self.p, params):
            dst.copy_(src)
        self.obs = shifted(obs, getattr(c, "oshift", 0))
        self.actions = actions.to(DEV).contiguous()
        self.ws_bytes = int(_lib.lib().rai_mlp_wide_workspace_bytes(c.B, c.H))
        assert self.ws_bytes > 0
        self.big, self.ws = guarded_workspace(self.ws_bytes)
        self.st = _lib.stream_handle(DEV)

    def outputs(self):
        c = self.c
        nan = lambda *s: torch.full(s, NAN, dtype=F32, device=DEV)
        return nan(c.B), (nan(c.B, c.out) if c.head == "g" else nan(c.B)), nan(c.B)

    def forward(self):
        c = self.c
        logp, ent, v = self.outputs()
        d = make_desc(c, self.p, None)
        rc = _lib.lib().rai_mlp_wide_forward(C.byref(d), self.obs.data_ptr(), self.actions.data_ptr(), c.B,
                                             logp.data_ptr(), ent.data_ptr(), v.data_ptr(), self.ws.data_ptr(),
                                             self.ws_bytes, self.st)
        assert rc == 0, rc
        return logp, ent, v

    def backward(self, cot, accumulate=0, base=None):
        """Gradient views: NaN-filled (accumulate == 0) or `base`; returns (buffer, views)."""
        c = self.c
        gbuf, g, _ = carve(param_shapes(c), c.pshift, NAN)
        if base is not None:
            for dst, src in zip(g, base):
                dst.copy_(src)
        d = make_desc(c, self.p, g, accumulate)
        d_logp, d_ent, d_v = cot
        rc = _lib.lib().rai_mlp_wide_backward(C.byref(d), self.obs.data_ptr(), self.actions.data_ptr(), c.B,
                                              d_logp.data_ptr(), d_ent.data_ptr(), d_v.data_ptr(),
                                              self.ws.data_ptr(), self.ws_bytes, self.st)
        assert rc == 0, rc
        return gbuf, g

    def dist_params(self):
        c = self.c
        po = torch.full((c.B, c.out), NAN, dtype=F32, device=DEV)
        vo = torch.full((c.B,), NAN, dtype=F32, device=DEV)
        d = make_desc(c, self.p, None)
        rc = _lib.lib().rai_mlp_wide_dist_params(C.byref(d), self.obs.data_ptr(), c.B, po.data_ptr(), vo.data_ptr(),
                                                 self.ws.data_ptr(), self.ws_bytes, self.st)
        assert rc == 0, rc
        return po, vo


def grad_names(c):
    net = lambda n: [f"{n}.{k}" for k in ("W1", "b1", "W2", "b2", "W3", "b3")]
    return (["log_std"] if c.head == "g" else []) + net("pi") + net("v")


# ---------------------------------------------------------------------------------------------
# 0. the reference against the project's module (CPU)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [
    Case(64, 5, 3, 7, "g", "tanh", seed=11),
    Case(64, 5, 3, 7, "g", "relu", seed=12),
    Case(64, 3, 4, 9, "c", "tanh", seed=13),
    Case(64, 3, 4, 9, "c", "relu", seed=14),
], ids=cid)
def test_reference_matches_actor_critic_module(c):
    """forward_ref / run_ref in float64 against ActorCritic cast to .double() on the CPU: forward and
    autograd gradients to 1e-12 relative.  The module is given the reference's parameters in
    parameters() order (which also checks param_shapes against the module).  The module's Flatten
    encoder casts observations to float32, so its heads are called as ConnectedTrioNetwork.forward
    calls them, on the float64 observations."""
    params, obs, actions, cot = make_inputs(c)
    env = SimpleNamespace(single_observation_space=Box(-np.inf, np.inf, (c.in_dim,), np.float32),
                          single_action_space=Box(-1.0, 1.0, (c.out,), np.float32) if c.head == "g"
                          else Discrete(c.out))
    pol = ActorCritic(env, pi_hidden_sizes=[c.H, c.H], v_hidden_sizes=[c.H, c.H], activation_fn=c.act).double()
    mp = list(pol.parameters())
    assert [tuple(p.shape) for p in mp] == param_shapes(c)
    with torch.no_grad():
        for p, src in zip(mp, params):
            p.copy_(src.double())
    ref = run_ref(c, params, obs, actions, cot, F64)
    assert_relu_condition(c, ref.zs)
    net = pol.network
    enc = net._feature_extractor.feature_extractor(obs.double())
    logp, ent = net._pi.logp_entropy(net._pi.params(enc), actions.double() if c.head == "g" else actions)
    v = net._v(enc)
    assert ent.shape == ((c.B, c.out) if c.head == "g" else (c.B,))
    d_logp, d_ent, d_v = cast(cot, F64)
    grads = torch.autograd.grad((d_logp * logp).sum() + (d_ent * ent).sum() + (d_v * v).sum(), mp)
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    for name, a, b in [("logp", logp, ref.logp), ("ent", ent, ref.ent), ("v", v, ref.v)]:
        assert rel(a.detach(), b) <= 1e-12, name
    for name, a, b in zip(grad_names(c), grads, ref.grads):
        assert rel(a, b) <= 1e-12, name


# ---------------------------------------------------------------------------------------------
# 1. forward, dist_params and backward against float64
# ---------------------------------------------------------------------------------------------
G, K = "g", "c"
CASES = [
    # every B at H = 256
    Case(256, 17, 6, 1, G, "relu"),
    Case(256, 4, 2, 15, K, "tanh"),
    Case(256, 64, 8, 64, G, "tanh", acc=1),
    Case(256, 3, 8, 65, K, "relu"),
    Case(256, 63, 1, 130, G, "relu", acc=1),
    Case(256, 1, 6, 255, K, "tanh"),
    Case(256, 17, 6, 256, G, "relu"),
    Case(256, 64, 8, 256, K, "relu", acc=1),
    # every in_dim at B = 65 (in_dim 3 above)
    Case(64, 1, 1, 65, G, "tanh"),
    Case(128, 3, 2, 65, G, "relu"),
    Case(192, 4, 6, 65, K, "relu", acc=1),
    Case(64, 17, 8, 65, G, "relu"),
    Case(128, 63, 2, 65, K, "tanh"),
    Case(192, 64, 6, 65, G, "tanh", acc=1),
    # the other widths over the other batch sizes
    Case(64, 4, 2, 1, K, "relu", acc=1),
    Case(64, 63, 6, 15, G, "relu"),
    Case(64, 3, 8, 64, K, "tanh"),
    Case(64, 64, 2, 130, G, "relu"),
    Case(64, 17, 6, 255, G, "tanh", acc=1),
    Case(64, 1, 8, 256, G, "relu"),
    Case(128, 17, 6, 1, G, "tanh"),
    Case(128, 1, 2, 15, K, "relu"),
    Case(128, 64, 1, 64, G, "relu", acc=1),
    Case(128, 4, 8, 130, K, "relu"),
    Case(128, 3, 6, 255, K, "relu"),
    Case(128, 63, 8, 256, G, "tanh"),
    Case(192, 3, 1, 1, G, "relu"),
    Case(192, 17, 8, 15, G, "tanh", acc=1),
    Case(192, 1, 2, 64, K, "tanh"),
    Case(192, 63, 6, 130, K, "relu"),
    Case(192, 4, 1, 255, G, "relu"),
    Case(192, 17, 2, 256, K, "tanh", acc=1),
    # the whole parameter / gradient layout and / or the observations one float off 16-byte alignment
    Case(256, 17, 6, 65, G, "relu", pshift=1),
    Case(128, 3, 2, 130, K, "tanh", acc=1, pshift=1, oshift=1),
    Case(64, 4, 8, 64, G, "relu", oshift=1),
    Case(256, 63, 1, 255, G, "tanh", pshift=1, oshift=1),
    Case(192, 64, 8, 256, K, "relu", pshift=1),
    # the two shapes the trainer tests use
    Case(256, 4, 2, 64, K, "relu"),
    Case(64, 17, 6, 64, G, "tanh"),
]
# one seed per case, searched on the CPU upwards from 1000 + index (ReLU cases: relu_margin >= 2^-18)
SEEDS = [1000, 1001, 1002, 1014, 1012, 1005, 1048, 1034, 1008, 1011, 1010, 1011, 1012, 1013, 1014, 1015, 1016, 1017,
         1018, 1039, 1020, 1021, 1022, 1026, 1035, 1025, 1026, 1027, 1028, 1029, 1173, 1031, 1034, 1033, 1035, 1035,
         1057, 1039, 1038]
assert len(SEEDS) == len(CASES)
CASES = [c._replace(seed=s) for c, s in zip(CASES, SEEDS)]


def test_case_table_covers_the_required_combinations():
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in CASES)
    assert all(has(H=256, B=b) for b in (1, 15, 64, 65, 130, 255, 256))
    assert all(has(B=65, in_dim=i) for i in (1, 3, 4, 17, 63, 64))
    assert has(out=8, head=G) and has(out=8, head=K)
    assert all(has(H=h) for h in (64, 128, 192, 256)) and all(has(out=o) for o in (1, 2, 6, 8))
    assert all(has(head=h, act=a, acc=m) for h in (G, K) for a in ("tanh", "relu") for m in (0, 1))
    assert not has(out=1, head=K)  # a one-action Categorical is degenerate
    assert len({cid(c) for c in CASES}) == len(CASES)
    # the whole-epoch cases: both value-loss forms, Huber with and without value clipping
    assert {c.vf for c in ECASES} == {"mse_loss", "huber_loss"}
    assert {c.vclip is not None for c in ECASES if c.vf == "huber_loss"} == {True, False}
    assert len({cid(c) for c in ECASES}) == len(ECASES)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_forward_backward_dist_params_vs_float64(c):
    """rai_mlp_wide_forward, rai_mlp_wide_backward and rai_mlp_wide_dist_params on parameter and
    gradient views carved from one flat buffer, NaN-filled outputs and an exactly-sized workspace
    between 0xFF guard bytes (the workspace itself starts as 0xFF = NaN too, so a read of an unwritten
    word shows).  accumulate = 1 adds ONE rounded value per element (put() in mlp_wide.hip), so it is
    held bit-equal to base + the accumulate = 0 result.  dist_params runs the forward's layer kernels
    and sums the slice partials in the same order, so its v is held bit-equal to the forward's."""
    params, obs, actions, cot = make_inputs(c)
    ref = run_ref(c, params, obs, actions, cot, F64)
    assert_relu_condition(c, ref.zs)
    t32 = run_ref(c, params, obs, actions, cot, F32, DEV)

    w = Wide(c, params, obs, actions)
    dcot = [t.to(DEV) for t in cot]
    logp, ent, v = w.forward()
    gbuf, g = w.backward(dcot)
    torch.cuda.synchronize()
    assert_guards(w.big, w.ws_bytes)
    ratios = {}
    for name, got, r64, r32 in [("logp", logp, ref.logp, t32.logp), ("ent", ent, ref.ent, t32.ent),
                                ("v", v, ref.v, t32.v)]:
        ratios[name] = check(name, got, r64, r32, "forward")
    for name, got, r64, r32 in zip(grad_names(c), g, ref.grads, t32.grads):
        ratios["d" + name] = check("d" + name, got, r64, r32, "backward")
    # nothing outside the views: the shift prefix and the tail keep their NaN
    assert bool(torch.isnan(gbuf[:c.pshift]).all()) and bool(torch.isnan(gbuf[c.pshift + w.P:]).all())

    # determinism: the same two calls again, bit-equal
    logp2, ent2, v2 = w.forward()
    gbuf2, _ = w.backward(dcot)
    for a, b in [(logp, logp2), (ent, ent2), (v, v2), (gbuf, gbuf2)]:
        assert torch.equal(bits(a), bits(b)), "two runs differ"

    if c.acc:
        gen = torch.Generator().manual_seed(c.seed + 1)
        base = [torch.randn(s, generator=gen).to(DEV) for s in param_shapes(c)]
        _, ga = w.backward(dcot, accumulate=1, base=base)
        for name, got, b0, g0 in zip(grad_names(c), ga, base, g):
            assert torch.equal(got, b0 + g0), f"accumulate: d{name} is not base + gradient"

    po, vo = w.dist_params()
    torch.cuda.synchronize()
    assert_guards(w.big, w.ws_bytes)
    ratios["params_out"] = check("params_out", po, ref.o, t32.o, "dist_params")
    ratios["v_out"] = check("v_out", vo, ref.v, t32.v, "dist_params")
    assert torch.equal(bits(vo), bits(v)), "dist_params' v differs from the forward's"
    worst = max(ratios, key=ratios.get)
    print(f"\n{cid(c)}: worst err/bound {ratios[worst]:.3f} ({worst})")


@pytest.mark.gpu
def test_bad_shapes_are_rejected_before_any_write():
    """check() admits observations at any 4-byte alignment (covered by the oshift cases); shapes outside
    its limits return an error code and leave NaN-filled outputs untouched."""
    c = Case(64, 4, 2, 8, K, "tanh", seed=5)
    params, obs, actions, _ = make_inputs(c)
    w = Wide(c, params, obs, actions)
    for field, val, code in [("in_dim", 65, _lib.RAI_E_UNSUPPORTED), ("in_dim", 0, _lib.RAI_E_UNSUPPORTED),
                             ("out_pi", 9, _lib.RAI_E_UNSUPPORTED), ("hidden", 96, _lib.RAI_E_UNSUPPORTED),
                             ("hidden", 320, _lib.RAI_E_UNSUPPORTED), ("head", 2, _lib.RAI_E_MODE)]:
        d = make_desc(c, w.p, None)
        setattr(d, field, val)
        logp, ent, v = w.outputs()
        rc = _lib.lib().rai_mlp_wide_forward(C.byref(d), w.obs.data_ptr(), w.actions.data_ptr(), c.B, logp.data_ptr(),
                                             ent.data_ptr(), v.data_ptr(), w.ws.data_ptr(), w.ws_bytes, w.st)
        assert rc == code, (field, val, rc)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (logp, ent, v))
    d = make_desc(c, w.p, None)
    logp, ent, v = w.outputs()
    for B, nbytes, code in [(0, w.ws_bytes, _lib.RAI_E_SHAPE), (257, 1 << 30, _lib.RAI_E_SHAPE),
                            (c.B, w.ws_bytes - 1, _lib.RAI_E_WORKSPACE)]:
        rc = _lib.lib().rai_mlp_wide_forward(C.byref(d), w.obs.data_ptr(), w.actions.data_ptr(), B, logp.data_ptr(),
                                             ent.data_ptr(), v.data_ptr(), w.ws.data_ptr(), nbytes, w.st)
        assert rc == code, (B, nbytes, rc)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (logp, ent, v))
    assert_guards(w.big, w.ws_bytes)


# ---------------------------------------------------------------------------------------------
# 2. rai_mlp_wide_forward_loss == rai_mlp_wide_forward + rai_ppo_loss
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("vclip", [None, 0.2])
@pytest.mark.parametrize("head", [G, K])
@pytest.mark.parametrize("B", [1, 64, 65, 256])
def test_forward_loss_equals_forward_then_ppo_loss(B, head, vclip, ent_coef):
    """The fused head + loss launch against the two separate calls, K = 1, hyperparameter and state
    blocks as pg_common.DeviceBlocks uploads them: logp, ent, v, d_logp, d_entropy, d_values, the
    stats row and the advanced stat_index are bit-equal (both launch pg_loss_body<1> of loss_body.h
    on one 256-thread workgroup without FP contraction).  B = 1 runs without advantage normalization:
    a one-row minibatch has no unbiased std (NaN in both)."""
    c = Case(128, 17, 6, B, G, "tanh", seed=2000 + B) if head == G else Case(64, 3, 8, B, K, "relu", seed=2100 + B)
    params, obs, actions, _ = make_inputs(c)
    g = torch.Generator().manual_seed(c.seed + 7)
    w = Wide(c, params, obs, actions)
    logp0, _, v0 = w.forward()
    old_logp = logp0 + 0.3 * torch.randn(B, generator=g).to(DEV)
    old_v = v0 + 0.3 * torch.randn(B, generator=g).to(DEV)
    adv, ret = torch.randn(B, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    hp = make_hparams(loss_kind=0, K=1, clip_range=0.2, clip_range_vf=vclip, ent_coef=ent_coef, vf_coef=0.5,
                      normalize_advantage=B > 1)
    L = _lib.lib()
    res = []
    for fused in (False, True):
        blocks = DeviceBlocks(DEV)
        blocks.stats.fill_(NAN)
        blocks.upload(hp, 0)
        logp, ent, v = w.outputs()
        d_logp, d_ent, d_v = w.outputs()
        d = make_desc(c, w.p, None)
        if fused:
            rc = L.rai_mlp_wide_forward_loss(
                C.byref(d), w.obs.data_ptr(), w.actions.data_ptr(), B, logp.data_ptr(), ent.data_ptr(), v.data_ptr(),
                old_logp.data_ptr(), old_v.data_ptr(), adv.data_ptr(), ret.data_ptr(), blocks.hp.data_ptr(),
                blocks.state.data_ptr(), d_logp.data_ptr(), d_ent.data_ptr(), d_v.data_ptr(), blocks.stats.data_ptr(),
                int(blocks.stats.shape[0]), w.ws.data_ptr(), w.ws_bytes, w.st)
            assert rc == 0, rc
        else:
            rc = L.rai_mlp_wide_forward(C.byref(d), w.obs.data_ptr(), w.actions.data_ptr(), B, logp.data_ptr(),
                                        ent.data_ptr(), v.data_ptr(), w.ws.data_ptr(), w.ws_bytes, w.st)
            assert rc == 0, rc
            rc = L.rai_ppo_loss(logp.data_ptr(), ent.data_ptr(), ent.numel(), v.data_ptr(), old_logp.data_ptr(),
                                old_v.data_ptr(), adv.data_ptr(), ret.data_ptr(), B, 1, blocks.hp.data_ptr(),
                                blocks.state.data_ptr(), d_logp.data_ptr(), d_ent.data_ptr(), d_v.data_ptr(),
                                blocks.stats.data_ptr(), int(blocks.stats.shape[0]), None, 0, w.st)
            assert rc == 0, rc
        torch.cuda.synchronize()
        res.append(dict(logp=logp, ent=ent, v=v, d_logp=d_logp, d_ent=d_ent, d_v=d_v, stats=blocks.stats[0].clone(),
                        state=blocks.state.clone()))
    assert_guards(w.big, w.ws_bytes)
    sep, fus = res
    for k in sep:
        assert torch.equal(sep[k].view(torch.uint8) if k == "state" else bits(sep[k]),
                           fus[k].view(torch.uint8) if k == "state" else bits(fus[k])), f"{k} differs"
    written = [0, 1, 2, 3, 4, 5, 5 + _lib.RAI_MAX_K]
    assert bool(torch.isfinite(fus["stats"][written]).all()), fus["stats"]
    for k in ("logp", "ent", "v", "d_logp", "d_ent", "d_v"):
        assert bool(torch.isfinite(fus[k]).all()), k
    assert int(fus["state"].view(torch.int32)[2]) == 1  # stat_index advanced
    assert bool((fus["d_ent"] == 0).all()) == (ent_coef == 0.0)


# ---------------------------------------------------------------------------------------------
# 3. the whole-epoch kernel's gradient, from Adam's first moment after one step
# ---------------------------------------------------------------------------------------------
ECase = namedtuple("ECase", "H in_dim out B head act vclip ent_coef pshift seed vf", defaults=(0, 0, "mse_loss"))
ECASES = [
    ECase(256, 17, 6, 64, G, "relu", None, 0.01),
    ECase(256, 17, 6, 50, G, "tanh", 0.2, 0.0),
    ECase(64, 17, 6, 16, G, "relu", 0.2, 0.01),
    ECase(64, 3, 1, 2, G, "tanh", None, 0.01),
    ECase(256, 1, 8, 64, G, "tanh", 0.2, 0.01),
    ECase(64, 64, 8, 50, G, "relu", None, 0.0),
    ECase(256, 64, 1, 16, G, "relu", 0.2, 0.0),
    ECase(256, 3, 6, 2, G, "relu", 0.2, 0.01),
    ECase(64, 1, 6, 64, K, "relu", None, 0.01),
    ECase(256, 3, 8, 50, K, "tanh", 0.2, 0.01),
    ECase(64, 17, 8, 16, K, "tanh", None, 0.0),
    ECase(256, 64, 6, 2, K, "relu", 0.2, 0.01),
    ECase(64, 64, 6, 64, K, "tanh", 0.2, 0.0),
    ECase(256, 17, 8, 64, K, "relu", 0.2, 0.01),
    ECase(64, 17, 1, 50, G, "tanh", 0.2, 0.01, pshift=1),
    ECase(256, 1, 6, 16, K, "relu", None, 0.01),
    # the critic's Huber branch (vf_loss_fn = 1), with and without value clipping
    ECase(64, 3, 6, 16, G, "tanh", 0.2, 0.01, vf="huber_loss"),
    ECase(256, 17, 8, 50, K, "relu", None, 0.0, vf="huber_loss"),
]
# one seed per case, searched on the CPU upwards from 3000 + 100 * index for epoch_conditions(margin=4e-4)
# (which, for a Huber case, also asks for rows on both sides of |v - R| = 1 in the float64 reference)
ESEEDS = [3000, 3100, 3200, 3301, 3400, 3500, 3600, 3702, 3802, 3900, 4000, 4102, 4200, 4302, 4400, 4500, 4600, 4700]
assert len(ESEEDS) == len(ECASES)
ECASES = [c._replace(seed=s) for c, s in zip(ECASES, ESEEDS)]
CLIP, VF_COEF, BETA1 = 0.2, 0.5, 0.9


def epoch_inputs(c):
    """The part-1 inputs plus the rollout columns: old_logp = the float64 reference's logp + N(0, 0.3)
    (so both clip branches occur), old_v likewise, advantages and returns N(0, 1)."""
    params, obs, actions, _ = make_inputs(c)
    with torch.no_grad():
        logp, _, v, _, zs = forward_ref(cast(params, F64), obs.double(), actions.double() if c.head == G else actions, c)
    g = torch.Generator().manual_seed(c.seed + 7)
    rn = lambda: torch.randn(c.B, generator=g)
    old_logp, old_v = (logp + 0.3 * rn().double()).float(), (v + 0.3 * rn().double()).float()
    return params, obs, actions, old_logp, old_v, rn(), rn(), zs


def ppo_ref(c, params, obs, actions, old_logp, old_v, adv, ret, dtype, device="cpu"):
    """rl_algo_impls/ppo/ppo.py:290-377 for K = 1: minibatch-normalized advantages, the clipped
    surrogate, the value loss (MSE, or Huber = smooth_l1 with beta 1: 0.5 z^2 for |z| < 1, else
    |z| - 0.5; optionally clipped around old_v), the entropy term; gradients by autograd.  Returns the gradients, their norm, stats columns 0..5 (column 0 without the value term,
    as the kernel writes it) and the ratios / value moves for the conditions."""
    p = [t.requires_grad_(True) for t in cast(params, dtype, device)]
    obs, actions, old_logp, old_v, adv, ret = cast([obs, actions, old_logp, old_v, adv, ret], dtype, device)
    logp, ent, v, _, _ = forward_ref(p, obs, actions, c)
    A = (adv - adv.mean()) / (adv.std() + 1e-8)
    logratio = logp - old_logp
    ratio = logratio.exp()
    pi_loss = -torch.min(ratio * A, ratio.clamp(1 - CLIP, 1 + CLIP) * A).mean()
    if c.vf == "huber_loss":
        vf = lambda z: torch.where(z.abs() < 1, 0.5 * z * z, z.abs() - 0.5)
    else:
        vf = lambda z: z ** 2
    v_loss = vf(v - ret)
    if c.vclip is not None:
        v_cl = old_v + (v - old_v).clamp(-c.vclip, c.vclip)
        v_loss = torch.max(v_loss, vf(v_cl - ret))
    v_loss = v_loss.mean()
    ent_loss = -ent.mean()
    grads = torch.autograd.grad(pi_loss + c.ent_coef * ent_loss + VF_COEF * v_loss, p)
    det = lambda t: t.detach().double().cpu()
    grads = [det(g_) for g_ in grads]
    stats = torch.stack([det(pi_loss + c.ent_coef * ent_loss), det(pi_loss), det(ent_loss),
                         det(((ratio - 1) - logratio).mean()),
                         det(((ratio - 1).abs() > CLIP).to(dtype).mean()), det(v_loss)])
    norm = torch.sqrt(sum((g_ ** 2).sum() for g_ in grads))
    return SimpleNamespace(grads=grads, stats=stats, norm=norm, ratio=det(ratio), dv=det(v - old_v),
                           verr=det(v - ret))


def epoch_conditions(c, ref, zs, margin=1e-4, both_branches=True):
    """None when the float64 reference is clear of every discontinuity, else what is too close
    (both_branches=False: a minibatch of two or three rows need not show both clip branches)."""
    if c.act == "relu" and relu_margin(zs) < 2.0 ** -20 * (margin / 1e-4):
        return "a pre-activation within 2^-20 of zero"
    if float(((ref.ratio - 1).abs() - CLIP).abs().min()) < margin:
        return "a ratio within 1e-4 of 1 +- clip_range"
    if c.vclip is not None and float((ref.dv.abs() - c.vclip).abs().min()) < margin:
        return "a value move within 1e-4 of +- clip_range_vf"
    clipped = (ref.ratio - 1).abs() > CLIP
    if both_branches and not (bool(clipped.any()) and bool((~clipped).any())):
        return "the rows do not exercise both clip branches"
    if c.vf == "huber_loss" and not (bool((ref.verr.abs() < 1).any()) and bool((ref.verr.abs() > 1).any())):
        return "the rows do not lie on both sides of |v - R| = 1"
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("c", ECASES, ids=cid)
def test_epoch_gradient_from_first_moment(c):
    """One rai_mlp_wide_epoch call with n_rows == batch_size from zero Adam moments and no clipping
    (max_grad_norm 1e30): exp_avg = (1 - beta1) * g, so g = exp_avg / (1 - beta1) is the gradient the
    kernel formed (it never writes gradients to memory).  g, norms[0] and stats columns 0..5 against
    float64 autograd of the PPO loss, by the part-1 tolerance rule.

    The stats row is held as ONE tensor (columns 0..5 against the row's max|ref64|), not column by
    column: pi_loss is a small difference of terms ratio_b A_b = exp(logp_b - old_logp_b) A_b, so one
    float32 ulp of a logp near -21 (1.9e-6) moves it by |A_b ratio_b| / B ulp -- 7e-7 at B = 2,
    against a per-column floor 1e-5 |pi_loss| = 1e-6.  No float32 evaluation of logp (a sum of `out`
    rounded terms) can promise under 1.5 ulp there: a first, per-column version of this check measured
    err / bound = 1.23 on column 0 of the H256-in3-out6-B2 case, with torch's own float32 run on the
    CPU at 0.55 of the same floor."""
    params, obs, actions, old_logp, old_v, adv, ret, zs = epoch_inputs(c)
    ref = ppo_ref(c, params, obs, actions, old_logp, old_v, adv, ret, F64)
    bad = epoch_conditions(c, ref, zs)
    assert bad is None, f"{bad}: pick another seed"
    t32 = ppo_ref(c, params, obs, actions, old_logp, old_v, adv, ret, F32, DEV)

    L = _lib.lib()
    pbuf, p, P = carve(param_shapes(c), c.pshift, NAN)
    for dst, src in zip(p, params):
        dst.copy_(src)
    flat = pbuf[c.pshift:c.pshift + P]
    p0 = flat.clone()
    mbuf, m, _ = carve(param_shapes(c), c.pshift, 0.0)
    vbuf, _, _ = carve(param_shapes(c), c.pshift, 0.0)
    d = make_desc(c, p, None)
    ws_bytes = int(L.rai_mlp_wide_epoch_workspace_bytes(c.H, c.in_dim, c.B))
    assert ws_bytes > 0
    big, ws = guarded_workspace(ws_bytes, fill=0)  # zeroed, as the trainer allocates it
    from rl_algo_impls_amd.optim import struct_to_device

    hp = struct_to_device(make_hparams(loss_kind=0, K=1, clip_range=CLIP, clip_range_vf=c.vclip, ent_coef=c.ent_coef,
                                       vf_coef=VF_COEF, normalize_advantage=True, vf_loss_fn=c.vf), DEV)
    ohp = struct_to_device(_lib.OptimHparams(lr=3e-4, beta1=BETA1, beta2=0.999, eps=1e-7, alpha=0.99,
                                             max_grad_norm=1e30, kind=0, beta1_d=BETA1, beta2_d=0.999), DEV)
    state = struct_to_device(_lib.TrainState(opt_step=0, stat_index=0, pi_coef_zero=0, norm_index=0), DEV)
    stats = torch.full((1, _lib.RAI_STAT_STRIDE), NAN, dtype=F32, device=DEV)
    norms = torch.full((1,), NAN, dtype=F32, device=DEV)
    dev = lambda t: t.to(DEV).contiguous()
    obs_d, act_d, olp_d, ov_d, adv_d, ret_d = map(dev, (obs, actions, old_logp, old_v, adv, ret))
    rc = L.rai_mlp_wide_epoch(C.byref(d), flat.data_ptr(), mbuf[c.pshift:].data_ptr(), vbuf[c.pshift:].data_ptr(), P,
                              obs_d.data_ptr(), act_d.data_ptr(), olp_d.data_ptr(), ov_d.data_ptr(), adv_d.data_ptr(),
                              ret_d.data_ptr(), c.B, c.B, hp.data_ptr(), ohp.data_ptr(), state.data_ptr(),
                              stats.data_ptr(), 1, norms.data_ptr(), 1, ws.data_ptr(), ws_bytes,
                              _lib.stream_handle(DEV))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert_guards(big, ws_bytes)
    st = state.cpu().numpy()
    assert int(st[:8].view(np.int64)[0]) == 1 and list(st[8:].view(np.int32)) == [1, 0, 1, 0], "one step, no err flag"
    # nothing outside the flat views; the parameters moved (Adam's first step is lr * sign(g))
    for buf, fill_nan in ((pbuf, True), (mbuf, False), (vbuf, False)):
        edge = torch.cat([buf[:c.pshift], buf[c.pshift + P:]])
        assert bool(torch.isnan(edge).all() if fill_nan else (edge == 0).all())
    assert bool(torch.isfinite(flat).all())
    c1 = float(np.float32(1.0 - BETA1))  # the kernel's (float)(1 - beta1_d)
    ratios = {}
    for name, mi, r64, r32 in zip(grad_names(c), m, ref.grads, t32.grads):
        ratios["d" + name] = check("d" + name, mi.double() / c1, r64, r32, "epoch_grad")
    ratios["norm"] = check("norm", norms, ref.norm, t32.norm, "epoch_grad")
    ratios["stats"] = check("stats[0:6]", stats[0, :6], ref.stats, t32.stats, "epoch_stats")
    # the step itself: every parameter with a non-negligible gradient moved against it by about lr
    gflat = torch.cat([g_.reshape(-1) for g_ in ref.grads])
    big_g = gflat.abs() > 1e-3 * float(gflat.abs().max())
    step = (flat - p0).double().cpu()
    assert bool((torch.sign(step[big_g]) == -torch.sign(gflat[big_g])).all())
    np.testing.assert_allclose(step[big_g].abs().numpy(), 3e-4, rtol=1e-2)
    worst = max(ratios, key=ratios.get)
    print(f"\n{cid(c)}: worst err/bound {ratios[worst]:.3f} ({worst})")


@pytest.mark.gpu
def test_report_worst_ratios():
    """Prints the worst err / bound ratio per part over the cases that ran before it in this module
    (every one of them already asserted <= 1)."""
    print("\nworst err/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))
    assert all(v <= 1.0 for v in WORST.values())
