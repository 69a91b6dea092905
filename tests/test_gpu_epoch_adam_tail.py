"""The tail of the CartPole epoch kernel's step (csrc/mlp_mc8.h, after the round-2 wait): the all-gather of the
summed gradient, the global norm from the share-norm granules, clip_grad_norm_'s coefficient and the
whole-network Adam on every CU's own copy of the weights and moments.

rai_mlp_ppo_epoch is called directly (test_gpu_mlp64_kernels' harness) on a CartPole-shaped policy
(in 4 -> 64 -> 64 -> 2 and -> 1) and the parameters and both Adam moments it leaves are held against a float64
restatement of clip-by-global-norm + Adam:

    g_k     the float64 gradient (test_gpu_mlp64_kernels.ppo64) of minibatch k at the restatement's own
            float64 parameters,
    coef_k  min(max_grad_norm / (norm_k + 1e-6), 1) with norm_k the norm the KERNEL reported for step k,
    m, v    m + w1 (coef g - m), beta2 v + w2 (coef g)^2 with the kernel's float w1, w2, beta2,
    p       p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps).

Tolerances: the ones test_gpu_epoch_dw2_registers.py and test_gpu_trainer.py::
test_fused_epoch_matches_generic_path state for the fused kernel's hardware sqrt / rcp Adam against another
implementation of the same update -- parameters rtol 1e-3, atol 2e-5; both moments rtol 2e-2, atol 1e-6.

Geometries (how each is reached: test_gpu_mlp64_kernels.VARIANTS): G = 16 at batch 256, RAI_MLP_CUS=8 (two row
tiles per CU) at batch 256 and the per-rank geometry at batch 128, each with tanh and with ReLU, three
minibatches per launch of which the last is short (the rows < B path; slot parities 0, 1, 0).  lr = 3e-3 as in
test_gpu_epoch_dw2_registers.py, and max_grad_norm lies inside the range of the three steps' gradient norms, so
that a launch has clipped and unclipped steps (asserted on the float64 reference's norms).

Discontinuities are a condition on the reference (test_gpu_mlp64_kernels.conditions, asserted at every step):
the seeds below were searched on the CPU with at least twice the margin, with the float64 reference's own norms
in the place of the kernel's, and so that no step's norm lies within 1 % of max_grad_norm.

One more launch runs M8_BC_MAX + 3 = 2,051 dependent steps at a 16-row batch (the per-rank geometry), past the
end of the kernel's table of Adam bias corrections, so the last three steps form them in the loop.  Over 2,051
steps no seed can keep every row of every step clear of the surrogate's clip boundaries, and the launch is about
the optimizer tail, not about the loss: it runs tanh, the plain value loss and clip_range 1e3 (in the
kernel's hyper-parameters and in the reference alike), a loss without discontinuities, at lr = 3e-4.

Each case also requires a second launch from the same inputs to leave identical bits (parameters, moments,
norms, stats rows), and the state block to end at (steps, steps, steps, err 0).

Measured on an MI355X, worst err / bound over the cases (each case prints its own): parameters 0.050, exp_avg
0.007, exp_avg_sq below 0.001; the kernel's norms within 9.1e-7 relative of the float64 reference's.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_mlp64_kernels as m64
from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.optim import struct_to_device
from test_gpu_mlp64_kernels import B2F, BETA1, BETA2, EPS, W1, W2, MCase, Run, conditions, ppo64, rollout, select_variant
from test_gpu_wide_kernels import DEV, F64, bits

pytestmark = pytest.mark.gpu

M8_BC_MAX = 2048  # csrc/mlp_mc8.h: steps of a launch whose bias corrections are tabulated
P_TOL = dict(rtol=1e-3, atol=2e-5)
M_TOL = dict(rtol=2e-2, atol=1e-6)
T, R = "tanh", "relu"


def _case(variant, act, B, tail, seed):
    return MCase(variant, 4, 2, B, act, None, 0.01, "mse_loss", 0, "norm", n_rows=2 * B + tail, seed=seed)


# three minibatches, the last short (seeds: see the module docstring)
CASES = [
    _case("mc16", T, 256, 77, 21001),
    _case("mc16", R, 256, 77, 21151),
    _case("mc8", T, 256, 45, 21201),
    _case("mc8", R, 256, 45, 21306),
    _case("mc8x16", T, 128, 37, 21400),
    _case("mc8x16", R, 128, 37, 21503),
]
LONG = MCase("mc8x16", 4, 2, 16, T, None, 0.0, "mse_loss", 0, "norm", n_rows=16 * (M8_BC_MAX + 3), seed=22000)
LONG_CLIP = 1e3


def _id(c):
    return f"{c.variant}-B{c.B}-{c.act}-n{c.rows}"


def adam_restatement(c, d, norms, lr, max_grad_norm, check_conditions):
    """The float64 restatement (module docstring) over every minibatch of the launch; `norms`: the per-step
    gradient norms that decide the clip coefficient.  Returns the flat parameters, both moments, the
    reference's own norms and the coefficients."""
    p = [t.double() for t in d.params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    ref_norms, coefs = [], []
    cur = SimpleNamespace(**vars(d))
    for k in range(d.nmb):
        cur.params = [t.clone() for t in p]  # ppo64 marks the tensors it is given as requiring grad
        ref = ppo64(c, cur, k, F64)
        if check_conditions:
            bad = conditions(c, ref)
            assert bad is None, f"step {k}: {bad}: pick another seed"
        ref_norms.append(float(ref.norm))
        nk = float(ref.norm) if norms is None else float(norms[k])
        coef = min(max_grad_norm / (nk + 1e-6), 1.0)
        coefs.append(coef)
        t = k + 1
        bc2_sqrt = (1.0 - BETA2 ** t) ** 0.5
        step = lr / (1.0 - BETA1 ** t)
        for i, g_ in enumerate(ref.grads):
            g = coef * g_
            m[i] = m[i] + W1 * (g - m[i])
            v[i] = B2F * v[i] + W2 * g * g
            p[i] = p[i] - step * m[i] / (v[i].sqrt() / bc2_sqrt + EPS)
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).numpy()
    return SimpleNamespace(params=flat(p), m=flat(m), v=flat(v), norms=np.array(ref_norms), coefs=np.array(coefs))


@functools.lru_cache(maxsize=None)
def clip_norm(c):
    """max_grad_norm of a case: the middle of the range of its steps' float64 gradient norms along the
    unclipped restatement's first pass -- some steps of the launch clip and some do not."""
    first = adam_restatement(c, rollout(c), None, 3e-3, 1e30, False)
    return 0.5 * float(first.norms.min() + first.norms.max())


def launch(c, d, lr, max_grad_norm):
    run = Run(c, d, lr=lr)
    run.ohp = struct_to_device(_lib.OptimHparams(lr=lr, beta1=BETA1, beta2=BETA2, eps=EPS, alpha=0.99,
                                                 max_grad_norm=max_grad_norm, kind=0, beta1_d=BETA1, beta2_d=BETA2),
                               DEV)
    rc = run.epoch()
    assert rc == 0, rc
    torch.cuda.synchronize()
    s, P = c.pshift, run.P
    return SimpleNamespace(params=run.flat.clone(), m=run.mbuf[s:s + P].clone(), v=run.vbuf[s:s + P].clone(),
                           norms=run.norms.clone(), stats=run.stats.clone(), state=m64.state_words(run.state))


def hold(c, d, lr, max_grad_norm, check_conditions):
    first = launch(c, d, lr, max_grad_norm)
    assert first.state == (d.nmb, d.nmb, d.nmb, 0), "every step taken, no err flag"
    second = launch(c, d, lr, max_grad_norm)
    for k in ("params", "m", "v", "norms", "stats"):
        assert torch.equal(bits(getattr(first, k)), bits(getattr(second, k))), f"{k} differs between two launches"
    for k in ("params", "m", "v", "norms"):
        assert bool(torch.isfinite(getattr(first, k)).all()), k
    norms = first.norms.double().cpu().numpy()
    ref = adam_restatement(c, d, norms, lr, max_grad_norm, check_conditions)
    got = {k: getattr(first, k).double().cpu().numpy() for k in ("params", "m", "v")}
    worst = lambda a, b, tol: float(np.max(np.abs(a - b) / (tol["atol"] + tol["rtol"] * np.abs(b))))
    print(f"\n{c.variant}-B{c.B}-{c.act}-n{c.rows}: err/bound params {worst(got['params'], ref.params, P_TOL):.3f}, "
          f"exp_avg {worst(got['m'], ref.m, M_TOL):.3f}, exp_avg_sq {worst(got['v'], ref.v, M_TOL):.3f}; "
          f"norm kernel/ref - 1 max {np.max(np.abs(norms / ref.norms - 1)):.2e}; "
          f"clipped steps {int((ref.coefs < 1).sum())} of {d.nmb}")
    np.testing.assert_allclose(got["params"], ref.params, **P_TOL)
    np.testing.assert_allclose(got["m"], ref.m, **M_TOL)
    np.testing.assert_allclose(got["v"], ref.v, **M_TOL)
    return ref


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_adam_tail_three_minibatches(c, monkeypatch):
    """Three minibatches per launch, the last short, in each geometry and activation: parameters and both
    moments against the float64 restatement, identical bits from a second launch, err 0."""
    d = rollout(c)
    assert d.nmb == 3 and d.n % c.B != 0
    mgn = clip_norm(c)
    select_variant(monkeypatch, c)
    ref = hold(c, d, 3e-3, mgn, True)
    assert bool((ref.coefs < 1).any()) and bool((ref.coefs == 1).any()), "clipped and unclipped steps"


def test_adam_tail_past_the_bias_correction_table(monkeypatch):
    """2,051 dependent steps at a 16-row batch in one launch: the last three steps form Adam's bias corrections
    in the loop.  clip_range 1e3 (see the module docstring); max_grad_norm 1.5, inside the range of the steps' norms."""
    c = LONG
    monkeypatch.setattr(m64, "CLIP", LONG_CLIP)
    d = rollout(c)
    assert d.nmb == M8_BC_MAX + 3
    select_variant(monkeypatch, c)
    hold(c, d, 3e-4, 1.5, False)
