"""rai_clip_optim_step_runs (the run-wise clip + Adam / RMSprop step behind PPO's freeze_* options) through
the C ABI: one run against the flat step bit for bit, several runs with different lags against
torch.optim on the CPU, and the error codes.

Tolerance against torch: max(1e-5 |ref|, 4 x |f32 - f64|) with the reference run in float32 and, from the
same bits, in float64 (the rule of tests/test_multidiscrete_cpu.py; the error term is computed in the test,
per tensor for parameters and moments as in the fixtures).
"""
from __future__ import annotations


import numpy as np
import pytest
import torch

from rl_algo_impls_amd import _lib
from rl_algo_impls_amd.optim import struct_to_device
from test_multidiscrete_cpu import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ADAM, RMSPROP = 0, 1
LR = 1e-2


def hparams(kind, max_norm):
    eps = 1e-7 if kind == ADAM else 1e-5
    hp = _lib.OptimHparams(lr=LR, beta1=0.9, beta2=0.999, eps=eps, alpha=0.99, max_grad_norm=max_norm, kind=kind,
                           beta1_d=0.9 if kind == ADAM else 0.99, beta2_d=0.999)
    return struct_to_device(hp, DEV)


def run_table(runs, out=None):
    arr = (_lib.OptimRun * _lib.RAI_OPTIM_MAX_RUNS)()
    for k, (b, e, lag, act) in enumerate(runs):
        arr[k] = _lib.OptimRun(begin=b, end=e, lag=lag, active=act)
    return struct_to_device(arr, DEV, out)


class Buffers:
    """p, g, m, v of P floats at a 16-byte-aligned address (shift 0) or one float past it (shift 1), the
    train-state block, a norms table and the workspace."""

    def __init__(self, P, shift, seed, kind):
        rng = np.random.default_rng(seed)
        self.P, self.kind = P, kind
        mk = lambda a: torch.from_numpy(np.concatenate([np.zeros(shift, np.float32), a.astype(np.float32)])).to(DEV)
        self._p = mk(rng.standard_normal(P))
        self._g = mk(rng.standard_normal(P))  # norm ~ sqrt(P): above 0.5 for every P used
        self._m = mk(np.abs(rng.standard_normal(P)) * 0.1 if kind == RMSPROP else rng.standard_normal(P) * 0.1)
        self._v = mk(np.abs(rng.standard_normal(P)) * 0.1)
        self.p, self.g, self.m, self.v = (t[shift:] for t in (self._p, self._g, self._m, self._v))
        assert self.p.data_ptr() % 16 == 4 * shift
        self.state = struct_to_device(_lib.TrainState(opt_step=3), DEV)
        self.norms = torch.full((8,), -1.0, device=DEV)
        self.ws = torch.zeros(int(_lib.lib().rai_optim_workspace_bytes(P)), dtype=torch.uint8, device=DEV)

    def args(self, hp):
        return (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(),
                self.v.data_ptr() if self.kind == ADAM else None, self.P, hp.data_ptr(), self.state.data_ptr())

    def tail(self):
        return (self.norms.data_ptr(), int(self.norms.numel()), self.ws.data_ptr(), self.ws.numel(), _lib.stream_handle(DEV))

    def flat_step(self, hp):
        _lib.check(_lib.lib().rai_clip_optim_step(*self.args(hp), *self.tail()), "flat")

    def runs_step(self, hp, table, n):
        _lib.check(_lib.lib().rai_clip_optim_step_runs(*self.args(hp), table.data_ptr(), n, *self.tail()), "runs")

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self.p, self.g, self.m, self.v, self.norms, self.state)]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "plus_one_float"])
@pytest.mark.parametrize("max_norm", [0.5, 0.0], ids=["clip", "noclip"])
@pytest.mark.parametrize("kind", [ADAM, RMSPROP], ids=["adam", "rmsprop"])
@pytest.mark.parametrize("P", [1, 1027, 70001])
def test_one_run_equals_the_flat_step_bit_for_bit(P, kind, max_norm, shift):
    hp = hparams(kind, max_norm)
    a, b = Buffers(P, shift, 5 + P, kind), Buffers(P, shift, 5 + P, kind)
    table = run_table([(0, P, 0, 1)])
    rng = np.random.default_rng(P)
    for step in range(2):
        if step:  # a fresh gradient for the second step (the first one zeroed it)
            g = torch.from_numpy(rng.standard_normal(P).astype(np.float32)).to(DEV)
            a.g.copy_(g)
            b.g.copy_(g)
        a.flat_step(hp)
        b.runs_step(hp, table, 1)
        sa, sb = a.snapshot(), b.snapshot()
        for name, x, y in zip(("params", "grads", "m", "v", "norms", "state"), sa, sb):
            assert torch.equal(x, y), (name, step)
        assert not sb[1].any(), "gradients zeroed"
        assert int(sb[5][:8].view(torch.int64)[0]) == 3 + step + 1, "opt_step"
        if P > 1:  # (the norm of a one-element gradient may be below the clip threshold)
            assert float(sb[4][step]) > 0.5


# frozen pattern per step (1: the run sits the step out); run 2 is frozen on step 1: it starts from absent state
FROZEN = {
    4: [(0, 0, 1, 0), (1, 0, 1, 0), (0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 1, 1), (0, 0, 0, 0)],
    3: [(0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 0), (0, 0, 0)],
}
SPLITS = {1027: [0, 3, 130, 131, 1027], 70001: [0, 4097, 50002, 70001]}


def torch_reference(kind, cuts, init, grads, dtype):
    """torch.optim + clip_grad_norm_ over one tensor per run, .grad = None where frozen."""
    nr = len(cuts) - 1
    ps = [torch.nn.Parameter(torch.from_numpy(init[cuts[k]:cuts[k + 1]]).to(dtype)) for k in range(nr)]
    if kind == ADAM:
        opt = torch.optim.Adam(ps, lr=LR, eps=1e-7)
    else:
        opt = torch.optim.RMSprop(ps, lr=LR, alpha=0.99, eps=1e-5)
    rec = []
    for s, frz in enumerate(FROZEN[nr]):
        for k, p in enumerate(ps):
            p.grad = None if frz[k] else torch.from_numpy(grads[s][cuts[k]:cuts[k + 1]]).to(dtype)
        norm = torch.nn.utils.clip_grad_norm_(ps, 0.5)
        opt.step()
        zeros = lambda p: torch.zeros_like(p)
        st = [opt.state.get(p, {}) for p in ps]
        k1, k2 = ("exp_avg", "exp_avg_sq") if kind == ADAM else ("square_avg", "square_avg")
        cat = lambda ts: torch.cat([t.detach().double() for t in ts]).numpy()
        rec.append(dict(p=cat(ps), m=cat([s_.get(k1, zeros(p)) for s_, p in zip(st, ps)]),
                        v=cat([s_.get(k2, zeros(p)) for s_, p in zip(st, ps)]), norm=float(norm)))
    return rec


def per_run(err, cuts):
    """|f32 - f64| per tensor (run): the maximum over its elements, spread back over them.  One element's own
    difference is a single draw of the rounding (it can be 0 where the float32 sequence happens to land on the
    float64 value); the tensor's maximum is the reference's rounding at that tensor's scale, as the
    fixtures' per-tensor `_err` of the parameters."""
    return np.concatenate([np.full(b - a, err[a:b].max()) for a, b in zip(cuts[:-1], cuts[1:])])


@pytest.mark.parametrize("kind", [ADAM, RMSPROP], ids=["adam", "rmsprop"])
@pytest.mark.parametrize("P", [1027, 70001])
def test_runs_match_torch_per_tensor_semantics(P, kind):
    cuts = SPLITS[P]
    nr = len(cuts) - 1
    rng = np.random.default_rng(100 + P + kind)
    init = rng.standard_normal(P).astype(np.float32)
    grads = [(rng.standard_normal(P) * 0.05).astype(np.float32) for _ in range(6)]
    grads[3] *= 0.01  # one step whose norm is below the clip threshold
    r32 = torch_reference(kind, cuts, init, grads, torch.float32)
    r64 = torch_reference(kind, cuts, init, grads, torch.float64)
    hp = hparams(kind, 0.5)
    b = Buffers(P, 0, 1, kind)
    b.p.copy_(torch.from_numpy(init))
    b.m.zero_()
    b.v.zero_()
    b.state = struct_to_device(_lib.TrainState(opt_step=0), DEV)
    table = run_table([(0, P, 0, 1)])
    lag = [0] * nr
    for s, frz in enumerate(FROZEN[nr]):
        b.g.copy_(torch.from_numpy(grads[s]))
        run_table([(cuts[k], cuts[k + 1], lag[k], 0 if frz[k] else 1) for k in range(nr)], out=table)  # the host rewrites
        before = b.snapshot()
        b.runs_step(hp, table, nr)
        after = b.snapshot()
        for k in range(nr):
            if frz[k]:
                lag[k] += 1
                sl = slice(cuts[k], cuts[k + 1])
                for i in (0, 2, 3):
                    assert torch.equal(after[i][sl], before[i][sl]), ("frozen run touched", s, k, i)
        assert not after[1].any(), "every gradient zeroed, frozen runs included"
        what = (P, "adam" if kind == ADAM else "rmsprop", s)
        for name, i in (("p", 0), ("m", 2)) + ((("v", 3),) if kind == ADAM else ()):
            assert_close(after[i].cpu().numpy(), r64[s][name], per_run(np.abs(r32[s][name] - r64[s][name]), cuts),
                         what + (name,))
        assert_close(float(after[4][s]), r64[s]["norm"], abs(r32[s]["norm"] - r64[s]["norm"]), what + ("norm",))
    assert len(set(lag)) > 1, "the runs reached different lags"
    assert int(after[5][:8].view(torch.int64)[0]) == 6


def test_error_codes_launch_nothing():
    P = 1027
    hp = hparams(ADAM, 0.5)
    b = Buffers(P, 0, 9, ADAM)
    table = run_table([(0, P, 0, 1)])
    before = b.snapshot()
    L = _lib.lib()
    a, t = b.args(hp), b.tail()
    E_NULL, E_SHAPE, E_WS = _lib.RAI_E_NULLPTR, _lib.RAI_E_SHAPE, _lib.RAI_E_WORKSPACE
    assert L.rai_clip_optim_step_runs(*a, table.data_ptr(), 0, *t) == E_SHAPE
    assert L.rai_clip_optim_step_runs(*a, table.data_ptr(), _lib.RAI_OPTIM_MAX_RUNS + 1, *t) == E_SHAPE
    assert L.rai_clip_optim_step_runs(*a, None, 1, *t) == E_NULL
    for i in (0, 1, 2, 5, 6):  # params, grads, state1, hp, state (a NULL state2 is RMSprop's layout)
        bad = list(a)
        bad[i] = None
        assert L.rai_clip_optim_step_runs(*bad, table.data_ptr(), 1, *t) == E_NULL, i
    assert L.rai_clip_optim_step_runs(*a, table.data_ptr(), 1, t[0], t[1], None, t[3], t[4]) == E_NULL
    assert L.rai_clip_optim_step_runs(*a, table.data_ptr(), 1, t[0], t[1], t[2], t[3] - 8, t[4]) == E_WS
    assert L.rai_optim_workspace_bytes(P) == b.ws.numel()
    for x, y in zip(before, b.snapshot()):
        assert torch.equal(x, y), "an error return launched something"
