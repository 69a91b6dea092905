"""References for rai_chan_ln_fwd / _bwd (csrc/chan_norm.hip), shared by
tests/test_gpu_chan_norm_kernels.py and tools/chan_norm_bench.py: seeded inputs, the formula in float64
(numpy), the same formula in float32 (torch on the CPU, autograd for the backward) whose error against
float64 sets the tolerance, and the call into the raw kernels."""
import math

import numpy as np
import torch

EPS = 1e-5
NAMES = ("out", "mean", "rstd", "dx", "dgamma", "dbeta", "dbias")


def make_inputs(rows, C, seed):
    """x (rows, C): unit normal rows; every third row has a large common offset (mean 100, std 1:
    E[z^2] - mean^2 loses all digits there); with more than two rows, row rows // 2 is constant after
    the bias (var = 0: rstd = eps^-1/2, y = beta).  bias in multiples of 1/8 so that the constant row
    is exactly constant in float32.  gamma = 1 + 0.5 N, beta = 0.5 N, dout = N."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g)
    x[1::3] += 100.0
    bias = torch.round(torch.randn(C, generator=g) * 8) / 8
    if rows > 2:
        x[rows // 2] = 3.0 - bias
    gamma = 1 + 0.5 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    dout = torch.randn(rows, C, generator=g)
    return x, bias, gamma, beta, dout


def ref64(x, bias, gamma, beta, dout, gelu):
    """The formula in float64 on the float32 inputs."""
    x, bias, gamma, beta, dout = (t.double().numpy() for t in (x, bias, gamma, beta, dout))
    C = x.shape[1]
    z = x + bias
    mean = z.mean(1, keepdims=True)
    var = ((z - mean) ** 2).sum(1, keepdims=True) / (C - 1)
    rstd = 1 / np.sqrt(var + EPS)
    xh = (z - mean) * rstd
    y = gamma * xh + beta
    if gelu:
        cdf = 0.5 * (1 + torch.erf(torch.from_numpy(y / math.sqrt(2))).numpy())  # float64 erf
        out = y * cdf
        dy = dout * (cdf + y * np.exp(-0.5 * y * y) / math.sqrt(2 * math.pi))
    else:
        out, dy = y, dout
    gg = dy * gamma
    dx = rstd * (gg - gg.mean(1, keepdims=True) - xh * (gg * xh).sum(1, keepdims=True) / (C - 1))
    return dict(out=out, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0),
                dbias=dx.sum(0))


def torch32(x, bias, gamma, beta, dout, gelu):
    """The torch composition the kernels replace, float32 on the CPU: bias add, the reference module's
    formula, GELU, autograd's backward."""
    x, bias, gamma, beta = (t.clone().requires_grad_() for t in (x, bias, gamma, beta))
    z = x + bias
    mean = z.mean(dim=1, keepdim=True)
    var = z.var(dim=1, keepdim=True)
    y = gamma * (z - mean) / torch.sqrt(var + EPS) + beta
    out = torch.nn.functional.gelu(y) if gelu else y
    out.backward(dout)
    n = lambda t: t.detach().numpy()
    return dict(out=n(out), mean=n(mean)[:, 0], rstd=n(1 / torch.sqrt(var + EPS))[:, 0], dx=n(x.grad),
                dgamma=n(gamma.grad), dbeta=n(beta.grad), dbias=n(bias.grad))


def run_kernels(x, bias, gamma, beta, dout, gelu, dev, repeat_bwd=1):
    """The raw kernels through _lib.  bias / gamma / beta are placed one float into a larger buffer
    (4-byte aligned only, like views into the flat parameter buffer).  Returns the arrays of NAMES on
    the host, one dict per backward launch."""
    from rl_algo_impls_amd import _lib

    rows, C = x.shape
    L, st = _lib.lib(), _lib.stream_handle(dev)
    par = torch.zeros(3 * C + 5, device=dev)
    b, g, be = par[1:1 + C], par[1 + C:1 + 2 * C], par[1 + 2 * C:1 + 3 * C]
    b.copy_(bias), g.copy_(gamma), be.copy_(beta)
    assert b.data_ptr() % 16 == 4
    xd, dd = x.to(dev), dout.to(dev)
    out, stats = torch.empty_like(xd), torch.empty(rows, 2, device=dev)
    _lib.check(L.rai_chan_ln_fwd(xd.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), rows, C, EPS, int(gelu),
                                 out.data_ptr(), stats.data_ptr(), st), "rai_chan_ln_fwd")
    nb = int(L.rai_chan_ln_workspace_bytes(C))
    res = []
    for _ in range(repeat_bwd):
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        dx = torch.full_like(xd, float("nan"))
        dpar = torch.full((3, C), float("nan"), device=dev)
        _lib.check(L.rai_chan_ln_bwd(dd.data_ptr(), xd.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(),
                                     stats.data_ptr(), rows, C, int(gelu), dx.data_ptr(), dpar[0].data_ptr(),
                                     dpar[1].data_ptr(), dpar[2].data_ptr(), ws.data_ptr(), nb, st),
                   "rai_chan_ln_bwd")
        h = lambda t: t.cpu().numpy()
        res.append(dict(out=h(out), mean=h(stats[:, 0]), rstd=h(stats[:, 1]), dx=h(dx), dgamma=h(dpar[0]),
                        dbeta=h(dpar[1]), dbias=h(dpar[2])))
    return res


def errors(got, t32, r64):
    """Per array: (kernel max error, torch float32 max error, bound = 4 x torch's + one float32 ulp of
    the array's largest magnitude)."""
    out = {}
    for k in NAMES:
        e_t = float(np.abs(t32[k].astype(np.float64) - r64[k]).max())
        e_k = float(np.abs(got[k].astype(np.float64) - r64[k]).max())
        ulp = float(np.spacing(np.float32(np.abs(r64[k]).max())))
        out[k] = (e_k, e_t, 4 * e_t + ulp)
    return out
