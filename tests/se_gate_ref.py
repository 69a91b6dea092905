"""Float64 numpy evaluation of the squeeze-excitation gate (csrc/se_gate.hip), the same formula in float32
by torch on the CPU, and a raw-kernel runner, for tests/test_gpu_se_gate_kernels.py.

    pooled = mean_hw r;  hidden = W1 pooled;  a = GELU(hidden);  s = sigmoid(W2 a)
    dz2 = ds s (1 - s);  da = W2^T dz2;  dh = da GELU'(hidden);  dpool = W1^T dh
    dr = dr0 + dpool / HW (every pixel);  dW2 = sum_b dz2 (x) a;  dW1 = sum_b dh (x) pooled
"""
import math

import numpy as np
import torch

DR_PATTERN = 0.5  # dr is pre-filled with DR_PATTERN * (a seeded normal): the add must keep it


def make_inputs(B, HW, C, seed):
    """r (B, HW, C) unit normal, every third sample with a common offset of 100; W1 (M, C), W2 (C, M) scaled
    like nn.Linear's default init; ds (B, C); dr0 (B, HW, C) the pattern dr holds on entry."""
    g = torch.Generator().manual_seed(seed)
    M = C // 16
    r = torch.randn(B, HW, C, generator=g)
    r[2::3] += 100.0
    w1 = (torch.rand(M, C, generator=g) * 2 - 1) / math.sqrt(C)
    w2 = (torch.rand(C, M, generator=g) * 2 - 1) / math.sqrt(M)
    ds = torch.randn(B, C, generator=g)
    dr0 = DR_PATTERN * torch.randn(B, HW, C, generator=g)
    return r, w1, w2, ds, dr0


def _erf64(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def ref64(r, w1, w2, ds, dr0):
    r, w1, w2, ds, dr0 = (t.double().numpy() for t in (r, w1, w2, ds, dr0))
    HW = r.shape[1]
    pooled = r.mean(1)
    hidden = pooled @ w1.T
    cdf = 0.5 * (1 + _erf64(hidden / math.sqrt(2)))
    a = hidden * cdf
    s = 1 / (1 + np.exp(-(a @ w2.T)))
    dz2 = ds * s * (1 - s)
    da = dz2 @ w2
    dh = da * (cdf + hidden * np.exp(-0.5 * hidden ** 2) / math.sqrt(2 * math.pi))
    dpool = dh @ w1
    return dict(pooled=pooled, hidden=hidden, s=s, dr=dr0 + dpool[:, None, :] / HW, dw1=dh.T @ pooled,
                dw2=dz2.T @ a)


def torch32(r, w1, w2, ds, dr0):
    """The torch composition of SqueezeExcitation's gate and its autograd in float32 on the CPU."""
    r = r.clone().requires_grad_()
    w1 = w1.clone().requires_grad_()
    w2 = w2.clone().requires_grad_()
    pooled = r.mean(1)
    hidden = pooled @ w1.T
    s = torch.sigmoid(torch.nn.functional.gelu(hidden) @ w2.T)
    dr, dw1, dw2 = torch.autograd.grad(s, (r, w1, w2), ds)
    return {k: v.detach().numpy() for k, v in dict(pooled=pooled, hidden=hidden, s=s, dr=dr0 + dr, dw1=dw1,
                                                    dw2=dw2).items()}


def _offset(t, dev):
    """t's values one float into a larger device buffer (4-byte aligned only, as a flat-parameter view)."""
    buf = torch.zeros(t.numel() + 8, device=dev)
    buf[1:1 + t.numel()] = t.reshape(-1).to(dev)
    return buf, buf.data_ptr() + 4


def run_kernels(r, w1, w2, ds, dr0, dev, repeat_bwd=1):
    """rai_se_gate_fwd, then rai_se_gate_bwd `repeat_bwd` times on fresh copies of dr0 (NaN-filled outputs
    and workspace).  Returns one dict of numpy arrays per backward call."""
    from rl_algo_impls_amd import _lib

    L, st = _lib.lib(), _lib.stream_handle(dev)
    B, HW, C = r.shape
    M = C // 16
    rd, dsd = r.to(dev).contiguous(), ds.to(dev).contiguous()
    (b1, p1), (b2, p2) = _offset(w1, dev), _offset(w2, dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    s, pooled, hidden = nan(B, C), nan(B, C), nan(B, M)
    _lib.check(L.rai_se_gate_fwd(rd.data_ptr(), p1, p2, B, C, HW, M, s.data_ptr(), pooled.data_ptr(),
                                 hidden.data_ptr(), st), "rai_se_gate_fwd")
    nb = int(L.rai_se_gate_workspace_bytes(C))
    outs = []
    for _ in range(repeat_bwd):
        dr = dr0.to(dev).contiguous()
        dw1, dw2 = nan(M, C), nan(C, M)
        ws = torch.full((nb // 4,), float("nan"), device=dev)
        _lib.check(L.rai_se_gate_bwd(dsd.data_ptr(), s.data_ptr(), pooled.data_ptr(), hidden.data_ptr(), p1, p2, B, C,
                                     HW, M, dr.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), ws.data_ptr(), nb, st),
                   "rai_se_gate_bwd")
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in dict(pooled=pooled, hidden=hidden, s=s, dr=dr, dw1=dw1,
                                                          dw2=dw2).items()})
    assert bool((b1[0] == 0) & (b1[-1] == 0) & (b2[0] == 0) & (b2[-1] == 0))  # the weights' neighbours untouched
    return outs


def errors(got, t32, r64):
    """key -> (kernel max error, torch-float32 max error, bound): 4 x torch's error + one float32 ulp of the
    array's largest magnitude."""
    out = {}
    for k, ref in r64.items():
        e_k = float(np.abs(got[k].astype(np.float64) - ref).max())
        e_t = float(np.abs(t32[k].astype(np.float64) - ref).max())
        ulp = float(np.spacing(np.float32(np.abs(ref).max())))
        out[k] = (e_k, e_t, 4 * e_t + ulp)
    return out


def bias_gelu_add_ref64(x, b, skip):
    z = x.double().numpy() + b.double().numpy()
    return skip.double().numpy() + 0.5 * z * (1 + _erf64(z / math.sqrt(2)))
