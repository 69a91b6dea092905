"""Plain-torch references for the CNN policies' head and epilogue kernels (csrc/heads.hip and the bias / SE
epilogues of csrc/se_block.hip), written from include/rai_amd.h's descriptions of the operations, for
tests/test_gpu_cnn_epilogue_kernels.py.  Every function is generic in dtype and device: run on float64 CPU
tensors it is the reference, run on float32 device tensors it is the comparator whose error against
float64 sets the tolerance.

    heads      logits = enc Wpi^T + bpi;  v = enc wv + bv;  n = logits - logsumexp(logits);
               logp = n[action];  H = -sum(clamp(n, min=finfo.min) * softmax(n))
               gradients of sum_b d_logp logp + d_entropy H + d_v v by autograd
               _bwd_relu:  dz = where(enc <= 0, 0, d_enc);  g_benc = dz.sum(0)
    bias_relu  y = relu(x + b);  dx = where(y <= 0, 0, dy) (threshold_backward);  db = dx.sum(rows)
    _nchw      x, dx NHWC (B, HW, C);  y, dy in nn.Flatten's order (B, C * HW)
    bias_gelu  y = gelu(x + b) (erf form);  dx = dy * gelu'(x + b)
    se_residual  out = gelu(x + r * s[b, c]);  dx, dr, ds by autograd
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TAILS = (-12.0, -8.0, -5.0, -1.0, -0.0, 0.0, 1.0, 5.0, 8.0, 12.0)  # erff saturates, expf underflows


def to(ts, dtype, device="cpu"):
    """Fresh copies (a caller's tensor is never made a leaf or written)."""
    return [t.detach().to(device=device, dtype=dtype if t.is_floating_point() else t.dtype, copy=True) for t in ts]


def _det(t):
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------
def heads_forward(enc, wpi, bpi, wv, bv, actions):
    """torch.distributions.Categorical(logits=...) arithmetic on the actor's logits, and the critic."""
    logits = enc @ wpi.t() + bpi
    v = enc @ wv.reshape(-1) + bv.reshape(())
    n = logits - logits.logsumexp(dim=-1, keepdim=True)
    p = torch.softmax(n, dim=-1)
    logp = n.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    ent = -(torch.clamp(n, min=torch.finfo(n.dtype).min) * p).sum(-1)
    return logits, logp, ent, v


def make_heads_inputs(B, D, A, logit_scale, seed):
    """float32 CPU tensors: enc (B, D) unit normal; Wpi (A, D) such that the logits are N(0, logit_scale^2);
    bpi, wv (D), bv; actions; the three cotangents."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    enc = rn(B, D)
    wpi, bpi = rn(A, D) * (logit_scale / D ** 0.5), 0.1 * rn(A)
    wv, bv = rn(D) / D ** 0.5, 0.1 * rn(1)
    actions = torch.randint(0, A, (B,), generator=g)
    cot = (rn(B), rn(B), rn(B))
    return SimpleNamespace(enc=enc, wpi=wpi, bpi=bpi, wv=wv, bv=bv, actions=actions, cot=cot)


def run_heads(inp, dtype, device="cpu", relu=False):
    """Forward and gradients in `dtype` on `device`, returned as float64 CPU tensors.  relu: enc is taken
    as the output of a ReLU (inp.enc clamped at zero: dead units) and dz / g_benc are returned too."""
    enc, wpi, bpi, wv, bv, actions = to([inp.enc, inp.wpi, inp.bpi, inp.wv, inp.bv, inp.actions], dtype, device)
    if relu:
        enc = torch.relu(enc)
    leaves = [t.requires_grad_(True) for t in (enc, wpi, bpi, wv, bv)]
    d_logp, d_ent, d_v = to(inp.cot, dtype, device)
    logits, logp, ent, v = heads_forward(*leaves, actions)
    grads = torch.autograd.grad((d_logp * logp).sum() + (d_ent * ent).sum() + (d_v * v).sum(), leaves)
    out = SimpleNamespace(logits=_det(logits), logp=_det(logp), ent=_det(ent), v=_det(v), d_enc=_det(grads[0]),
                          g_wpi=_det(grads[1]), g_bpi=_det(grads[2]), g_wv=_det(grads[3]), g_bv=_det(grads[4]),
                          finite=all(bool(torch.isfinite(t).all()) for t in (logits, logp, ent, v) + tuple(grads)))
    if relu:
        dz = torch.where(enc.detach() <= 0, torch.zeros((), dtype=dtype, device=device), grads[0])
        out.dz, out.g_benc = _det(dz), _det(dz.sum(0))
    return out


# ---------------------------------------------------------------------------------------------------
# bias + ReLU
# ---------------------------------------------------------------------------------------------------
def bias_relu_fwd(x, b):
    return torch.relu(x + b)


def bias_relu_bwd(dy, y):
    """threshold_backward on the saved output, and its column sums."""
    dx = torch.where(y <= 0, torch.zeros((), dtype=dy.dtype, device=dy.device), dy)
    return dx, dx.reshape(-1, dx.shape[-1]).sum(0)


def bias_relu_fwd_nchw(x, b):
    """x NHWC (B, HW, C) -> relu(x + b) in the order nn.Flatten gives a (B, C, H, W) tensor: (B, C * HW)."""
    B, HW, C = x.shape
    return torch.relu(x + b).permute(0, 2, 1).reshape(B, C * HW)


def bias_relu_bwd_nchw(dy, y, HW, C):
    """dy, y (B, C * HW) -> dx NHWC (B, HW, C) and db (C)."""
    B = dy.shape[0]
    dflat = torch.where(y <= 0, torch.zeros((), dtype=dy.dtype, device=dy.device), dy)
    dx = dflat.view(B, C, HW).permute(0, 2, 1).contiguous()
    return dx, dx.sum((0, 1))


# ---------------------------------------------------------------------------------------------------
# bias + GELU, SE residual
# ---------------------------------------------------------------------------------------------------
def tail_inputs(shape, b, seed):
    """3 * randn of `shape` (channels last), its first elements forced into the GELU's tails: first TAILS
    itself (cycled over max(10, C) elements: the values before the bias), then, where b is given,
    TAILS - b (b in multiples of 1/8, so that x + b is TAILS exactly)."""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(*shape, generator=g)
    flat, C = x.view(-1), shape[-1]
    k = min(flat.numel(), max(len(TAILS), C))
    t = torch.tensor(TAILS).repeat(k // len(TAILS) + 1)
    flat[:k] = t[:k]
    if b is not None and flat.numel() >= 2 * k:
        flat[k:2 * k] = t[:k] - b[(torch.arange(k) + k) % C]
    return x, g


def eighths(C, g):
    return torch.round(torch.randn(C, generator=g) * 8) / 8


def run_bias_gelu(x, b, dy, dtype, device="cpu"):
    x, b, dy = to([x, b, dy], dtype, device)
    x.requires_grad_(True)
    y = F.gelu(x + b)
    (dx,) = torch.autograd.grad(y, x, dy)
    return SimpleNamespace(y=_det(y), dx=_det(dx))


def run_se_residual(x, r, s, dout, dtype, device="cpu", backward=True):
    """x, r, dout (B, HW, C); s (B, C)."""
    x, r, s = to([x, r, s], dtype, device)
    leaves = [t.requires_grad_(True) for t in (x, r, s)]
    out = F.gelu(x + r * s.unsqueeze(1))
    res = SimpleNamespace(out=_det(out))
    if backward:
        dx, dr, ds = torch.autograd.grad(out, leaves, to([dout], dtype, device)[0])
        res.dx, res.dr, res.ds = _det(dx), _det(dr), _det(ds)
    return res
