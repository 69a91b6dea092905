"""MultiDiscrete actor head operators over csrc/multidiscrete.hip (rl_algo_impls/shared/actor/multi_discrete.py
over shared/actor/categorical.py MaskedCategorical).

`MdHeadLogpEntropy` is the update path's (logp, entropy) of a minibatch from the head's final Linear input:
ONE launch forward (rai_md_head_fwd: the Linear, the masked per-group log-softmax, log-prob and entropy) and
two backward (rai_md_head_bwd), through a torch.autograd.Function like sde_ops.SdeLogpEntropy.  Inside the
trainer's cnn_ops.direct_grads() the weight and bias gradients are added straight into their flat .grad views.
`logits` is the same kernel without actions (the rollout's forward), `sample` the rollout's one launch.
`logp_entropy_torch` is the same formula in plain torch (CPU, or shapes outside the kernels' limits).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib


def in_limits(H: int, nvec: Sequence[int]) -> bool:
    return (1 <= H <= _lib.RAI_MD_MAX_H and 1 <= len(nvec) <= _lib.RAI_MD_MAX_G
            and sum(int(n) for n in nvec) <= _lib.RAI_GRID_MAX_A)


def nvec_array(nvec: Sequence[int]):
    return (C.c_int32 * len(nvec))(*[int(n) for n in nvec])


def _u8(m: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if m is None:
        return None
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


def logp_entropy_torch(logits, nvec: Sequence[int], actions, action_masks=None):
    """MultiCategorical.log_prob / entropy written out (no torch.distributions validation): per group,
    MaskedCategorical's masked logits (finfo.min), normalised by the group's own logsumexp; the masked
    entropy form -sum_valid p logp with a mask, Categorical.entropy without."""
    sizes = [int(n) for n in nvec]
    fmin = torch.finfo(logits.dtype).min
    actions = actions.long().reshape(logits.shape[0], len(sizes))
    masks = torch.split(action_masks, sizes, dim=1) if action_masks is not None else [None] * len(sizes)
    logp, ent = [], []
    for g, (lg, m) in enumerate(zip(torch.split(logits, sizes, dim=1), masks)):
        if m is not None:
            lg = torch.where(m, lg, fmin)
        norm = lg - lg.logsumexp(dim=-1, keepdim=True)
        probs = torch.softmax(norm, dim=-1)
        logp.append(norm.gather(-1, actions[:, g:g + 1]).squeeze(-1))
        if m is None:
            ent.append(-(torch.clamp(norm, min=fmin) * probs).sum(-1))
        else:
            ent.append(-torch.where(m, norm * probs, torch.zeros((), dtype=norm.dtype, device=norm.device)).sum(-1))
    return torch.stack(logp, dim=-1).sum(dim=-1), torch.stack(ent, dim=-1).sum(dim=-1)


class MdHeadLogpEntropy(torch.autograd.Function):
    """(x (B, H), W (A, H), b (A), actions (B, G), masks (B, A) | None, nvec) -> (logp (B,), entropy (B,))."""

    @staticmethod
    def forward(ctx, x, W, b, actions, masks, nvec):
        from .cnn_ops import _direct

        _lib.require_device(x, W, b, actions, masks)
        B, H, A, G = int(x.shape[0]), int(x.shape[1]), int(W.shape[0]), len(nvec)
        xc, Wc, bc = x.contiguous(), W.contiguous(), b.contiguous()
        act = actions.long().reshape(B, G).contiguous()
        m = _u8(masks)
        logits = torch.empty((B, A), dtype=torch.float32, device=x.device)
        logp = torch.empty(B, dtype=torch.float32, device=x.device)
        ent = torch.empty_like(logp)
        rc = _lib.lib().rai_md_head_fwd(xc.data_ptr(), Wc.data_ptr(), bc.data_ptr(), _lib.ptr(m), act.data_ptr(),
                                        nvec_array(nvec), G, B, H, logits.data_ptr(), logp.data_ptr(),
                                        ent.data_ptr(), _lib.stream_handle(x.device))
        _lib.check(rc, "rai_md_head_fwd")
        ctx.save_for_backward(xc, W, b, logits, act, m if m is not None else torch.empty(0, dtype=torch.uint8,
                                                                                        device=x.device))
        ctx.nvec, ctx.has_mask = tuple(int(n) for n in nvec), m is not None
        # decided here: autograd runs the backward on its device thread, where direct_grads() is not visible
        ctx.direct = (W.is_contiguous() and b.is_contiguous() and _direct(W, raw=True) and _direct(b, raw=True))
        return logp, ent

    @staticmethod
    def backward(ctx, d_logp, d_ent):
        from .dp_buckets import notify_grad_written

        x, W, b, logits, act, m = ctx.saved_tensors
        nvec = ctx.nvec
        B, H, A = int(x.shape[0]), int(x.shape[1]), int(W.shape[0])
        dev = x.device
        z = lambda t: t.contiguous().float() if t is not None else torch.zeros(B, dtype=torch.float32, device=dev)
        gl, ge = z(d_logp), z(d_ent)
        dx = torch.empty_like(x)
        d_logits = torch.empty((B, A), dtype=torch.float32, device=dev)
        if ctx.direct:
            dW, db = W.grad, b.grad
        else:
            dW = torch.empty((A, H), dtype=torch.float32, device=dev)
            db = torch.empty(A, dtype=torch.float32, device=dev)
        rc = _lib.lib().rai_md_head_bwd(x.data_ptr(), W.contiguous().data_ptr(), logits.data_ptr(),
                                        m.data_ptr() if ctx.has_mask else None, act.data_ptr(), nvec_array(nvec),
                                        len(nvec), gl.data_ptr(), ge.data_ptr(), B, H, d_logits.data_ptr(),
                                        dx.data_ptr(), dW.data_ptr(), db.data_ptr(), 1 if ctx.direct else 0,
                                        _lib.stream_handle(dev))
        _lib.check(rc, "rai_md_head_bwd")
        if ctx.direct:
            notify_grad_written(W)
            notify_grad_written(b)
            return dx, None, None, None, None, None
        return dx, dW, db, None, None, None


def fusable(x: torch.Tensor, lin: torch.nn.Linear, nvec: Sequence[int]) -> bool:
    """The head kernels apply: float32 rows on the GPU, contiguous, a Linear with a bias, within the limits."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and lin.bias is not None
            and lin.weight.is_contiguous() and lin.weight.dtype == torch.float32
            and in_limits(int(x.shape[1]), nvec))


def logits(x: torch.Tensor, lin: torch.nn.Linear, nvec: Sequence[int]) -> torch.Tensor:
    """The head's logits by rai_md_head_fwd (no actions: logits only, no gradient): what the rollout samples
    from, the same bits the update's forward recomputes."""
    B, H, A = int(x.shape[0]), int(x.shape[1]), int(lin.weight.shape[0])
    out = torch.empty((B, A), dtype=torch.float32, device=x.device)
    W, b = lin.weight.detach(), lin.bias.detach().contiguous()
    rc = _lib.lib().rai_md_head_fwd(x.data_ptr(), W.data_ptr(), b.data_ptr(), None, None, nvec_array(nvec),
                                    len(nvec), B, H, out.data_ptr(), None, None, _lib.stream_handle(x.device))
    _lib.check(rc, "rai_md_head_fwd")
    return out


def sample(logits_: torch.Tensor, masks: Optional[torch.Tensor], nvec: Sequence[int], seed: int, offset: int,
           actions: torch.Tensor, logp: torch.Tensor, v_in=None, v_out=None, K: int = 1) -> None:
    """actions (N, G) int64 / logp (N) (and the value pass-through) of one env step (rai_md_sample)."""
    assert logits_.is_contiguous() and actions.is_contiguous() and logp.is_contiguous()
    m = _u8(masks)
    rc = _lib.lib().rai_md_sample(logits_.data_ptr(), _lib.ptr(m), nvec_array(nvec), len(nvec),
                                  int(logits_.shape[0]), seed, offset, actions.data_ptr(), logp.data_ptr(),
                                  _lib.ptr(v_in), _lib.ptr(v_out), K, _lib.stream_handle(logits_.device))
    _lib.check(rc, "rai_md_sample")
