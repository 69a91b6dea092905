"""gSDE actor head operators over csrc/sde.hip (rl_algo_impls/shared/actor/state_dependent_noise.py).

`SdeLogpEntropy` is the update path's (logp, entropy) of a minibatch: ONE launch forward
(rai_sde_head_fwd) and ONE backward (rai_sde_head_bwd) in place of the 10-20 small torch kernels of
the distribution formula and its autograd, through a torch.autograd.Function like
gridnet.GridnetLogpEntropy.  Inside the trainer's cnn_ops.direct_grads() the log_std gradient is added
straight into its flat .grad view.  `sample_weights` / `sample` are the rollout's two launches.
`logp_entropy_torch` is the same formula in plain torch (CPU, or shapes outside the kernels' limits).
"""
from __future__ import annotations

import math

import torch

from . import _lib

F32_EPS = float(torch.finfo(torch.float32).eps)


def in_limits(H: int, A: int) -> bool:
    return 1 <= H <= _lib.RAI_SDE_MAX_H and 1 <= A <= _lib.RAI_SDE_MAX_A


def atanh_clamped(a: torch.Tensor) -> torch.Tensor:
    """TanhBijector.inverse: the clamp uses the tensor dtype's machine epsilon."""
    eps = torch.finfo(a.dtype).eps
    return torch.atanh(a.clamp(min=-1.0 + eps, max=1.0 - eps))


def logp_entropy_torch(mu, log_std, latent, actions, full_std: bool, squash: bool):
    """StateDependentNoiseDistribution.log_prob and pi_forward's entropy, written out (no
    torch.distributions validation).  latent carries no gradient (learn_std is never set)."""
    latent = latent.detach()
    std = torch.exp(log_std)
    if not full_std:
        std = torch.ones(log_std.shape[0], mu.shape[-1], dtype=std.dtype, device=std.device) * std
    sigma = torch.sqrt(torch.mm(latent ** 2, std ** 2) + 1e-6)
    g = atanh_clamped(actions) if squash else actions
    log_sigma = sigma.log()
    logp = (-((g - mu) ** 2) / (2 * sigma ** 2) - log_sigma - math.log(math.sqrt(2 * math.pi))).sum(dim=1)
    if squash:
        logp = logp - torch.log(1.0 - torch.tanh(g) ** 2 + 1e-6).sum(dim=1)
        return logp, -logp
    return logp, (0.5 + 0.5 * math.log(2 * math.pi) + log_sigma).sum(dim=1)


class SdeLogpEntropy(torch.autograd.Function):
    """(mu (B, A), log_std (H, A | 1), latent (B, H), actions (B, A)) -> (logp (B,), entropy (B,))."""

    @staticmethod
    def forward(ctx, mu, log_std, latent, actions, full_std: bool, squash: bool):
        from .cnn_ops import _direct

        _lib.require_device(mu, log_std, latent, actions)
        B, A, H = int(mu.shape[0]), int(mu.shape[1]), int(latent.shape[1])
        mu_c, ls, lat, act = mu.contiguous(), log_std.contiguous(), latent.contiguous(), actions.contiguous().float()
        logp = torch.empty(B, dtype=torch.float32, device=mu.device)
        ent = torch.empty_like(logp)
        sigma = torch.empty((B, A), dtype=torch.float32, device=mu.device)
        rc = _lib.lib().rai_sde_head_fwd(lat.data_ptr(), mu_c.data_ptr(), ls.data_ptr(), act.data_ptr(), B, H, A,
                                         int(full_std), int(squash), logp.data_ptr(), ent.data_ptr(),
                                         sigma.data_ptr(), _lib.stream_handle(mu.device))
        _lib.check(rc, "rai_sde_head_fwd")
        ctx.save_for_backward(mu_c, log_std, lat, act, sigma)
        ctx.conf = (bool(full_std), bool(squash))
        # decided here: autograd runs the backward on its device thread, where direct_grads() is not visible
        ctx.direct = log_std.is_contiguous() and _direct(log_std, raw=True)
        return logp, ent

    @staticmethod
    def backward(ctx, d_logp, d_ent):
        from .dp_buckets import notify_grad_written

        mu, log_std, lat, act, sigma = ctx.saved_tensors
        full_std, squash = ctx.conf
        B, A, H = int(mu.shape[0]), int(mu.shape[1]), int(lat.shape[1])
        dev = mu.device
        z = lambda t: t.contiguous().float() if t is not None else torch.zeros(B, dtype=torch.float32, device=dev)
        gl, ge = z(d_logp), z(d_ent)
        d_mu = torch.empty_like(mu)
        d_ls = log_std.grad if ctx.direct else torch.empty_like(log_std, memory_format=torch.contiguous_format)
        rc = _lib.lib().rai_sde_head_bwd(lat.data_ptr(), mu.data_ptr(), log_std.contiguous().data_ptr(), act.data_ptr(),
                                         sigma.data_ptr(), gl.data_ptr(), ge.data_ptr(), B, H, A, int(full_std),
                                         int(squash), d_mu.data_ptr(), d_ls.data_ptr(), 1 if ctx.direct else 0,
                                         _lib.stream_handle(dev))
        _lib.check(rc, "rai_sde_head_bwd")
        if ctx.direct:
            notify_grad_written(log_std)
            return d_mu, None, None, None, None, None
        return d_mu, d_ls, None, None, None, None


def logp_entropy(mu, log_std, latent, actions, full_std: bool, squash: bool):
    """The head kernels on the GPU within their limits, the torch formula elsewhere."""
    if (mu.is_cuda and mu.dtype == torch.float32 and mu.dim() == 2 and latent.dim() == 2
            and in_limits(int(latent.shape[1]), int(mu.shape[1]))):
        return SdeLogpEntropy.apply(mu, log_std, latent.detach(), actions, full_std, squash)
    return logp_entropy_torch(mu, log_std, latent, actions, full_std, squash)


def sample_weights(log_std: torch.Tensor, E: torch.Tensor, E0: torch.Tensor, full_std: bool, seed: int,
                   offset: int) -> None:
    """E (N, H, A) and E0 (H, A) <- exp(log_std) * standard normals keyed by (seed, offset)."""
    N, H, A = (int(d) for d in E.shape)
    assert E.is_contiguous() and E0.is_contiguous() and tuple(E0.shape) == (H, A)
    ls = log_std.detach().contiguous()
    rc = _lib.lib().rai_sde_sample_weights(ls.data_ptr(), N, H, A, int(full_std), seed, offset, E.data_ptr(),
                                           E0.data_ptr(), _lib.stream_handle(E.device))
    _lib.check(rc, "rai_sde_sample_weights")


def sample(mu, latent, log_std, E, per_env: bool, full_std: bool, squash: bool, low, high, actions, clamped, logp,
           v_in=None, v_out=None, K: int = 1) -> None:
    """actions / clamped / logp (and the value pass-through) of one env step (rai_sde_sample); E is the
    (N, H, A) stack when per_env, else one (H, A) matrix used by every row."""
    N, A, H = int(mu.shape[0]), int(mu.shape[1]), int(latent.shape[1])
    ls = log_std.detach().contiguous()
    rc = _lib.lib().rai_sde_sample(mu.data_ptr(), latent.data_ptr(), ls.data_ptr(), E.data_ptr(),
                                   H * A if per_env else 0, N, H, A, int(full_std), int(squash), _lib.ptr(low),
                                   _lib.ptr(high), actions.data_ptr(), _lib.ptr(clamped), logp.data_ptr(),
                                   _lib.ptr(v_in), _lib.ptr(v_out), K, _lib.stream_handle(mu.device))
    _lib.check(rc, "rai_sde_sample")
