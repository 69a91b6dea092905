"""Squeeze-U-Net GridNet actor-critic (MicroRTS, BASELINE config C5) on PyTorch-ROCm.

Mirrors, for state_dict keys, parameter shapes and the seeded initialisation order:

  SqueezeExcitation / SEResidualBlock   rl_algo_impls/shared/policy/actor_critic_network/double_cone.py:18-86
  SqueezeUnetBackbone                    rl_algo_impls/shared/policy/actor_critic_network/squeeze_unet.py:20-195
  SqueezeUnetActorCriticNetwork          squeeze_unet.py:198-270
  BackboneActorCritic (actor head, critic heads, _preprocess, value)
                                         rl_algo_impls/shared/policy/actor_critic_network/backbone_actor_critic.py:31-232

The backbone's convolutions run on MIOpen / hipBLASLt (the north star keeps the CNN contractions on
PyTorch-ROCm).  The GridNet head's log-prob and entropy over every cell and sub-action is the fused
HIP operator of gridnet.py (one launch forward, one backward) instead of the reference's H*W*7
MaskedCategoricals.

`normalization="layer"` (shared/module/normalization.py, channel_layer_norm.py) puts a
ChannelLayerNorm2d after every backbone and critic convolution (unbiased variance over the channels
of each pixel, eps 1e-5) and an nn.LayerNorm after the critic's Linear, at the reference's Sequential
indices.  On NHWC fp32 GPU activations with C in {16, 32, 64, 128, 256} the convolution runs
bias-free and bias + norm + GELU is one HIP pass forward and two launches backward
(rai_chan_ln_fwd / _bwd, csrc/chan_norm.hip); elsewhere (CPU, NCHW, other widths) the modules' own
torch path runs.  `normalization="batch"` / `"batch_renorm"`, the non-shared critic
(`critic_shares_backbone=False`, `save_critic_separate`), the shared critic head and the Lux
`pick_position` action space are outside the hot path and raise NotImplementedError.

DoubleCone (actor_head_style: double_cone; double_cone.py:89-228): DoubleConeBlock (a 4x4 stride-4
convolution down to the cone's map, the cone's SE blocks, two 2x2 transposed convolutions up, and the
skip add), DoubleConeBackbone (in_block, double_cone, out_block) and DoubleConeActorCritic under the same
BackboneActorCritic heads as the squeeze-U-Net, which is now a subclass of it with unchanged keys and
construction order.  The network's SE blocks compute their gate s = sigmoid(W2 . GELU(W1 . mean_hw r))
in ONE launch (rai_se_gate_fwd, csrc/se_gate.hip) and its backward in two, adding into the epilogue's dr
in place (_SETail: two launches forward, three backward, instead of the torch gate's ~5 and ~10);
C % 16 == 0, C / 4 dividing 256, C <= 1024, NHWC fp32 on the GPU, else the torch gate.  SEResidualBlock's
`fused_gate` attribute is off by default: the squeeze-U-Net's blocks keep their path.  RAI_SE_GATE=0 keeps
the torch gate in DoubleCone too.  The cone's last up-convolution adds its skip inside the bias + GELU pass
(rai_bias_gelu_add_fwd).  DoubleCone takes no normalization (the reference passes none on).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from .gridnet import GridnetDistribution, ValueDependentMask

Strides = Sequence[Union[int, Sequence[int]]]
# NHWC activations on the GPU (RAI_SQUNET_NHWC=0 keeps NCHW): MIOpen's implicit-GEMM solvers take
# them without the NCHW<->NHWC transposes, and the fused SE epilogue below runs on them.  (The
# NatureCNN encoder has its own switch, RAI_CHANNELS_LAST, also on by default.)
_CHANNELS_LAST = os.environ.get("RAI_SQUNET_NHWC", "1") == "1"
if _CHANNELS_LAST:
    os.environ.setdefault("PYTORCH_MIOPEN_SUGGEST_NHWC", "1")


def _nhwc(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous(
        memory_format=torch.channels_last)


class _SEResidualEpilogue(torch.autograd.Function):
    """GELU(x + r * s) (double_cone.py:43-47,85-86) as one HIP pass forward and one backward
    (rai_se_residual_fwd / _bwd, csrc/se_block.hip); NHWC fp32 activations, s (B, C)."""

    @staticmethod
    def forward(ctx, x, r, s):
        from . import _lib

        B, C, H, W = (int(d) for d in x.shape)
        s = s.contiguous()
        out = torch.empty_like(x)
        _lib.check(_lib.lib().rai_se_residual_fwd(x.data_ptr(), r.data_ptr(), s.data_ptr(), B, C, H * W,
                                                  out.data_ptr(), _lib.stream_handle(x.device)),
                   "rai_se_residual_fwd")
        ctx.save_for_backward(x, r, s)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import _lib

        x, r, s = ctx.saved_tensors
        B, C, H, W = (int(d) for d in x.shape)
        dout = dout.contiguous(memory_format=torch.channels_last)
        dx, dr, ds = torch.empty_like(x), torch.empty_like(r), torch.empty_like(s)
        _lib.check(_lib.lib().rai_se_residual_bwd(dout.data_ptr(), x.data_ptr(), r.data_ptr(), s.data_ptr(), B, C,
                                                  H * W, dx.data_ptr(), dr.data_ptr(), ds.data_ptr(),
                                                  _lib.stream_handle(x.device)), "rai_se_residual_bwd")
        return dx, dr, ds


class _BiasGelu(torch.autograd.Function):
    """GELU(x + b) over an NHWC conv output (rai_bias_gelu_fwd / _bwd): MIOpen's separate bias pass and
    the GELU kernel in one pass; the bias gradient is the rows-sum of dx."""

    @staticmethod
    def forward(ctx, x, b):
        from . import _lib

        C = int(x.shape[1])
        out = torch.empty_like(x)
        _lib.check(_lib.lib().rai_bias_gelu_fwd(x.data_ptr(), b.data_ptr(), x.numel() // C, C, out.data_ptr(),
                                                _lib.stream_handle(x.device)), "rai_bias_gelu_fwd")
        ctx.save_for_backward(x, b)
        return out

    @staticmethod
    def backward(ctx, dy):
        from . import _lib

        x, b = ctx.saved_tensors
        C = int(x.shape[1])
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().rai_bias_gelu_bwd(dy.data_ptr(), x.data_ptr(), b.data_ptr(), x.numel() // C, C,
                                                dx.data_ptr(), _lib.stream_handle(x.device)), "rai_bias_gelu_bwd")
        # NHWC: dx viewed (rows, C) is contiguous; the bias gradient is its column sum
        db = dx.permute(0, 2, 3, 1).reshape(-1, C).sum(0)
        return dx, db


class _BiasGeluAdd(torch.autograd.Function):
    """skip + GELU(x + b) over an NHWC conv output (rai_bias_gelu_add_fwd): the DoubleCone block's last
    up-convolution and its skip add in one pass.  Backward: dskip = dout, dx by rai_bias_gelu_bwd."""

    @staticmethod
    def forward(ctx, x, b, skip):
        from . import _lib

        C = int(x.shape[1])
        out = torch.empty_like(x)
        _lib.check(_lib.lib().rai_bias_gelu_add_fwd(x.data_ptr(), b.data_ptr(), skip.data_ptr(), x.numel() // C, C,
                                                    out.data_ptr(), _lib.stream_handle(x.device)),
                   "rai_bias_gelu_add_fwd")
        ctx.save_for_backward(x, b)
        return out

    @staticmethod
    def backward(ctx, dy):
        dx, db = _BiasGelu.backward(ctx, dy)
        return dx, db, dy


# The fused squeeze-excitation gate (csrc/se_gate.hip) of the DoubleCone blocks; RAI_SE_GATE=0 keeps the
# torch gate (AdaptiveAvgPool2d, two Linears, GELU, sigmoid) for A/B runs.
_SE_GATE = os.environ.get("RAI_SE_GATE", "1") == "1"


def _se_gate_fusable(C: int) -> bool:
    return C >= 16 and C % 16 == 0 and 256 % (C // 4) == 0 and C // 16 <= 64


class _SETail(torch.autograd.Function):
    """GELU(x + r * s(r)), s = sigmoid(W2 . GELU(W1 . mean_hw r)) (double_cone.py:43-47,85-86), from
    (x, r, W1, W2): rai_se_gate_fwd then rai_se_residual_fwd forward (two launches); rai_se_residual_bwd,
    then rai_se_gate_bwd adding the gate's term into that dr in place, backward (three launches)."""

    @staticmethod
    def forward(ctx, x, r, w1, w2):
        from . import _lib

        B, C, H, W = (int(d) for d in x.shape)
        M = int(w1.shape[0])
        w1, w2 = w1.contiguous(), w2.contiguous()
        s = torch.empty((B, C), dtype=torch.float32, device=x.device)
        pooled = torch.empty_like(s)
        hidden = torch.empty((B, M), dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        L, st = _lib.lib(), _lib.stream_handle(x.device)
        _lib.check(L.rai_se_gate_fwd(r.data_ptr(), w1.data_ptr(), w2.data_ptr(), B, C, H * W, M, s.data_ptr(),
                                     pooled.data_ptr(), hidden.data_ptr(), st), "rai_se_gate_fwd")
        _lib.check(L.rai_se_residual_fwd(x.data_ptr(), r.data_ptr(), s.data_ptr(), B, C, H * W, out.data_ptr(), st),
                   "rai_se_residual_fwd")
        ctx.save_for_backward(x, r, w1, w2, s, pooled, hidden)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import _lib

        x, r, w1, w2, s, pooled, hidden = ctx.saved_tensors
        B, C, H, W = (int(d) for d in x.shape)
        M = int(w1.shape[0])
        dout = dout.contiguous(memory_format=torch.channels_last)
        dx, dr, ds = torch.empty_like(x), torch.empty_like(r), torch.empty_like(s)
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        L, st = _lib.lib(), _lib.stream_handle(x.device)
        _lib.check(L.rai_se_residual_bwd(dout.data_ptr(), x.data_ptr(), r.data_ptr(), s.data_ptr(), B, C, H * W,
                                         dx.data_ptr(), dr.data_ptr(), ds.data_ptr(), st), "rai_se_residual_bwd")
        nb = int(L.rai_se_gate_workspace_bytes(C))
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        _lib.check(L.rai_se_gate_bwd(ds.data_ptr(), s.data_ptr(), pooled.data_ptr(), hidden.data_ptr(), w1.data_ptr(),
                                     w2.data_ptr(), B, C, H * W, M, dr.data_ptr(), dw1.data_ptr(), dw2.data_ptr(),
                                     ws.data_ptr(), nb, st), "rai_se_gate_bwd")
        return dx, dr, dw1, dw2


class ChannelLayerNorm2d(nn.Module):  # shared/module/channel_layer_norm.py
    """gamma * (x - mean_c) / sqrt(var_c + eps) + beta over the channels of each pixel of an NCHW
    tensor; var is torch's default unbiased one (C - 1), unlike nn.LayerNorm's.  This forward is the
    CPU / NCHW / out-of-limits path; run_sequential fuses it with its convolution on the GPU."""

    def __init__(self, num_channels: int, eps: float = 1e-5) -> None:
        super().__init__()
        self.eps = eps
        self.gamma = nn.Parameter(torch.ones(1, num_channels, 1, 1))
        self.beta = nn.Parameter(torch.zeros(1, num_channels, 1, 1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        mean = x.mean(dim=1, keepdim=True)
        var = x.var(dim=1, keepdim=True)
        return self.gamma * (x - mean) / torch.sqrt(var + self.eps) + self.beta


_NORMALIZATIONS = ("batch", "layer", "batch_renorm")  # shared/module/normalization.py:NormalizationMethod


def _norm_method(method_name: str) -> str:
    m = str(method_name).lower()
    if m not in _NORMALIZATIONS:
        raise KeyError(method_name)  # NormalizationMethod[method_name.upper()]
    if m != "layer":
        raise NotImplementedError(f"normalization '{m}' is not built (only 'layer' is): batch / batch_renorm "
                                  "statistics across the captured rollout graph are outside the hot-path scope")
    return m


def normalization2d(method_name: str, num_features: int) -> nn.Module:
    _norm_method(method_name)
    return ChannelLayerNorm2d(num_features)


def normalization1d(method_name: str, num_features: int) -> nn.Module:
    _norm_method(method_name)
    return nn.LayerNorm(num_features)


class _ConvBiasChanLN(torch.autograd.Function):
    """[GELU](ChannelLayerNorm2d(x + b)) over an NHWC bias-free conv output: one HIP pass forward
    (rai_chan_ln_fwd) and the row pass + partial-sum launch backward (rai_chan_ln_bwd)."""

    @staticmethod
    def forward(ctx, x, b, gamma, beta, eps, gelu):
        from . import _lib

        C = int(x.shape[1])
        rows = x.numel() // C
        out = torch.empty_like(x)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().rai_chan_ln_fwd(x.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rows, C,
                                              float(eps), int(gelu), out.data_ptr(), stats.data_ptr(),
                                              _lib.stream_handle(x.device)), "rai_chan_ln_fwd")
        ctx.save_for_backward(x, b, gamma, beta, stats)
        ctx.gelu = int(gelu)
        return out

    @staticmethod
    def backward(ctx, dout):
        from . import _lib

        x, b, gamma, beta, stats = ctx.saved_tensors
        C = int(x.shape[1])
        rows = x.numel() // C
        dout = dout.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(x)
        dpar = torch.empty((3, C), dtype=torch.float32, device=x.device)  # dgamma, dbeta, dbias
        L = _lib.lib()
        nb = int(L.rai_chan_ln_workspace_bytes(C))
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
        _lib.check(L.rai_chan_ln_bwd(dout.data_ptr(), x.data_ptr(), b.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                     stats.data_ptr(), rows, C, ctx.gelu, dx.data_ptr(), dpar[0].data_ptr(),
                                     dpar[1].data_ptr(), dpar[2].data_ptr(), ws.data_ptr(), nb,
                                     _lib.stream_handle(x.device)), "rai_chan_ln_bwd")
        return dx, dpar[2], dpar[0].view(1, C, 1, 1), dpar[1].view(1, C, 1, 1), None, None


def _conv_nobias(conv: nn.Module, x: torch.Tensor) -> torch.Tensor:
    if isinstance(conv, nn.ConvTranspose2d):
        return torch.nn.functional.conv_transpose2d(x, conv.weight, None, conv.stride, conv.padding,
                                                    conv.output_padding, conv.groups, conv.dilation)
    return torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups)


def _chan_ln_fusable(C: int) -> bool:
    from . import _lib

    return 16 <= C <= _lib.RAI_CLN_MAX_C and C % 4 == 0 and (C // 4) & (C // 4 - 1) == 0


def chan_ln_fused(y: torch.Tensor, bias: torch.Tensor, norm: ChannelLayerNorm2d, gelu: bool) -> torch.Tensor:
    """The fused pass over a bias-free NHWC conv output (the one entry to the autograd Function)."""
    return _ConvBiasChanLN.apply(y, bias, norm.gamma, norm.beta, norm.eps, gelu)


def conv_norm(conv: nn.Module, norm: ChannelLayerNorm2d, x: torch.Tensor, gelu: bool) -> torch.Tensor:
    """[GELU](norm(conv(x))) for a Conv2d / ConvTranspose2d with bias and a ChannelLayerNorm2d: on NHWC
    fp32 GPU activations whose C the kernel takes (C / 4 a power of two, 16 <= C <= 256) the convolution
    runs bias-free on MIOpen and bias + norm + GELU is one HIP pass; else the modules' own path."""
    if (_nhwc(x) and conv.bias is not None and _chan_ln_fusable(int(conv.out_channels))
            and norm.gamma.is_cuda and norm.gamma.dtype == torch.float32):
        y = _conv_nobias(conv, x)
        if _nhwc(y):
            return chan_ln_fused(y, conv.bias, norm, gelu)
        y = norm(y + conv.bias.view(1, -1, 1, 1))
    else:
        y = norm(conv(x))
    return torch.nn.functional.gelu(y) if gelu else y


def conv_gelu(conv: nn.Module, x: torch.Tensor) -> torch.Tensor:
    """GELU(conv(x)) for a Conv2d / ConvTranspose2d with bias: on NHWC fp32 GPU activations the
    convolution runs bias-free on MIOpen and bias + GELU is one HIP pass; else the modules' own path."""
    if _nhwc(x) and conv.bias is not None and conv.out_channels % 4 == 0:
        if isinstance(conv, nn.ConvTranspose2d):
            y = torch.nn.functional.conv_transpose2d(x, conv.weight, None, conv.stride, conv.padding,
                                                     conv.output_padding, conv.groups, conv.dilation)
        else:
            y = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation,
                                           conv.groups)
        if _nhwc(y):
            return _BiasGelu.apply(y, conv.bias)
        return torch.nn.functional.gelu(y + conv.bias.view(1, -1, 1, 1))
    return torch.nn.functional.gelu(conv(x))


def _exact_gelu(m: nn.Module) -> bool:
    return isinstance(m, nn.GELU) and m.approximate == "none"


def run_sequential(seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """seq(x) with every (conv, GELU) pair through conv_gelu and every (conv, ChannelLayerNorm2d[,
    GELU]) run through conv_norm (same modules, same state_dict)."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        is_conv = isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))
        if is_conv and i + 1 < len(mods) and _exact_gelu(mods[i + 1]):
            x = conv_gelu(m, x)
            i += 2
        elif is_conv and i + 1 < len(mods) and isinstance(mods[i + 1], ChannelLayerNorm2d):
            gelu = i + 2 < len(mods) and _exact_gelu(mods[i + 2])
            x = conv_norm(m, mods[i + 1], x, gelu)
            i += 3 if gelu else 2
        else:
            x = m(x)
            i += 1
    return x


def se_residual_epilogue(x: torch.Tensor, r: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """GELU(x + r * s[..., None, None]); the fused HIP pass for NHWC fp32 GPU activations whose C
    the kernel tiles (C % 4 == 0, C / 4 divides 256), else the PyTorch composition."""
    C = int(x.shape[1]) if x.dim() == 4 else 0
    if (_nhwc(x) and _nhwc(r) and r.shape == x.shape and C % 4 == 0 and C >= 4 and 256 % (C // 4) == 0
            and s.is_cuda and s.dtype == torch.float32):
        return _SEResidualEpilogue.apply(x, r, s)
    return torch.nn.functional.gelu(x + r * s.view(s.shape[0], s.shape[1], 1, 1))


def _init(layer: nn.Module, orthogonal: bool, std: float = float(np.sqrt(2))) -> nn.Module:
    """shared/module/utils.py:36-45 (bias-free layers: orthogonal weight only)."""
    if orthogonal:
        nn.init.orthogonal_(layer.weight, std)
        if getattr(layer, "bias", None) is not None:
            nn.init.constant_(layer.bias, 0.0)
    return layer


def _as_list(s) -> List[int]:
    return list(s) if isinstance(s, (list, tuple)) else [int(s)]


class SqueezeExcitation(nn.Module):  # double_cone.py:18-47
    def __init__(self, in_channels: int, reduction_ratio: int = 16, init_layers_orthogonal: bool = False) -> None:
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        mid = in_channels // reduction_ratio
        self.fc = nn.Sequential(_init(nn.Linear(in_channels, mid, bias=False), init_layers_orthogonal), nn.GELU(),
                                _init(nn.Linear(mid, in_channels, bias=False), init_layers_orthogonal), nn.Sigmoid())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        b, c = x.shape[0], x.shape[1]
        return x * self.fc(self.avg_pool(x).view(b, c)).view(b, c, 1, 1)


class SEResidualBlock(nn.Module):  # double_cone.py:50-86
    """residual = conv, [norm], GELU, conv, [norm], SqueezeExcitation (the second norm has no GELU)."""

    def __init__(self, channels: int, init_layers_orthogonal: bool = False,
                 normalization: Optional[str] = None) -> None:
        super().__init__()
        conv = lambda: _init(nn.Conv2d(channels, channels, 3, padding=1), init_layers_orthogonal)
        layers: List[nn.Module] = [conv()]
        if normalization:
            layers.append(normalization2d(normalization, channels))
        layers.append(nn.GELU())
        layers.append(conv())
        if normalization:
            layers.append(normalization2d(normalization, channels))
        layers.append(SqueezeExcitation(channels, init_layers_orthogonal=init_layers_orthogonal))
        self.residual = nn.Sequential(*layers)
        self.gelu = nn.GELU()
        self._normalized = bool(normalization)
        # the gate as one HIP launch (_SETail); off here, DoubleConeBackbone turns it on for its blocks
        self.fused_gate = False

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._normalized:
            conv0, norm0, act, conv1, norm1, se = self.residual
            r = conv_norm(conv1, norm1, conv_norm(conv0, norm0, x, True), False)
        else:
            conv0, act, conv1, se = self.residual
            r = conv1(conv_gelu(conv0, x))  # act = GELU
        b, c = r.shape[0], r.shape[1]
        w1, w2 = se.fc[0].weight, se.fc[2].weight
        if (self.fused_gate and _nhwc(x) and _nhwc(r) and r.shape == x.shape and _se_gate_fusable(int(c))
                and w1.is_cuda and w1.dtype == torch.float32):
            return _SETail.apply(x, r, w1, w2)
        s = se.fc(se.avg_pool(r).view(b, c))
        return se_residual_epilogue(x, r, s)  # == self.gelu(x + self.residual(x))


class SqueezeUnetBackbone(nn.Module):  # squeeze_unet.py:20-195
    """Encoder levels (3x3 head conv + SE blocks; then per level strided down-convs + SE blocks),
    decoder levels (transposed-conv up-sampling + SE blocks) with additive skips."""

    def __init__(self, in_channels: int, channels_per_level: List[int], strides_per_level: Strides,
                 encoder_residual_blocks_per_level: List[int], decoder_residual_blocks_per_level: List[int],
                 deconv_strides_per_level: Optional[Strides] = None, init_layers_orthogonal: bool = False,
                 increment_kernel_size_on_down_conv: bool = False, normalization: Optional[str] = None) -> None:
        super().__init__()
        if normalization:
            _norm_method(normalization)  # batch / batch_renorm: NotImplementedError
        orth = init_layers_orthogonal
        ch = list(channels_per_level)
        se = lambda c, n: [SEResidualBlock(c, init_layers_orthogonal=orth, normalization=normalization)
                           for _ in range(n)]
        # [conv, norm?, GELU]: the reference's Sequential indices with and without a normalization
        post = lambda c: ([normalization2d(normalization, c)] if normalization else []) + [nn.GELU()]

        def down(cin: int, cout: int, stride) -> List[nn.Module]:
            mods: List[nn.Module] = []
            for i, s in enumerate(_as_list(stride)):
                k, pad = s, 0
                if increment_kernel_size_on_down_conv and s % 2 == 0:  # squeeze_unet.py:47-55
                    k, pad = s + 1, 1
                mods += [_init(nn.Conv2d(cin if i == 0 else cout, cout, kernel_size=k, stride=s, padding=pad), orth)]
                mods += post(cout)
            return mods

        def up(cin: int, cout: int, stride) -> List[nn.Module]:
            mods: List[nn.Module] = []
            for i, s in enumerate(_as_list(stride)):
                mods += [_init(nn.ConvTranspose2d(cin if i == 0 else cout, cout, kernel_size=s, stride=s), orth)]
                mods += post(cout)
            return mods

        head = [_init(nn.Conv2d(in_channels, ch[0], 3, padding=1), orth)] + post(ch[0])
        self.encoders = nn.ModuleList([nn.Sequential(*(head + se(ch[0], encoder_residual_blocks_per_level[0])))])
        for lvl in range(1, len(ch)):
            self.encoders.append(nn.Sequential(*(down(ch[lvl - 1], ch[lvl], strides_per_level[lvl - 1])
                                                 + se(ch[lvl], encoder_residual_blocks_per_level[lvl]))))
        dstr = list(deconv_strides_per_level or strides_per_level)
        self.decoders = nn.ModuleList([nn.Sequential(*up(ch[-1], ch[-2], dstr[-1]))])
        # middle levels, deepest first: SE blocks at the level's width, then up-sample one level
        # (squeeze_unet.py:151-171 zips the reversed lists, so it stops at the shortest)
        mids = list(zip(reversed(ch[1:-1]), reversed(ch[:-2]), reversed(dstr[:-1]),
                        reversed(decoder_residual_blocks_per_level[:-1])))
        for c, cout, s, n in mids:
            self.decoders.append(nn.Sequential(*(se(c, n) + up(c, cout, s))))
        self.decoders.append(nn.Sequential(*se(ch[0], decoder_residual_blocks_per_level[0])))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        skips = []
        for enc in self.encoders:
            x = run_sequential(enc, x)
            skips.append(x)
        d = None
        for e, dec in zip(reversed(skips), self.decoders):
            d = run_sequential(dec, e if d is None else e + d)  # the reference adds zeros_like at the deepest level
        return d


class _Transpose(nn.Module):  # actor/gridnet_decoder.py:14-20
    def __init__(self, permutation) -> None:
        super().__init__()
        self.permutation = tuple(permutation)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x.permute(self.permutation)


class _HStack(nn.ModuleList):  # shared/module/stack.py
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.hstack([run_sequential(m, x) for m in self])


_OUT_ACT = {"tanh": nn.Tanh, "relu": nn.ReLU, "identity": nn.Identity, "sigmoid": nn.Sigmoid}


def _check_shared_critic(critic_shares_backbone: bool, save_critic_separate: bool, shared_critic_head: bool) -> None:
    if not critic_shares_backbone or save_critic_separate or shared_critic_head:
        raise NotImplementedError("non-shared / shared-head critics are outside the hot-path scope")


class BackboneActorCritic(nn.Module):
    """backbone_actor_critic.py:31-252 (per-position GridNet actions): the actor head and the critic
    heads over a built backbone's (B, backbone_out_channels, H, W) features.  `strides`: the critic
    heads' down-convolutions."""

    def __init__(self, observation_space, action_space, action_plane_space, backbone: nn.Module,
                 backbone_out_channels: int, num_additional_critics: int = 0,
                 additional_critic_activation_functions: Optional[List[str]] = None, critic_channels: int = 64,
                 init_layers_orthogonal: bool = True, cnn_layers_init_orthogonal: bool = False,
                 strides: Strides = (2, 2), output_activation_fn: str = "identity",
                 subaction_mask: Optional[Dict[int, Dict[int, int]]] = None, critic_shares_backbone: bool = True,
                 save_critic_separate: bool = False, shared_critic_head: bool = False,
                 normalization: Optional[str] = None) -> None:
        super().__init__()
        _check_shared_critic(critic_shares_backbone, save_critic_separate, shared_critic_head)
        cnn_orth = bool(cnn_layers_init_orthogonal)
        if num_additional_critics and not additional_critic_activation_functions:
            additional_critic_activation_functions = ["identity"] * num_additional_critics
        # construction order = the reference's (backbone, actor head, critic heads): the seeded
        # default initialisation consumes the RNG identically
        self.backbone = backbone
        self.range_size = float(np.max(observation_space.high) - np.min(observation_space.low))
        self.action_vec = np.asarray(action_plane_space.nvec)
        if isinstance(action_space, dict) or hasattr(action_space, "spaces"):
            raise NotImplementedError("pick_position (Lux) GridNet actions are outside the hot path")
        self.map_size = len(action_space.nvec) // len(self.action_vec)
        self.subaction_mask = subaction_mask
        self._sub = (ValueDependentMask.from_reference_index_to_index_to_value(subaction_mask)
                     if subaction_mask else None)
        self.actor_head = nn.Sequential(
            _init(nn.Conv2d(backbone_out_channels, int(self.action_vec.sum()), kernel_size=3, padding=1),
                  init_layers_orthogonal, std=0.01),
            _Transpose((0, 2, 3, 1)))
        flat_strides: List[int] = []
        for s in strides:
            flat_strides += _as_list(s)

        def critic(act: nn.Module) -> nn.Sequential:  # backbone_actor_critic.py:111-171
            mods: List[nn.Module] = []
            cin = backbone_out_channels
            for s in flat_strides:
                k = max(3, s)
                mods += [_init(nn.Conv2d(cin, critic_channels, k, stride=s, padding=1 if k % 2 else 0), cnn_orth)]
                if normalization:
                    mods.append(normalization2d(normalization, critic_channels))
                mods.append(nn.GELU())
                cin = critic_channels
            mods += [nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                     _init(nn.Linear(critic_channels, critic_channels), init_layers_orthogonal)]
            if normalization:  # (B, critic_channels): torch's LayerNorm
                mods.append(normalization1d(normalization, critic_channels))
            mods += [nn.GELU(), _init(nn.Linear(critic_channels, 1), init_layers_orthogonal, std=1.0), act]
            return nn.Sequential(*mods)

        acts = [_OUT_ACT[n]() for n in [output_activation_fn] + list(additional_critic_activation_functions or [])]
        self._critic_features = len(acts)
        self.critic_heads = _HStack([critic(a) for a in acts])

    # -- backbone_actor_critic.py:189-232 ----------------------------------------------------
    def _preprocess(self, obs: torch.Tensor) -> torch.Tensor:
        if obs.dim() == 3:
            obs = obs.unsqueeze(0)
        x = obs.float() / self.range_size
        if _CHANNELS_LAST and x.is_cuda:  # NHWC activations for MIOpen's implicit-GEMM solvers
            x = x.contiguous(memory_format=torch.channels_last)
        return x

    def _values(self, x: torch.Tensor) -> torch.Tensor:
        v = self.critic_heads(x)
        return v.squeeze(-1) if v.shape[-1] == 1 else v

    def distribution_and_value(self, obs: torch.Tensor, action_masks: torch.Tensor):
        if action_masks is None:
            raise AssertionError(f"No mask case unhandled in {self.__class__.__name__}")
        o = self._preprocess(obs)
        x = self.backbone(o)
        pi = GridnetDistribution(int(np.prod(o.shape[-2:])), self.action_vec, self.actor_head(x), action_masks,
                                 subaction_mask=self._sub)
        return pi, self._values(x)

    def logits_and_value(self, obs: torch.Tensor):
        """(actor-head logits (B, H, W, sum(nvec)), values) — the graph-captured rollout forward."""
        x = self.backbone(self._preprocess(obs))
        return self.actor_head(x), self._values(x)

    def distribution(self, logits: torch.Tensor, action_masks: torch.Tensor) -> GridnetDistribution:
        return GridnetDistribution(int(np.prod(logits.shape[1:3])), self.action_vec, logits, action_masks,
                                   subaction_mask=self._sub)

    def forward(self, obs, action, action_masks=None):
        pi, v = self.distribution_and_value(obs, action_masks)
        logp = pi.log_prob(action)
        return logp, pi.entropy(), v

    def value(self, obs: torch.Tensor) -> torch.Tensor:
        return self._values(self.backbone(self._preprocess(obs)))

    @property
    def action_shape(self):
        return (self.map_size, len(self.action_vec))

    @property
    def value_shape(self):
        return (self._critic_features,) if self._critic_features > 1 else ()


class SqueezeUnetActorCriticNetwork(BackboneActorCritic):
    """squeeze_unet.py:198-270: the squeeze-U-Net backbone under BackboneActorCritic's heads."""

    def __init__(self, observation_space, action_space, action_plane_space, init_layers_orthogonal: bool = True,
                 cnn_layers_init_orthogonal: Optional[bool] = None, channels_per_level: Optional[List[int]] = None,
                 strides_per_level: Optional[Strides] = None, deconv_strides_per_level: Optional[Strides] = None,
                 encoder_residual_blocks_per_level: Optional[List[int]] = None,
                 decoder_residual_blocks_per_level: Optional[List[int]] = None, num_additional_critics: int = 0,
                 additional_critic_activation_functions: Optional[List[str]] = None, critic_channels: int = 64,
                 increment_kernel_size_on_down_conv: bool = False, output_activation_fn: str = "identity",
                 subaction_mask: Optional[Dict[int, Dict[int, int]]] = None, critic_shares_backbone: bool = True,
                 save_critic_separate: bool = False, shared_critic_head: bool = False,
                 normalization: Optional[str] = None) -> None:
        _check_shared_critic(critic_shares_backbone, save_critic_separate, shared_critic_head)
        cnn_orth = bool(cnn_layers_init_orthogonal) if cnn_layers_init_orthogonal is not None else False
        ch = list(channels_per_level or [64, 128, 256])
        strides = list(strides_per_level or [2] * (len(ch) - 1))
        enc_blocks = list(encoder_residual_blocks_per_level or [1] * len(ch))
        dec_blocks = list(decoder_residual_blocks_per_level or enc_blocks[:-1])
        assert len(strides) == len(ch) - 1 and len(enc_blocks) == len(ch) and len(dec_blocks) == len(ch) - 1
        backbone = SqueezeUnetBackbone(int(observation_space.shape[0]), ch, strides, enc_blocks, dec_blocks,
                                       deconv_strides_per_level=deconv_strides_per_level,
                                       init_layers_orthogonal=cnn_orth,
                                       increment_kernel_size_on_down_conv=increment_kernel_size_on_down_conv,
                                       normalization=normalization)
        super().__init__(observation_space, action_space, action_plane_space, backbone, ch[0],
                         num_additional_critics=num_additional_critics,
                         additional_critic_activation_functions=additional_critic_activation_functions,
                         critic_channels=critic_channels, init_layers_orthogonal=init_layers_orthogonal,
                         cnn_layers_init_orthogonal=cnn_orth, strides=strides,
                         output_activation_fn=output_activation_fn, subaction_mask=subaction_mask,
                         normalization=normalization)


class DoubleConeBlock(nn.Module):  # double_cone.py:89-131
    """x + up_conv(res_blocks(gelu(pool_conv(x)))): a 4x4 stride-4 convolution down to the cone's map,
    the cone's SE blocks there, and two 2x2 stride-2 transposed convolutions back up."""

    def __init__(self, channels: int, pooled_channels: int, num_residual_blocks: int = 6,
                 init_layers_orthogonal: bool = False, gelu_pool_conv: bool = True) -> None:
        super().__init__()
        orth = init_layers_orthogonal
        self.pool_conv = _init(nn.Conv2d(channels, pooled_channels, 4, stride=4), orth)
        self.gelu = nn.GELU() if gelu_pool_conv else nn.Identity()
        self.res_blocks = nn.Sequential(*[SEResidualBlock(pooled_channels, init_layers_orthogonal=orth)
                                          for _ in range(num_residual_blocks)])
        mid = (channels + pooled_channels) // 2
        self.up_conv = nn.Sequential(_init(nn.ConvTranspose2d(pooled_channels, mid, 2, stride=2), orth), nn.GELU(),
                                     _init(nn.ConvTranspose2d(mid, channels, 2, stride=2), orth), nn.GELU())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        assert x.shape[-2] % 4 == 0 and x.shape[-1] % 4 == 0, (
            f"DoubleConeBlock needs a map whose height and width are multiples of 4, got {tuple(x.shape[-2:])}")
        # (gelu_pool_conv=False: the plain convolution with its bias)
        p = conv_gelu(self.pool_conv, x) if _exact_gelu(self.gelu) else self.gelu(self.pool_conv(x))
        p = run_sequential(self.res_blocks, p)
        up0, _, up1, _ = self.up_conv
        u = conv_gelu(up0, p)
        if _nhwc(u) and _nhwc(x) and up1.out_channels % 4 == 0:
            y = _conv_nobias(up1, u)
            if _nhwc(y) and y.shape == x.shape:
                return _BiasGeluAdd.apply(y, up1.bias, x)  # x + GELU(y + bias) in one pass
            return x + torch.nn.functional.gelu(y + up1.bias.view(1, -1, 1, 1))
        return x + conv_gelu(up1, u)


class DoubleConeBackbone(nn.Module):  # double_cone.py:134-179
    def __init__(self, in_channels: int, channels: int, pooled_channels: int, init_layers_orthogonal: bool = False,
                 in_num_res_blocks: int = 4, cone_num_res_blocks: int = 6, out_num_res_blocks: int = 4,
                 gelu_pool_conv: bool = True) -> None:
        super().__init__()
        orth = init_layers_orthogonal
        se = lambda n: [SEResidualBlock(channels, init_layers_orthogonal=orth) for _ in range(n)]
        self.in_block = nn.Sequential(_init(nn.Conv2d(in_channels, channels, 3, padding=1), orth), nn.GELU(),
                                      *se(in_num_res_blocks))
        self.double_cone = DoubleConeBlock(channels, pooled_channels, num_residual_blocks=cone_num_res_blocks,
                                           init_layers_orthogonal=orth, gelu_pool_conv=gelu_pool_conv)
        self.out_block = nn.Sequential(*se(out_num_res_blocks))
        set_fused_gate(self, _SE_GATE)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return run_sequential(self.out_block, self.double_cone(run_sequential(self.in_block, x)))


def set_fused_gate(module: nn.Module, on: bool) -> None:
    """Turn the one-launch SE gate (rai_se_gate_fwd / _bwd) on or off for every SE block under `module`."""
    for m in module.modules():
        if isinstance(m, SEResidualBlock):
            m.fused_gate = bool(on)


class DoubleConeActorCritic(BackboneActorCritic):
    """double_cone.py:182-228.  The reference passes no normalization on to this network."""

    def __init__(self, observation_space, action_space, action_plane_space, init_layers_orthogonal: bool = True,
                 cnn_layers_init_orthogonal: Optional[bool] = None, backbone_channels: int = 128,
                 pooled_channels: int = 512, critic_channels: int = 64, in_num_res_blocks: int = 4,
                 cone_num_res_blocks: int = 6, out_num_res_blocks: int = 4, num_additional_critics: int = 0,
                 additional_critic_activation_functions: Optional[List[str]] = None, gelu_pool_conv: bool = True,
                 output_activation_fn: str = "identity",
                 subaction_mask: Optional[Dict[int, Dict[int, int]]] = None) -> None:
        cnn_orth = bool(cnn_layers_init_orthogonal) if cnn_layers_init_orthogonal is not None else False
        backbone = DoubleConeBackbone(int(observation_space.shape[0]), backbone_channels, pooled_channels,
                                      init_layers_orthogonal=cnn_orth, in_num_res_blocks=in_num_res_blocks,
                                      cone_num_res_blocks=cone_num_res_blocks, out_num_res_blocks=out_num_res_blocks,
                                      gelu_pool_conv=gelu_pool_conv)
        super().__init__(observation_space, action_space, action_plane_space, backbone, backbone_channels,
                         num_additional_critics=num_additional_critics,
                         additional_critic_activation_functions=additional_critic_activation_functions,
                         critic_channels=critic_channels, init_layers_orthogonal=init_layers_orthogonal,
                         cnn_layers_init_orthogonal=cnn_orth, output_activation_fn=output_activation_fn,
                         subaction_mask=subaction_mask)
