"""IMPALA CNN encoder (cnn_style: impala) on the GPU: the fused layers of csrc/conv3x3.hip.

The reference encoder (rl_algo_impls/shared/encoder/impala_cnn.py:11-92) is, per ConvSequence, a
Conv2d(3x3, pad 1), a MaxPool2d(3, stride 2, pad 1) and two residual blocks
x + conv(relu(conv(relu(x)))), then one final activation and the flatten.  Here that is three
autograd nodes, all on hand-written f32 MFMA kernels with the elementwise work in their loads and stores:

    ConvPool        conv -> max-pool: rai_conv3x3_fwd(_first), rai_maxpool3x3s2_fwd (argmax bytes kept)
    ResBlock        h = conv1(relu(x)) + b1 (ReLU on load), y = x + conv2(relu(h)) + b2 (skip added in
                    the store); the encoder's last block also applies the final ReLU and writes
                    nn.Flatten's (B, C*H*W) order in that store
    backward        d(h) = dgrad2(dy) * [h > 0], dx = dy + dgrad1(d(h)) * [x > 0]: the masks and the skip
                    are rai_conv3x3_dgrad's epilogue; the weight and bias gradients are rai_conv3x3_wgrad
                    (ReLU on load again), added straight into the flat .grad views inside
                    cnn_ops.direct_grads()

Saved for backward: the block input x, the mid activation h, the pool's argmax bytes and the final
output -- never a stored relu(x).  Tensors are (B, C, H, W) in channels_last memory (NHWC), as on the
NatureCNN path.  `fusable()` is the shape gate, evaluated before any kernel is launched: outside it
(CPU, a non-ReLU activation, RAI_CONV_MFMA=0, channel counts the kernels do not take) the encoder runs
its modules through F.conv2d / F.max_pool2d.
"""
from __future__ import annotations

import torch

from . import _lib, cnn_ops
from .cnn_ops import _BRT_MAX_ELEMS, _WG_WS, _WS, _direct
from .dp_buckets import notify_grad_written

_CL = torch.channels_last


def _chan_ok(c: int) -> bool:
    return 16 <= c <= 128 and c % 16 == 0


def _conv_ok(conv, first: bool) -> bool:
    if not (isinstance(conv, torch.nn.Conv2d) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1)
            and conv.padding == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros" and conv.bias is not None):
        return False
    if not (_chan_ok(conv.out_channels) and (conv.in_channels in (3, 4) if first else _chan_ok(conv.in_channels))):
        return False
    return all(p.dtype == torch.float32 and p.data_ptr() % 16 == 0 for p in (conv.weight, conv.bias))


def convs(encoder) -> list:
    """The encoder's convolutions in module order: five per ConvSequence."""
    out = []
    for seq in list(encoder.cnn)[:-1]:
        s = seq.seq
        out += [s[0], s[2].residual[1], s[2].residual[3], s[3].residual[1], s[3].residual[3]]
    return out


def fusable(encoder, x: torch.Tensor) -> bool:
    """The fused path applies to this encoder and input: a GPU tensor (fp32, or the uint8 frames),
    ReLU activations and shapes csrc/conv3x3.hip takes.  Evaluated before any launch."""
    if not (cnn_ops._CONV_MFMA and encoder._relu and x.is_cuda and x.dim() == 4
            and x.dtype in (torch.float32, torch.uint8)):
        return False
    if x.requires_grad:  # the first layer has no input gradient kernel (Ci 3 / 4): the module path differentiates
        return False
    cs = convs(encoder)
    if int(x.shape[1]) != cs[0].in_channels:
        return False
    return all(_conv_ok(c, i == 0) for i, c in enumerate(cs))


def _weight(w: torch.Tensor) -> torch.Tensor:
    """The weight as (Co, 3, 3, Ci) memory: as stored inside the trainer (optim.FlatParams keeps the
    convolution weights channels_last), a copy for a module outside it."""
    return w if w.is_contiguous(memory_format=_CL) else w.contiguous(memory_format=_CL)


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous(memory_format=_CL)
    if t.data_ptr() % 16:
        t = t.clone(memory_format=_CL)
    return t


def _empty(B, C, H, W, device, dtype=torch.float32) -> torch.Tensor:
    return torch.empty((B, C, H, W), dtype=dtype, device=device, memory_format=_CL)


def _conv_fwd(x, w, b, res=None, pre=False, post=False, flatten=False, x_div=None) -> torch.Tensor:
    B, Ci, H, W = (int(v) for v in x.shape)
    Co = int(w.shape[0])
    L, st = _lib.lib(), _lib.stream_handle(x.device)
    if Ci in (3, 4):
        y = _empty(B, Co, H, W, x.device)
        u8 = x.dtype == torch.uint8
        _lib.check(L.rai_conv3x3_fwd_first(x.data_ptr(), 1 if u8 else 0, float(x_div) if u8 else 1.0, w.data_ptr(),
                                           b.data_ptr(), B, H, W, Ci, Co, y.data_ptr(), st), "rai_conv3x3_fwd_first")
        return y
    y = (torch.empty((B, Co * H * W), dtype=torch.float32, device=x.device) if flatten
         else _empty(B, Co, H, W, x.device))
    _lib.check(L.rai_conv3x3_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), None if res is None else res.data_ptr(),
                                 B, H, W, Ci, Co, int(pre), int(post), int(flatten), y.data_ptr(), st),
               "rai_conv3x3_fwd")
    return y


def _conv_dgrad(dz, w, m=None, res=None) -> torch.Tensor:
    B, Co, H, W = (int(v) for v in dz.shape)
    Ci = int(w.shape[1])
    dx = _empty(B, Ci, H, W, dz.device)
    _lib.check(_lib.lib().rai_conv3x3_dgrad(dz.data_ptr(), w.data_ptr(), None if m is None else m.data_ptr(),
                                            None if res is None else res.data_ptr(), B, H, W, Ci, Co, dx.data_ptr(),
                                            _lib.stream_handle(dz.device)), "rai_conv3x3_dgrad")
    return dx


def _conv_wgrad(key, x, dz, w, b, pre: bool, direct: bool, x_div=None):
    """The layer's weight and bias gradients: added into the flat .grad views (direct; returns
    (None, None)) or returned as fresh tensors."""
    B, Ci, H, W = (int(v) for v in x.shape)
    Co = int(dz.shape[1])
    L, st = _lib.lib(), _lib.stream_handle(x.device)
    nb = int(L.rai_conv3x3_wgrad_workspace_bytes(B, H, W, Ci, Co))
    ws = _WG_WS.get(key, nb, x.device)
    if direct:
        dw, db = w.grad, b.grad
    else:
        dw = torch.empty((Co, Ci, 3, 3), dtype=torch.float32, device=x.device, memory_format=_CL)
        db = torch.empty(Co, dtype=torch.float32, device=x.device)
    acc = 1 if direct else 0
    if Ci in (3, 4):
        u8 = x.dtype == torch.uint8
        _lib.check(L.rai_conv3x3_wgrad_first(x.data_ptr(), 1 if u8 else 0, float(x_div) if u8 else 1.0, dz.data_ptr(),
                                             B, H, W, Ci, Co, dw.data_ptr(), db.data_ptr(), acc, ws.data_ptr(), nb,
                                             st), "rai_conv3x3_wgrad_first")
    else:
        _lib.check(L.rai_conv3x3_wgrad(x.data_ptr(), dz.data_ptr(), B, H, W, Ci, Co, int(pre), dw.data_ptr(),
                                       db.data_ptr(), acc, ws.data_ptr(), nb, st), "rai_conv3x3_wgrad")
    if direct:
        notify_grad_written(w)
        notify_grad_written(b)
        return None, None
    return dw, db


def _direct_pair(w: torch.Tensor, b: torch.Tensor) -> bool:
    """Both gradients are flat-buffer views a kernel may add into through their data pointers."""
    return (_direct(w) and _direct(b, raw=True) and w.grad.is_contiguous(memory_format=_CL)
            and w.is_contiguous(memory_format=_CL) and w.grad.data_ptr() % 16 == 0 and b.grad.data_ptr() % 16 == 0)


def _pool_fwd(z: torch.Tensor):
    B, C, H, W = (int(v) for v in z.shape)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = _empty(B, C, OH, OW, z.device)
    am = _empty(B, C, OH, OW, z.device, torch.uint8)
    _lib.check(_lib.lib().rai_maxpool3x3s2_fwd(z.data_ptr(), B, H, W, C, y.data_ptr(), am.data_ptr(),
                                               _lib.stream_handle(z.device)), "rai_maxpool3x3s2_fwd")
    return y, am


def _pool_bwd(dy: torch.Tensor, am: torch.Tensor, H: int, W: int) -> torch.Tensor:
    B, C = int(dy.shape[0]), int(dy.shape[1])
    dx = _empty(B, C, H, W, dy.device)
    _lib.check(_lib.lib().rai_maxpool3x3s2_bwd(dy.data_ptr(), am.data_ptr(), B, H, W, C, dx.data_ptr(),
                                               _lib.stream_handle(dy.device)), "rai_maxpool3x3s2_bwd")
    return dx


class ConvPool(torch.autograd.Function):
    """max_pool2d(conv2d(x, W, b, padding=1), 3, stride=2, padding=1): a ConvSequence's first two
    modules.  x: NHWC fp32, or for the first sequence the uint8 frames (read as x / x_div)."""

    @staticmethod
    def forward(ctx, x, w, b, key, x_div):
        wc = _weight(w)
        z = _conv_fwd(x, wc, b, x_div=x_div)
        y, am = _pool_fwd(z)
        ctx.save_for_backward(x, w, b, am)
        ctx.conf = (key, x_div, _direct_pair(w, b), tuple(int(v) for v in z.shape[2:]))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, am = ctx.saved_tensors
        key, x_div, direct, (H, W) = ctx.conf
        wc = _weight(w)
        dz = _pool_bwd(_nhwc(dy), am, H, W)
        dx = _conv_dgrad(dz, wc) if ctx.needs_input_grad[0] else None
        dw = db = None  # (a frozen layer under a trainable input: no weight-gradient launch)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, db = _conv_wgrad(key, x, dz, w, b, False, direct, x_div)
        return dx, dw, db, None, None


class ResBlock(torch.autograd.Function):
    """x + conv2(relu(conv1(relu(x)))) (impala_cnn.py:11-31); final: relu of it, flattened in NCHW
    order (the encoder's last activation and nn.Flatten)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, key1, key2, final):
        h = _conv_fwd(x, _weight(w1), b1, pre=True)
        y = _conv_fwd(h, _weight(w2), b2, res=x, pre=True, post=final, flatten=final)
        saved = (x, h, w1, b1, w2, b2) + ((y,) if final else ())
        ctx.save_for_backward(*saved)
        ctx.conf = (key1, key2, final, _direct_pair(w1, b1), _direct_pair(w2, b2))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h, w1, b1, w2, b2 = ctx.saved_tensors[:6]
        key1, key2, final, direct1, direct2 = ctx.conf
        B, C, H, W = (int(v) for v in x.shape)
        if final:
            y = ctx.saved_tensors[6]
            if _final_bwd_fused(C, H * W):
                dout = _empty(B, C, H, W, x.device)
                scratch = torch.empty(C, dtype=torch.float32, device=x.device)  # (the wgrad below gives db)
                ws = _WS.get(key2, C, x.device)
                dy = dy.contiguous()
                _lib.check(_lib.lib().rai_bias_relu_bwd_nchw(dy.data_ptr(), y.data_ptr(), B, H * W, C,
                                                             dout.data_ptr(), scratch.data_ptr(), 0, ws.data_ptr(),
                                                             ws.numel(), _lib.stream_handle(x.device)),
                           "rai_bias_relu_bwd_nchw")
            else:  # beyond the transposing kernel's (C + 1) * HW limit: torch ops for this one step
                dout = _nhwc(torch.ops.aten.threshold_backward(dy.reshape(B, C, H, W), y.view(B, C, H, W), 0))
        else:
            dout = _nhwc(dy)
        need = ctx.needs_input_grad  # a frozen layer's weight-gradient launch is skipped
        need1 = need[1] or need[2]
        dh = _conv_dgrad(dout, _weight(w2), m=h) if need[0] or need1 else None
        dw1 = db1 = dw2 = db2 = None
        if need[3] or need[4]:
            dw2, db2 = _conv_wgrad(key2, h, dout, w2, b2, True, direct2)
        dx = _conv_dgrad(dh, _weight(w1), m=x, res=dout) if need[0] else None
        if need1:
            dw1, db1 = _conv_wgrad(key1, x, dh, w1, b1, True, direct1)
        return dx, dw1, db1, dw2, db2, None, None, None


def _final_bwd_fused(C: int, HW: int) -> bool:
    """rai_bias_relu_bwd_nchw's documented limits (include/rai_amd.h)."""
    return C % 4 == 0 and 256 % (C // 4) == 0 and (C + 1) * HW <= _BRT_MAX_ELEMS


def conv_pool(conv: torch.nn.Conv2d, x: torch.Tensor, x_div=None) -> torch.Tensor:
    return ConvPool.apply(x, conv.weight, conv.bias, conv, x_div)


def res_block(block, x: torch.Tensor, final: bool = False) -> torch.Tensor:
    c1, c2 = block.residual[1], block.residual[3]
    if final and _final_bwd_fused(int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])):
        _WS.prewarm(c2, int(x.shape[1]), x.device)
    return ResBlock.apply(x, c1.weight, c1.bias, c2.weight, c2.bias, c1, c2, final)
