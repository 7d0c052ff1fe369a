"""The device operations of a CNN training step: ctypes wrappers over include/qgx_conv_train.h, include/qgx_head_train.h,
include/qgx_flux_train.h, include/qgx_latent_train.h and include/qgx_dconv_train.h and the torch.autograd.Functions that put them
behind autograd.

The convolutions — more than 95 % of a step's FLOPs — are the kernels of csrc/conv_train.hip behind ``circular_conv2d``.  The
two ends of a step — the gather of a batch from the resident set into the engine layout, and the loss head (MSE, or softplus
then MSE) with its gradient — are the kernels of csrc/train_head.hip behind ``gather_batch``, ``head_loss`` and ``head_apply``.
A flux-form net (div=True) ends in ``flux_divergence``: the generators' spectral divergence and its adjoint, csrc/fluxdiv_train.hip.
A conditional VAE has ``latent_sample`` between its encoder and its decoder: the reparameterised sample, the KL divergence and
the variance diagnostics in one call each way, csrc/latent_train.hip; ``latent_prior`` is the same forward without an encoder.
A GAN's discriminator is made of ``strided_conv2d``, csrc/dconv_train.hip: three Functions whose backwards are each other, so that
the gradient penalty's second derivative runs on the same three kernels.
The DeepInversion U-Net generator is made of ``unet_conv2d``, csrc/uconv_train.hip (include/qgx_uconv_train.h): the circular 3 x 3
and 1 x 1 convolution on any grid down to 2 x 2 with up to 512 -> 1024 channels, differentiable once.
Every tensor is checked here, once per layout (``_engine``, ``_planar``, ``_rows``), before a pointer reaches the library.
The nets and loops that use these operations are in tools/train_CNN.py, tools/train_CVAE.py and tools/train_CGAN.py.
"""
import contextlib
import ctypes as C

import torch

from .. import _lib
from .._lib import lib, check

GRIDS = (16, 32, 48, 64, 96, 128)          # what include/qgx_conv_train.h admits


def c8(c):
    """channels per pixel of the engine's layout: rounded up to 8"""
    return (int(c) + 7) // 8 * 8


_WORK = {}


def workspace(kind, size_call, shape, device):
    """the workspace of one kind ('conv', 'dconv', 'uconv': one size for the three calls; 'head': the loss partials; 'latent': the partial
    sums of the KL divergence and the variances) and shape, of
    size_call(*shape, &bytes) bytes, cached per device, stream and shape: calls on one stream run in order, so they may share
    it; calls on different streams may not"""
    key = (kind, device.index, torch.cuda.current_stream(device).cuda_stream) + shape
    ws = _WORK.get(key)
    if ws is None:
        n = C.c_size_t()
        check(size_call(*shape, C.byref(n)))
        ws = _WORK[key] = torch.empty(n.value, dtype=torch.uint8, device=device)
    return ws


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _engine(t, name, channels=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == t.shape[2] and t.shape[3] % 8 == 0):
        raise ValueError(f'{name}: a float32 device tensor (B, N, N, C8) in the engine layout, not {tuple(t.shape)} {t.dtype} on {t.device}')
    if channels is not None and t.shape[3] != c8(channels):
        raise ValueError(f'{name}: {t.shape[3]} channels per pixel, {channels} channels take {c8(channels)}')
    return t.contiguous()


def _planar(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[2] == t.shape[3]
            and 1 <= t.shape[1] <= 8 and t.shape[0] >= 1):
        raise ValueError(f'{name}: a float32 device tensor (n, C, N, N) with 1 ... 8 channels, not '
                         f'{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}'
                         f'{(" %s on %s" % (t.dtype, t.device)) if torch.is_tensor(t) else ""}')
    return _aligned(t.contiguous())


def _rows(idx, like):
    """idx -> None or a contiguous, aligned int64 vector on `like`'s device (the indices' range is the caller's duty: train()
    checks an epoch's order on the host before it uploads it)"""
    if idx is None:
        return None
    if not (torch.is_tensor(idx) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.device == like.device and len(idx) >= 1):
        raise ValueError(f'idx: an int64 vector on {like.device}, or None')
    return _aligned(idx.contiguous())


def _weight(w):
    if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.shape[2] == w.shape[3]):
        raise ValueError(f'weight: a float32 device tensor (cout, cin, k, k), not {tuple(w.shape)} {w.dtype} on {w.device}')
    return w.contiguous(), int(w.shape[0]), int(w.shape[1]), int(w.shape[2])


def _ptr(t):
    return None if t is None else t.data_ptr()


def conv2d_forward(x, w, b=None):
    """y (B, N, N, c8(cout)) = conv_circular(x (B, N, N, c8(cin)), w (cout, cin, k, k)) + b"""
    w, cout, cin, k = _weight(w)
    x = _engine(x, 'x', cin)
    B, N = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        ws = workspace('conv', lib.qgx_conv2d_workspace, (B, N, cin, cout, k), x.device)
        y = torch.empty((B, N, N, c8(cout)), dtype=torch.float32, device=x.device)
        check(lib.qgx_conv2d_forward(x.data_ptr(), w.data_ptr(), _ptr(None if b is None else b.contiguous()), y.data_ptr(),
                                     B, N, cin, cout, k, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    return y


def conv2d_backward_data(dy, w):
    """dx (B, N, N, c8(cin)) of dy (B, N, N, c8(cout))"""
    w, cout, cin, k = _weight(w)
    dy = _engine(dy, 'dy', cout)
    B, N = int(dy.shape[0]), int(dy.shape[1])
    with torch.cuda.device(dy.device):
        ws = workspace('conv', lib.qgx_conv2d_workspace, (B, N, cin, cout, k), dy.device)
        dx = torch.empty((B, N, N, c8(cin)), dtype=torch.float32, device=dy.device)
        check(lib.qgx_conv2d_backward_data(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, N, cin, cout, k, ws.data_ptr(),
                                           ws.numel(), _lib.current_stream_ptr()))
    return dx


def conv2d_backward_weight(x, dy, cin, cout, k, bias=True):
    """dw (cout, cin, k, k) and db (cout) (None without `bias`)"""
    x, dy = _engine(x, 'x', cin), _engine(dy, 'dy', cout)
    B, N = int(x.shape[0]), int(x.shape[1])
    if dy.shape[:3] != x.shape[:3]:
        raise ValueError(f'x {tuple(x.shape)} and dy {tuple(dy.shape)} differ in batch or grid')
    with torch.cuda.device(x.device):
        ws = workspace('conv', lib.qgx_conv2d_workspace, (B, N, cin, cout, k), x.device)
        dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
        db = torch.empty((cout,), dtype=torch.float32, device=x.device) if bias else None
        check(lib.qgx_conv2d_backward_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), B, N, cin, cout, k,
                                             ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    return dw, db


LAUNCHES = {'forward': 0, 'backward_data': 0, 'backward_weight': 0}      # counted per call of the Function (tests, timing)


class _CircularConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        LAUNCHES['forward'] += 1
        return conv2d_forward(x, w, b)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            LAUNCHES['backward_data'] += 1
            dx = conv2d_backward_data(dy, w)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            LAUNCHES['backward_weight'] += 1
            dw, db = conv2d_backward_weight(x, dy, int(w.shape[1]), int(w.shape[0]), int(w.shape[2]), bias=ctx.has_bias)
        return dx, dw, db


def circular_conv2d(x, w, b=None):
    """Conv2d(padding='same', padding_mode='circular') on the engine layout, differentiable: x (B, N, N, c8(cin)) float32 on
    the device with zero pad channels, w (cout, cin, k, k), b (cout) or None -> (B, N, N, c8(cout)).  The data gradient is
    computed only if x requires it (a net's first layer does not)."""
    return _CircularConv2d.apply(x, w, b)


UCONV_LAUNCHES = {'forward': 0, 'backward_data': 0, 'backward_weight': 0}  # counted per call of the Function (tests, timing)


def _uconv_call(call, ptrs, B, N, cin, cout, k, device):
    """one call of include/qgx_uconv_train.h with the workspace of the shape"""
    with torch.cuda.device(device):
        ws = workspace('uconv', lib.qgx_uconv2d_workspace, (B, N, cin, cout, k), device)
        check(call(*ptrs, B, N, cin, cout, k, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))


def uconv2d_forward(x, w, b=None):
    """y (B, N, N, c8(cout)) = conv_circular(x (B, N, N, c8(cin)), w (cout, cin, k, k)) + b: k 1 or 3, any grid 2 ... 128"""
    w, cout, cin, k = _weight(w)
    x, w = _aligned(_engine(x, 'x', cin)), _aligned(w)
    if b is not None:
        if not (b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (cout,)):
            raise ValueError(f'bias: a float32 device tensor ({cout},), not {tuple(b.shape)} {b.dtype} on {b.device}')
        b = _aligned(b.contiguous())
    B, N = int(x.shape[0]), int(x.shape[1])
    y = torch.empty((B, N, N, c8(cout)), dtype=torch.float32, device=x.device)
    _uconv_call(lib.qgx_uconv2d_forward, (x.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr()), B, N, cin, cout, k, x.device)
    return y


def uconv2d_backward_data(dy, w):
    """dx (B, N, N, c8(cin)) of dy (B, N, N, c8(cout))"""
    w, cout, cin, k = _weight(w)
    dy, w = _aligned(_engine(dy, 'dy', cout)), _aligned(w)
    B, N = int(dy.shape[0]), int(dy.shape[1])
    dx = torch.empty((B, N, N, c8(cin)), dtype=torch.float32, device=dy.device)
    _uconv_call(lib.qgx_uconv2d_backward_data, (dy.data_ptr(), w.data_ptr(), dx.data_ptr()), B, N, cin, cout, k, dy.device)
    return dx


def uconv2d_backward_weight(x, dy, cin, cout, k, bias=True):
    """dw (cout, cin, k, k) and db (cout) (None without `bias`)"""
    x, dy = _aligned(_engine(x, 'x', cin)), _aligned(_engine(dy, 'dy', cout))
    B, N = int(x.shape[0]), int(x.shape[1])
    if dy.shape[:3] != x.shape[:3] or dy.device != x.device:
        raise ValueError(f'x {tuple(x.shape)} and dy {tuple(dy.shape)} differ in batch, grid or device')
    dw = torch.empty((int(cout), int(cin), int(k), int(k)), dtype=torch.float32, device=x.device)
    db = torch.empty((int(cout),), dtype=torch.float32, device=x.device) if bias else None
    _uconv_call(lib.qgx_uconv2d_backward_weight, (x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db)), B, N, int(cin), int(cout),
                int(k), x.device)
    return dw, db


class _UnetConv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        UCONV_LAUNCHES['forward'] += 1
        return uconv2d_forward(x, w, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            UCONV_LAUNCHES['backward_data'] += 1
            dx = uconv2d_backward_data(dy, w)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            UCONV_LAUNCHES['backward_weight'] += 1
            dw, db = uconv2d_backward_weight(x, dy, int(w.shape[1]), int(w.shape[0]), int(w.shape[2]), bias=ctx.has_bias)
        return dx, dw, db


def unet_conv2d(x, w, b=None):
    """Conv2d(cin, cout, k, padding=k // 2, padding_mode='circular'), k 1 or 3, on the engine layout, differentiable ONCE (a
    generator needs no second derivative; asking for one raises): x (B, N, N, c8(cin)) float32 on the device with zero pad
    channels, any grid 2 ... 128, w (cout, cin, k, k) with cin <= 512 and cout <= 1024, b (cout) or None -> (B, N, N, c8(cout)).
    The layer of the DeepInversion U-Net generator, csrc/uconv_train.hip.  A gradient is computed only where it is asked for:
    the net's first layer gets no data gradient."""
    return _UnetConv2d.apply(x, w, b)


def _dconv_weight(w):
    w, cout, cin, k = _weight(w)
    if k != 4:
        raise ValueError(f'weight: (cout, cin, 4, 4), not {tuple(w.shape)}')
    return _aligned(w), cout, cin


def _dconv_call(call, a, b, out, B, N, cin, cout):
    """one call of include/qgx_dconv_train.h: two inputs, one output, the workspace of the shape"""
    with torch.cuda.device(out.device):
        ws = workspace('dconv', lib.qgx_dconv2d_workspace, (B, N, cin, cout), out.device)
        check(call(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, N, cin, cout, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    return out


def dconv2d_forward(x, w):
    """y (B, N/2, N/2, c8(cout)) = conv(x (B, N, N, c8(cin)), w (cout, cin, 4, 4); stride 2, zero padding 1)"""
    w, cout, cin = _dconv_weight(w)
    x = _aligned(_engine(x, 'x', cin))
    B, N = int(x.shape[0]), int(x.shape[1])
    y = torch.empty((B, N // 2, N // 2, c8(cout)), dtype=torch.float32, device=x.device)
    return _dconv_call(lib.qgx_dconv2d_forward, x, w, y, B, N, cin, cout)


def dconv2d_backward_data(dy, w):
    """dx (B, N, N, c8(cin)) of dy (B, N/2, N/2, c8(cout))"""
    w, cout, cin = _dconv_weight(w)
    dy = _aligned(_engine(dy, 'dy', cout))
    B, N = int(dy.shape[0]), 2 * int(dy.shape[1])
    dx = torch.empty((B, N, N, c8(cin)), dtype=torch.float32, device=dy.device)
    return _dconv_call(lib.qgx_dconv2d_backward_data, dy, w, dx, B, N, cin, cout)


def dconv2d_backward_weight(x, dy, cin, cout):
    """dw (cout, cin, 4, 4) of x (B, N, N, c8(cin)) and dy (B, N/2, N/2, c8(cout))"""
    x, dy = _aligned(_engine(x, 'x', cin)), _aligned(_engine(dy, 'dy', cout))
    B, N = int(x.shape[0]), int(x.shape[1])
    if dy.shape[0] != B or 2 * dy.shape[1] != N or dy.device != x.device:
        raise ValueError(f'x {tuple(x.shape)} and dy {tuple(dy.shape)} differ in batch, grid or device: dy has half of x\'s grid')
    dw = torch.empty((int(cout), int(cin), 4, 4), dtype=torch.float32, device=x.device)
    return _dconv_call(lib.qgx_dconv2d_backward_weight, x, dy, dw, B, N, int(cin), int(cout))


DCONV_LAUNCHES = {'forward': 0, 'backward_data': 0, 'backward_weight': 0}  # counted per call of a Function (tests, timing)
_DATA_ONLY = [False]      # a module-level flag, not a thread-local one: autograd runs a backward on a thread of its own


@contextlib.contextmanager
def data_gradient_only():
    """Inside the block the backward of strided_conv2d's forward computes the data gradient alone.  A Function's
    needs_input_grad says which inputs require a gradient, not which of them the caller of autograd.grad asked for; a
    gradient penalty asks for the input's alone, and a generator step uses the discriminator's alone, so both would pay a
    weight gradient per layer for nothing.  The weights then receive None, which autograd reads as zero."""
    old, _DATA_ONLY[0] = _DATA_ONLY[0], True
    try:
        yield
    finally:
        _DATA_ONLY[0] = old


# The convolution is bilinear in (x, w), so the derivative of each of the three operations with respect to either operand is
# another of the three.  Each Function's backward calls the other two through their .apply: under create_graph=True the graph
# of a backward exists, and the layer is differentiable as often as one likes.
class _DconvForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        DCONV_LAUNCHES['forward'] += 1
        return dconv2d_forward(x, w)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = _DconvBackwardData.apply(dy, w) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1] and not _DATA_ONLY[0]:
            dw = _DconvBackwardWeight.apply(x, dy, int(w.shape[1]), int(w.shape[0]))
        return dx, dw


class _DconvBackwardData(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, w):
        ctx.save_for_backward(dy, w)
        DCONV_LAUNCHES['backward_data'] += 1
        return dconv2d_backward_data(dy, w)

    @staticmethod
    def backward(ctx, g):                    # <g, dx(dy, w)> = <forward(g, w), dy> = <backward_weight(g, dy), w>
        dy, w = ctx.saved_tensors
        g = g.contiguous()
        d_dy = _DconvForward.apply(g, w) if ctx.needs_input_grad[0] else None
        d_w = _DconvBackwardWeight.apply(g, dy, int(w.shape[1]), int(w.shape[0])) if ctx.needs_input_grad[1] else None
        return d_dy, d_w


class _DconvBackwardWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dy, cin, cout):
        ctx.save_for_backward(x, dy)
        DCONV_LAUNCHES['backward_weight'] += 1
        return dconv2d_backward_weight(x, dy, cin, cout)

    @staticmethod
    def backward(ctx, g):                    # <g, dw(x, dy)> = <backward_data(dy, g), x> = <forward(x, g), dy>
        x, dy = ctx.saved_tensors
        g = g.contiguous()
        d_x = _DconvBackwardData.apply(dy, g) if ctx.needs_input_grad[0] else None
        d_dy = _DconvForward.apply(x, g) if ctx.needs_input_grad[1] else None
        return d_x, d_dy, None, None


def strided_conv2d(x, w):
    """Conv2d(cin, cout, 4, stride=2, padding=1, bias=False) — zero padding — on the engine layout, differentiable TWICE (and
    more): x (B, N, N, c8(cin)) float32 on the device, w (cout, cin, 4, 4) -> (B, N/2, N/2, c8(cout)).  The layer of
    CGANRegression's discriminator, whose gradient penalty differentiates a gradient.  A gradient is computed only where it
    is asked for."""
    return _DconvForward.apply(x, w)


def to_engine_layout(x):
    """planar (B, C, N, N) -> (B, N, N, c8(C)) with zero pad channels"""
    B, Cn, N = int(x.shape[0]), int(x.shape[1]), int(x.shape[-1])
    out = torch.zeros((B, N, N, c8(Cn)), dtype=torch.float32, device=x.device)
    out[..., :Cn] = x.permute(0, 2, 3, 1)
    return out


FLUX_LAUNCHES = {'forward': 0, 'backward': 0}                             # counted per call of the Function (tests, timing)


def _flux_call(call, t, name, channels):
    """one call of include/qgx_flux_train.h in the engine layout: (B, N, N, 8) -> (B, N, N, 8), no workspace"""
    t = _aligned(_engine(t, name, channels))
    B, N = int(t.shape[0]), int(t.shape[1])
    with torch.cuda.device(t.device):
        out = torch.empty((B, N, N, 8), dtype=torch.float32, device=t.device)
        check(call(t.data_ptr(), out.data_ptr(), B, N, _lib.FLUX_ENGINE, _lib.current_stream_ptr()))
    return out


class _FluxDivergence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, F):
        FLUX_LAUNCHES['forward'] += 1
        return _flux_call(lib.qgx_fluxdiv_forward, F, 'F', 4)

    @staticmethod
    def backward(ctx, dy):
        FLUX_LAUNCHES['backward'] += 1
        return _flux_call(lib.qgx_fluxdiv_backward, dy, 'dy', 2)


def flux_divergence(F):
    """10000 * divergence(F) of a flux-form net (AndrewCNN(div=True)) on the engine layout, differentiable: F (B, N, N, 8) with
    channels [fx1, fx2, fy1, fy2, 0, 0, 0, 0] -> (B, N, N, 8) with channels [y1, y2, 0, ...].  The forward is the kernel body
    the generators run at inference, the backward its adjoint (csrc/fluxdiv_core.hpp); the operator is linear, so nothing is
    saved.  One HIP call each way."""
    return _FluxDivergence.apply(F)


HEADS = {'mse': _lib.HEAD_MSE, 'softplus_mse': _lib.HEAD_SOFTPLUS_MSE}     # the modes of include/qgx_head_train.h
HEAD_LAUNCHES = {'gather': 0, 'loss': 0, 'grad': 0, 'apply': 0}           # counted per call of a wrapper (tests, timing)


def head_mode(head):
    if head not in HEADS:
        raise ValueError(f'head={head!r}: one of {sorted(HEADS)}')
    return HEADS[head]


def _head_args(head, y, T, idx):
    """(mode, y, T, idx, B, N, C, n) of a head call: y (B, N, N, 8) in the engine layout against rows idx of the planar set T"""
    mode, T = head_mode(head), _planar(T, 'T')
    y = _aligned(_engine(y, 'y', int(T.shape[1])))
    idx = _rows(idx, y)
    B, N = int(y.shape[0]), int(y.shape[1])
    if T.device != y.device or int(T.shape[-1]) != N or (len(T) < B if idx is None else len(idx) != B):
        raise ValueError(f'y {tuple(y.shape)}, T {tuple(T.shape)}, idx {None if idx is None else tuple(idx.shape)} do not fit')
    return mode, y, T, idx, B, N, int(T.shape[1]), len(T)


def gather_batch(X, idx=None):
    """X[idx] (all of X without idx) of the planar device set X (n, C, N, N), in the engine layout (B, N, N, 8) with zero pad
    channels: one launch for the index gather, the zero fill and the permuted copy of to_engine_layout"""
    X = _planar(X, 'X')
    idx = _rows(idx, X)
    n, Cn, N = int(X.shape[0]), int(X.shape[1]), int(X.shape[-1])
    B = n if idx is None else len(idx)
    with torch.cuda.device(X.device):
        out = torch.empty((B, N, N, 8), dtype=torch.float32, device=X.device)
        check(lib.qgx_batch_gather(X.data_ptr(), _ptr(idx), out.data_ptr(), n, B, N, Cn, _lib.current_stream_ptr()))
    HEAD_LAUNCHES['gather'] += 1
    return out


def head_loss_value(y, T, idx, head):
    """mean over b, c, y, x of (h(y[b]) - T[idx[b]])^2 as a 0-dim float64 device tensor (no autograd: see head_loss)"""
    mode, y, T, idx, B, N, Cn, n = _head_args(head, y, T, idx)
    with torch.cuda.device(y.device):
        ws = workspace('head', lib.qgx_head_workspace, (B, N), y.device)
        loss = torch.empty((), dtype=torch.float64, device=y.device)
        check(lib.qgx_head_loss(y.data_ptr(), T.data_ptr(), _ptr(idx), mode, loss.data_ptr(), B, N, Cn, n, ws.data_ptr(),
                                ws.numel(), _lib.current_stream_ptr()))
    HEAD_LAUNCHES['loss'] += 1
    return loss


def head_loss_grad(y, T, idx, head, gout):
    """dy (B, N, N, 8) of head_loss_value times the 0-dim float64 device tensor gout, which is read on the device"""
    mode, y, T, idx, B, N, Cn, n = _head_args(head, y, T, idx)
    if not (torch.is_tensor(gout) and gout.numel() == 1 and gout.device == y.device):
        raise ValueError('gout: one number on the device of y')
    gout = _aligned(gout.detach().to(torch.float64).contiguous())
    with torch.cuda.device(y.device):
        dy = torch.empty_like(y)
        check(lib.qgx_head_grad(y.data_ptr(), T.data_ptr(), _ptr(idx), mode, gout.data_ptr(), dy.data_ptr(), B, N, Cn, n,
                                _lib.current_stream_ptr()))
    HEAD_LAUNCHES['grad'] += 1
    return dy


class _HeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, T, idx, head):
        ctx.save_for_backward(y, T, idx)
        ctx.head = head
        return head_loss_value(y, T, idx, head)

    @staticmethod
    def backward(ctx, gout):
        y, T, idx = ctx.saved_tensors
        return head_loss_grad(y, T, idx, ctx.head, gout), None, None, None


def head_loss(y_engine, T, idx, mode):
    """The loss of a net's last activation y_engine (B, N, N, 8) against rows idx (None: 0 ... B - 1) of the planar device set
    T (n, C, N, N): mse_loss(h(y), T[idx]) with h the identity (mode 'mse') or softplus ('softplus_mse'), a 0-dim float64
    device tensor, differentiable in y_engine.  Forward and backward are one HIP call each; the backward recomputes from
    y_engine and T, nothing but those two is kept."""
    return _HeadLoss.apply(y_engine, T, idx, mode)


def head_apply(y_engine, channels, mode, T=None, idx=None, out=None):
    """planar (B, channels, N, N): h(y_engine) without T, else the squared residuals (T[idx] - h(y_engine))^2; written into
    `out` if given (a contiguous float32 device tensor of that shape).  Not differentiable."""
    Cn, n = int(channels), 0
    if not 1 <= Cn <= 8:
        raise ValueError(f'channels = {channels}: 1 ... 8')
    if T is None:
        m, y = head_mode(mode), _aligned(_engine(y_engine.detach(), 'y', Cn))
        B, N = int(y.shape[0]), int(y.shape[1])
    else:
        m, y, T, idx, B, N, Ct, n = _head_args(mode, y_engine.detach(), T, idx)
        if Ct != Cn:
            raise ValueError(f'T has {Ct} channels, not {channels}')
    with torch.cuda.device(y.device):
        if out is None:
            out = torch.empty((B, Cn, N, N), dtype=torch.float32, device=y.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, Cn, N, N) and out.is_contiguous()
                  and out.data_ptr() % 16 == 0):
            raise ValueError(f'out: a contiguous float32 device tensor {(B, Cn, N, N)}')
        check(lib.qgx_head_apply(y.data_ptr(), _ptr(T), None if T is None else _ptr(idx), m, out.data_ptr(), B, N, Cn, n,
                                 _lib.current_stream_ptr()))
    HEAD_LAUNCHES['apply'] += 1
    return out


LATENT_LAUNCHES = {'forward': 0, 'backward': 0, 'prior': 0}               # counted per call of a wrapper (tests, timing)
_U64 = (1 << 64) - 1


def _latent_args(enc, X, idx, eps, seed, step):
    """(enc, X, idx, eps, B, N, n, seed, step) of a call of include/qgx_latent_train.h: enc (B, N, N, 8) in the engine layout
    or None, rows idx of the planar PV set X (n, 2, N, N), eps planar (B, 2, N, N) or None"""
    X = _planar(X, 'X')
    idx = _rows(idx, X)
    N, n = int(X.shape[-1]), len(X)
    B = n if idx is None else len(idx)
    if enc is not None:
        enc = _aligned(_engine(enc, 'enc', 4))
        B = int(enc.shape[0]) if idx is None else B
    if int(X.shape[1]) != 2 or (enc is not None and (enc.device != X.device or tuple(enc.shape) != (B, N, N, 8))) or n < B:
        raise ValueError(f'enc {None if enc is None else tuple(enc.shape)}, X {tuple(X.shape)}, idx '
                         f'{None if idx is None else tuple(idx.shape)} do not fit: X has 2 channels, enc is (B, N, N, 8)')
    if eps is not None:
        eps = _planar(eps, 'eps')
        if eps.device != X.device or tuple(eps.shape) != (B, 2, N, N):
            raise ValueError(f'eps {tuple(eps.shape)}: expected {(B, 2, N, N)} on {X.device}')
    seed, step = int(seed), int(step)
    if not (0 <= seed <= _U64 and 0 <= step <= _U64):
        raise ValueError(f'seed = {seed}, step = {step}: unsigned 64-bit numbers')
    return enc, X, idx, eps, B, N, n, seed, step


def latent_forward(enc, X, idx, seed, step, eps=None):
    """qgx_latent_forward -> (dec_in (B, N, N, 8), stats (3) float64 on the device: loss_KL, var_latent, var_aggr; None
    without enc).  No autograd: see latent_sample"""
    enc, X, idx, eps, B, N, n, seed, step = _latent_args(enc, X, idx, eps, seed, step)
    with torch.cuda.device(X.device):
        dec_in = torch.empty((B, N, N, 8), dtype=torch.float32, device=X.device)
        stats = ws = None
        if enc is not None:
            ws = workspace('latent', lib.qgx_latent_workspace, (B, N), X.device)
            stats = torch.empty((3,), dtype=torch.float64, device=X.device)
        check(lib.qgx_latent_forward(_ptr(enc), X.data_ptr(), _ptr(idx), _ptr(eps), seed, step, dec_in.data_ptr(), _ptr(stats), B, N, n,
                                     _ptr(ws), 0 if ws is None else ws.numel(), _lib.current_stream_ptr()))
    LATENT_LAUNCHES['prior' if enc is None else 'forward'] += 1
    return dec_in, stats


def latent_backward(enc, eps, seed, step, d_dec_in, gout_kl):
    """qgx_latent_backward -> d_enc (B, N, N, 8); gout_kl is one number on the device, read there"""
    enc = _aligned(_engine(enc, 'enc', 4))
    B, N = int(enc.shape[0]), int(enc.shape[1])
    d_dec_in = _aligned(_engine(d_dec_in, 'd_dec_in', 4))
    if d_dec_in.shape != enc.shape or d_dec_in.device != enc.device:
        raise ValueError(f'd_dec_in {tuple(d_dec_in.shape)} and enc {tuple(enc.shape)} differ')
    if eps is not None:
        eps = _planar(eps, 'eps')
        if eps.device != enc.device or tuple(eps.shape) != (B, 2, N, N):
            raise ValueError(f'eps {tuple(eps.shape)}: expected {(B, 2, N, N)} on {enc.device}')
    if not (torch.is_tensor(gout_kl) and gout_kl.numel() == 1 and gout_kl.device == enc.device):
        raise ValueError('gout_kl: one number on the device of enc')
    gout_kl = _aligned(gout_kl.detach().to(torch.float64).contiguous())
    with torch.cuda.device(enc.device):
        d_enc = torch.empty_like(enc)
        check(lib.qgx_latent_backward(enc.data_ptr(), _ptr(eps), int(seed), int(step), d_dec_in.data_ptr(), gout_kl.data_ptr(),
                                      d_enc.data_ptr(), B, N, _lib.current_stream_ptr()))
    LATENT_LAUNCHES['backward'] += 1
    return d_enc


class _LatentSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc, X, idx, seed, step, eps):
        dec_in, stats = latent_forward(enc, X, idx, seed, step, eps)
        ctx.save_for_backward(enc, eps)
        ctx.draw = (int(seed), int(step))
        loss_KL, var_latent, var_aggr = stats[0], stats[1], stats[2]
        ctx.mark_non_differentiable(var_latent, var_aggr)
        return dec_in, loss_KL, var_latent, var_aggr

    @staticmethod
    def backward(ctx, d_dec_in, g_kl, _g_latent, _g_aggr):
        enc, eps = ctx.saved_tensors          # an output that took no part in the loss comes with a zero gradient
        return latent_backward(enc, eps, *ctx.draw, d_dec_in.contiguous(), g_kl), None, None, None, None, None


def latent_sample(enc, X, idx, seed, step, eps=None):
    """The latent step of a conditional VAE between its encoder and its decoder, differentiable in enc.  enc (B, N, N, 8) is the
    encoder's last activation in the engine layout, channels [mu1, mu2, logvar1, logvar2]; X the planar PV set (n, 2, N, N) on
    the device and idx its B rows (None: rows 0 ... B - 1).  Returns (dec_in, loss_KL, var_latent, var_aggr): dec_in (B, N, N, 8)
    with channels [x1, x2, z1, z2], z = eps exp(logvar / 2) + mu, and three 0-dim float64 device tensors, the KL divergence to
    the standard normal summed over pixels and channels and averaged over the batch, the mean of exp(logvar), and the latter plus
    the unbiased variance of mu (the two are diagnostics: no gradient).  eps planar (B, 2, N, N), or None: the standard
    normals of the Philox stream (seed, member b, step), drawn in the forward and AGAIN in the backward: nothing but enc is
    kept (a given eps is).  One HIP call forward (two launches: the kernel and the finish of its sums), one backward."""
    return _LatentSample.apply(enc, X, idx, seed, step, eps)


def latent_prior(X, idx, seed, step):
    """dec_in (B, N, N, 8) = [x1, x2, z1, z2] with z drawn from the prior: the standard normals of the Philox stream (seed,
    member b, step); what a decoder predicts from.  Not differentiable."""
    return latent_forward(None, X, idx, seed, step)[0]
