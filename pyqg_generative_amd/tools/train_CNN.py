"""Training of OLSModel on the device (reference: models/ols_model.py:35-57 fit / save_model, tools/cnn_tools.py:125-182
AndrewCNN, :402-421 prepare_PV_data, :607-700 minibatch / evaluate_test / train).

The convolutions — more than 95 % of a step's FLOPs — are the HIP kernels of csrc/conv_train.hip behind
``circular_conv2d``, a torch.autograd.Function over the three entry points of include/qgx_conv_train.h.  BatchNorm's batch
statistics, ReLU, the MSE, Adam and the learning-rate schedule are torch ops on device tensors, and autograd does their
backward.  ``fit_ols`` writes the reference's model folder (net.pt, x_scale.json, y_scale.json, model_args.json, stats.nc)
and returns ``OLSModel(folder=...)`` read back from those files.

Training of MeanVarModel (reference: models/mean_var_model.py:14-17 VarCNN, :41-80 fit / save_model): ``fit_meanvar`` trains
net_mean, evaluates it over both sets and trains net_var on the squared residuals.  Its nets are ``FusedHeadCNN``s: the two
ends of a step — the gather of a batch from the resident set into the engine layout, and the loss head (MSE, or softplus
then MSE) with its gradient — are the kernels of csrc/train_head.hip behind ``gather_batch``, ``head_loss`` (a
torch.autograd.Function) and ``head_apply`` (include/qgx_head_train.h).

Command line:
    python -m pyqg_generative_amd.tools.train_CNN [--model OLSModel|MeanVarModel] --train 'GLOB' --validate 'GLOB' \\
        [--test 'GLOB'] --model_args "{'hidden_channels': [128, 64, 32, 32, 32, 32, 32]}" --fit_args "{'num_epochs': 50}"
"""
import ctypes as C
import json
import math
import os
from time import time

import numpy as np
import torch
from torch import nn

from .. import _lib, weights as _weights
from .._lib import lib, check
from .cnn_tools import ChannelwiseScaler
from .train_ANN import learning_rates

GRIDS = (16, 32, 48, 64, 96, 128)          # what include/qgx_conv_train.h admits


def c8(c):
    """channels per pixel of the engine's layout: rounded up to 8"""
    return (int(c) + 7) // 8 * 8


_WORK = {}


def conv_workspace(device, B, N, cin, cout, k):
    """the workspace of one shape (one size for the three calls), cached per device, stream and shape: calls on one stream
    run in order, so they may share it; calls on different streams may not"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, int(B), int(N), int(cin), int(cout), int(k))
    ws = _WORK.get(key)
    if ws is None:
        n = C.c_size_t()
        check(lib.qgx_conv2d_workspace(B, N, cin, cout, k, C.byref(n)))
        ws = _WORK[key] = torch.empty(n.value, dtype=torch.uint8, device=device)
    return ws


def _activation(t, name, channels=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == t.shape[2] and t.shape[3] % 8 == 0):
        raise ValueError(f'{name}: a float32 device tensor (B, N, N, C8) in the engine layout, not {tuple(t.shape)} {t.dtype} on {t.device}')
    if channels is not None and t.shape[3] != c8(channels):
        raise ValueError(f'{name}: {t.shape[3]} channels per pixel, {channels} channels take {c8(channels)}')
    return t.contiguous()


def _weight(w):
    if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.shape[2] == w.shape[3]):
        raise ValueError(f'weight: a float32 device tensor (cout, cin, k, k), not {tuple(w.shape)} {w.dtype} on {w.device}')
    return w.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def conv2d_forward(x, w, b=None):
    """y (B, N, N, c8(cout)) = conv_circular(x (B, N, N, c8(cin)), w (cout, cin, k, k)) + b"""
    w = _weight(w)
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    x = _activation(x, 'x', cin)
    B, N = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        ws = conv_workspace(x.device, B, N, cin, cout, k)
        y = torch.empty((B, N, N, c8(cout)), dtype=torch.float32, device=x.device)
        check(lib.qgx_conv2d_forward(x.data_ptr(), w.data_ptr(), _ptr(None if b is None else b.contiguous()), y.data_ptr(),
                                     B, N, cin, cout, k, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()))
    return y


def conv2d_backward_data(dy, w):
    """dx (B, N, N, c8(cin)) of dy (B, N, N, c8(cout))"""
    w = _weight(w)
    cout, cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    dy = _activation(dy, 'dy', cout)
    B, N = int(dy.shape[0]), int(dy.shape[1])
    with torch.cuda.device(dy.device):
        ws = conv_workspace(dy.device, B, N, cin, cout, k)
        dx = torch.empty((B, N, N, c8(cin)), dtype=torch.float32, device=dy.device)
        check(lib.qgx_conv2d_backward_data(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), B, N, cin, cout, k, ws.data_ptr(),
                                           ws.numel(), _lib.current_stream_ptr()))
    return dx


def conv2d_backward_weight(x, dy, cin, cout, k, bias=True):
    """dw (cout, cin, k, k) and db (cout) (None without `bias`)"""
    x, dy = _activation(x, 'x', cin), _activation(dy, 'dy', cout)
    B, N = int(x.shape[0]), int(x.shape[1])
    if dy.shape[:3] != x.shape[:3]:
        raise ValueError(f'x {tuple(x.shape)} and dy {tuple(dy.shape)} differ in batch or grid')
    with torch.cuda.device(x.device):
        ws = conv_workspace(x.device, B, N, cin, cout, k)
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


def to_engine_layout(x):
    """planar (B, C, N, N) -> (B, N, N, c8(C)) with zero pad channels"""
    B, Cn, N = int(x.shape[0]), int(x.shape[1]), int(x.shape[-1])
    out = torch.zeros((B, N, N, c8(Cn)), dtype=torch.float32, device=x.device)
    out[..., :Cn] = x.permute(0, 2, 3, 1)
    return out


HEADS = {'mse': _lib.HEAD_MSE, 'softplus_mse': _lib.HEAD_SOFTPLUS_MSE}     # the modes of include/qgx_head_train.h
HEAD_LAUNCHES = {'gather': 0, 'loss': 0, 'grad': 0, 'apply': 0}           # counted per call of a wrapper (tests, timing)


def head_workspace(device, B, N):
    """the loss partials of one (B, N), cached per device and stream like conv_workspace"""
    key = ('head', device.index, torch.cuda.current_stream(device).cuda_stream, int(B), int(N))
    ws = _WORK.get(key)
    if ws is None:
        n = C.c_size_t()
        check(lib.qgx_head_workspace(B, N, C.byref(n)))
        ws = _WORK[key] = torch.empty(n.value, dtype=torch.uint8, device=device)
    return ws


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()


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


def _head_record(y, name='y'):
    y = _activation(y, name)
    if y.shape[3] != 8:
        raise ValueError(f'{name}: {y.shape[3]} channels per pixel; the heads take nets of 1 ... 8 output channels (8 per pixel)')
    return _aligned(y)


def _mode(head):
    if head not in HEADS:
        raise ValueError(f'head={head!r}: one of {sorted(HEADS)}')
    return HEADS[head]


def _targets(y, T, idx):
    """(T, idx, B, N, C, n) of a head call on y (B, N, N, 8)"""
    T, idx = _planar(T, 'T'), _rows(idx, y)
    B, N = int(y.shape[0]), int(y.shape[1])
    if T.device != y.device or int(T.shape[-1]) != N or (len(T) < B if idx is None else len(idx) != B):
        raise ValueError(f'y {tuple(y.shape)}, T {tuple(T.shape)}, idx {None if idx is None else tuple(idx.shape)} do not fit')
    return T, idx, B, N, int(T.shape[1]), len(T)


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
    mode, y = _mode(head), _head_record(y)
    T, idx, B, N, Cn, n = _targets(y, T, idx)
    with torch.cuda.device(y.device):
        ws = head_workspace(y.device, B, N)
        loss = torch.empty((), dtype=torch.float64, device=y.device)
        check(lib.qgx_head_loss(y.data_ptr(), T.data_ptr(), _ptr(idx), mode, loss.data_ptr(), B, N, Cn, n, ws.data_ptr(),
                                ws.numel(), _lib.current_stream_ptr()))
    HEAD_LAUNCHES['loss'] += 1
    return loss


def head_loss_grad(y, T, idx, head, gout):
    """dy (B, N, N, 8) of head_loss_value times the 0-dim float64 device tensor gout, which is read on the device"""
    mode, y = _mode(head), _head_record(y)
    T, idx, B, N, Cn, n = _targets(y, T, idx)
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
    m, y = _mode(mode), _head_record(y_engine.detach())
    B, N, Cn, n = int(y.shape[0]), int(y.shape[1]), int(channels), 0
    if T is not None:
        T, idx, B, N, Cn, n = _targets(y, T, idx)
        if Cn != int(channels):
            raise ValueError(f'T has {Cn} channels, not {channels}')
    if not 1 <= Cn <= 8:
        raise ValueError(f'channels = {channels}: 1 ... 8')
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


def _pad(v, n):
    return v if v.shape[0] == n else torch.nn.functional.pad(v, (0, n - v.shape[0]))


class TrainableAndrewCNN(nn.Module):
    """AndrewCNN(n_in, n_out, batch_norm=, bias=, hidden_channels=) (cnn_tools.py:125-182) with the reference's state dict —
    `conv` is the same nn.Sequential of Conv2d / ReLU / BatchNorm2d modules, which hold the parameters and buffers and give
    torch's default initialisation, drawn on the CPU under `seed` — and a forward on the device kernels: activations stay
    in the engine layout (B, N, N, C8) between layers, ReLU and BatchNorm are torch expressions on them with the
    per-channel vectors padded by zeros to C8, so the pad channels stay zero."""

    def __init__(self, n_in, n_out, hidden_channels=(128, 64, 32, 32, 32, 32, 32), batch_norm=True, bias=True, div=False,
                 final_activation='None', seed=0):
        super().__init__()
        if div:
            raise NotImplementedError('div=True: the backward of the divergence has no device path yet')
        if final_activation != 'None':
            raise NotImplementedError(f'final_activation={final_activation!r} has no device path')
        hidden = _weights.check_hidden_channels(hidden_channels)
        self.n_in, self.n_out, self.hidden_channels = int(n_in), int(n_out), hidden
        self.batch_norm, self.bias = bool(batch_norm), bool(bias)
        ch = [self.n_in] + hidden + [self.n_out]
        ks = _weights.arch_kernels(hidden)
        blocks = []
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            for l in range(len(ch) - 1):
                blocks.append(nn.Conv2d(ch[l], ch[l + 1], ks[l], padding='same', padding_mode='circular', bias=self.bias))
                if l < len(ch) - 2:
                    blocks.append(nn.ReLU())
                    if self.batch_norm:
                        blocks.append(nn.BatchNorm2d(ch[l + 1]))
        self.conv = nn.Sequential(*blocks)
        self.log_dict = {}

    def _bn(self, bn, a):
        C8 = a.shape[-1]
        if self.training:
            mean = a.mean(dim=(0, 1, 2))
            var = a.var(dim=(0, 1, 2), unbiased=False)
            with torch.no_grad():
                Cn, n = bn.num_features, a.numel() // C8
                m = bn.momentum
                bn.running_mean.mul_(1 - m).add_(mean[:Cn], alpha=m)
                bn.running_var.mul_(1 - m).add_(var[:Cn] * (n / (n - 1)), alpha=m)
                bn.num_batches_tracked += 1
        else:
            mean, var = _pad(bn.running_mean, C8), _pad(bn.running_var, C8)
        return (a - mean) / torch.sqrt(var + bn.eps) * _pad(bn.weight, C8) + _pad(bn.bias, C8)

    def forward_engine(self, a):
        """(B, N, N, c8(n_in)) -> (B, N, N, c8(n_out))"""
        for mod in self.conv:
            if isinstance(mod, nn.Conv2d):
                a = circular_conv2d(a, mod.weight, mod.bias)
            elif isinstance(mod, nn.ReLU):
                a = torch.relu(a)
            else:
                a = self._bn(mod, a)
        return a

    def forward(self, x):
        """x planar (B, n_in, N, N) on the device -> planar (B, n_out, N, N)"""
        if x.dim() != 4 or x.shape[1] != self.n_in or x.shape[-1] != x.shape[-2] or int(x.shape[-1]) not in GRIDS:
            raise ValueError(f'input {tuple(x.shape)}: expected (B, {self.n_in}, N, N) with N one of {GRIDS}')
        y = self.forward_engine(to_engine_layout(x.to(torch.float32)))
        return y[..., :self.n_out].permute(0, 3, 1, 2)

    def compute_loss(self, x, ytrue):
        return {'loss': nn.functional.mse_loss(self.forward(x), ytrue)}


class FusedHeadCNN(TrainableAndrewCNN):
    """TrainableAndrewCNN whose two ends are the kernels of include/qgx_head_train.h.  head='mse' is AndrewCNN itself (net_mean
    of MeanVarModel); head='softplus_mse' is the reference's VarCNN (mean_var_model.py:14-17: the forward ends in softplus),
    which adds no parameter: state dict and seeded initialisation are the parent's.

      forward(x)                 planar h(conv(x)) through qgx_batch_gather and qgx_head_apply: the inference surface, NOT
                                 differentiable (it runs under no_grad)
      compute_loss(x, y)         mse_loss(h(conv(x)), y) as torch expressions at both ends (to_engine_layout, slice and permute,
                                 softplus, mse_loss): differentiable, the form the reference states
      indexed_loss(X, T, idx)    the same value for x = X[idx], y = T[idx] of device-resident sets: gather_batch ->
                                 forward_engine -> head_loss; differentiable; what train() runs"""

    def __init__(self, n_in, n_out, hidden_channels=(128, 64, 32, 32, 32, 32, 32), head='mse', seed=0):
        _mode(head)
        if not (1 <= int(n_in) <= 8 and 1 <= int(n_out) <= 8):
            raise ValueError(f'n_in = {n_in}, n_out = {n_out}: the fused ends take 1 ... 8 channels')
        super().__init__(n_in, n_out, hidden_channels=hidden_channels, seed=seed)
        self.head = head

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.n_in or x.shape[-1] != x.shape[-2] or int(x.shape[-1]) not in GRIDS:
            raise ValueError(f'input {tuple(x.shape)}: expected (B, {self.n_in}, N, N) with N one of {GRIDS}')
        with torch.no_grad():
            return head_apply(self.forward_engine(gather_batch(x.to(torch.float32))), self.n_out, self.head)

    def compute_loss(self, x, ytrue):
        y = TrainableAndrewCNN.forward(self, x)
        if self.head == 'softplus_mse':
            y = nn.functional.softplus(y)
        return {'loss': nn.functional.mse_loss(y, ytrue)}

    def indexed_loss(self, X, T, idx=None):
        return {'loss': head_loss(self.forward_engine(gather_batch(X, idx)), T, idx, self.head)}


def evaluate_test(net, X, Y, batch_size=64, acc=None):
    """evaluate_test (cnn_tools.py:624-643): eval mode, no gradients; sum over the batches of loss * n into acc[0], n into acc[1]"""
    net.eval()
    with torch.no_grad():
        for s in range(0, len(X), batch_size):
            x, y = X[s:s + batch_size], Y[s:s + batch_size]
            loss = net.indexed_loss(x, y) if hasattr(net, 'indexed_loss') else net.compute_loss(x, y)
            acc[0] += loss['loss'].to(torch.float64) * len(x)
            acc[1] += len(x)
    net.train()


def train(net, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, device=0, orders=None, verbose=True):
    """train (cnn_tools.py:645-700) with the data resident on the device: Adam, MultiStepLR with milestones int(E / 2),
    int(3 E / 4), int(7 E / 8) stepped per epoch, a shuffle of the samples per epoch (numpy's global stream, as minibatch
    does; orders(epoch, n) replaces it), evaluate_test in eval mode, net.log_dict with 'loss' and 'loss_test' per epoch.
    The losses are accumulated on the device and read back once per epoch.  A net that offers indexed_loss(X, T, idx)
    (FusedHeadCNN) is given the resident sets and the batch's indices instead of the gathered batch, in training and in
    evaluate_test; its epoch orders are checked on the host, since the gather kernel does not check them."""
    dev = torch.device('cuda', int(device)) if not isinstance(device, torch.device) else device
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if not torch.is_tensor(a) else a.to(dev, torch.float32)
    X_train, Y_train, X_test, Y_test = (as_dev(a) for a in (X_train, Y_train, X_test, Y_test))
    n = len(X_train)
    if verbose:
        print(f'Training starts on device {torch.cuda.get_device_name(dev)}, number of samples {n}')
    net.to(dev)
    net.train()
    optimizer = torch.optim.Adam(net.parameters(), lr=learning_rate)
    E = int(num_epochs)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    if not hasattr(net, 'log_dict'):
        net.log_dict = {}
    log = net.log_dict
    log.setdefault('loss', [])
    log.setdefault('loss_test', [])
    indexed = hasattr(net, 'indexed_loss')       # a net with fused ends (FusedHeadCNN): batches are gathered by the kernels
    t_s = time()
    with torch.cuda.device(dev):
        for epoch in range(E):
            t_e = time()
            acc = torch.zeros((2, 2), dtype=torch.float64, device=dev)
            order = np.arange(n)
            if orders is None:
                np.random.shuffle(order)
            else:
                order = np.asarray(orders(epoch, n), dtype=np.int64)
            if indexed and not (order.shape == (n,) and order.min() >= 0 and order.max() < n):
                raise ValueError(f'orders({epoch}, {n}): not {n} indices in 0 ... {n - 1}')      # the kernels do not check them
            order = torch.as_tensor(order).to(dev)
            for s in range(0, n, batch_size):
                idx = order[s:s + batch_size]
                optimizer.zero_grad()
                if indexed:
                    loss = net.indexed_loss(X_train, Y_train, idx)['loss']
                else:
                    x, y = X_train[idx], Y_train[idx]
                    loss = net.compute_loss(x, y)['loss']
                loss.backward()
                optimizer.step()
                acc[0, 0] += loss.detach().to(torch.float64) * len(idx)
                acc[0, 1] += len(idx)
            scheduler.step()
            evaluate_test(net, X_test, Y_test, batch_size=batch_size, acc=acc[1])
            a = acc.cpu().numpy()                        # the epoch's one host read
            log['loss'].append(float(a[0, 0] / a[0, 1]))
            log['loss_test'].append(float(a[1, 0] / a[1, 1]))
            if verbose:
                t = time()
                print('[%d/%d] [%.2f/%.2f] Loss: [%.3f, %.3f]' % (epoch + 1, E, t - t_e, (t - t_s) * (E / (epoch + 1) - 1),
                                                                  log['loss'][-1], log['loss_test'][-1]))
    return net


def extract(ds, key):
    """extract (cnn_tools.py:398-400): ds[key] (run, time, lev, y, x) -> (run * time, lev, y, x)"""
    if key not in ds:
        raise ValueError(f'fit_ols needs {key!r} in every dataset')
    a = ds[key]
    dims = tuple(a.dims)
    if dims != ('run', 'time', 'lev', 'y', 'x'):
        if set(dims) != {'run', 'time', 'lev', 'y', 'x'}:
            raise ValueError(f'{key}: dims {dims}, expected (run, time, lev, y, x)')
        a = a.transpose('run', 'time', 'lev', 'y', 'x')
    v = np.asarray(a.values)
    if v.shape[-1] != v.shape[-2] or v.shape[-1] not in GRIDS:
        raise ValueError(f'{key}: a {v.shape[-2]} x {v.shape[-1]} grid; the device trains on square grids of {GRIDS}')
    if v.shape[2] != 2:
        raise ValueError(f'{key}: {v.shape[2]} levels, expected 2')
    return v.reshape((-1,) + v.shape[2:])


def channel_scaler(X):
    """ChannelwiseScaler(X) (cnn_tools.py:458-515): per-channel mean and population std in float64, cast to float32"""
    X = np.asarray(X, dtype=np.float64)
    return ChannelwiseScaler(std=X.std(axis=(0, 2, 3)).astype('float32'), mean=X.mean(axis=(0, 2, 3)).astype('float32'))


def prepare_PV_data(ds_train, ds_test):
    """prepare_PV_data (cnn_tools.py:402-421): q and q_forcing_advection divided by the training set's channelwise std"""
    X_train, Y_train = extract(ds_train, 'q'), extract(ds_train, 'q_forcing_advection')
    X_test, Y_test = extract(ds_test, 'q'), extract(ds_test, 'q_forcing_advection')
    x_scale, y_scale = channel_scaler(X_train), channel_scaler(Y_train)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return (f32(x_scale.normalize(X_train)), f32(y_scale.normalize(Y_train)), f32(x_scale.normalize(X_test)),
            f32(y_scale.normalize(Y_test)), x_scale, y_scale)


def write_model_folder(folder, state_dict, x_scale, y_scale, model_args, log):
    """OLSModel.save_model (ols_model.py:48-57): net.pt (CPU state dict), x_scale.json, y_scale.json, model_args.json with
    model: 'OLSModel' and the constructor arguments, stats.nc (log_to_xarray: one variable per key over `epoch`)"""
    os.makedirs(folder, exist_ok=True)
    torch.save({k: v.detach().cpu().clone() for k, v in state_dict.items()}, os.path.join(folder, 'net.pt'))
    x_scale.write('x_scale.json', folder=folder)
    y_scale.write('y_scale.json', folder=folder)
    with open(os.path.join(folder, 'model_args.json'), 'w') as f:
        json.dump(dict(model='OLSModel', **model_args), f)
    _write_log(os.path.join(folder, 'stats.nc'), log)


def _write_log(path, log):
    """log_to_xarray(log).to_netcdf(path): one variable per key over `epoch`; a file already there is replaced"""
    from .simulate import dataset_backend
    xr = dataset_backend()
    E = len(next(iter(log.values())))
    stats = xr.Dataset({k: (['epoch'], np.asarray(v, dtype=np.float64)) for k, v in log.items()},
                       coords={'epoch': np.arange(1, E + 1)})
    if os.path.exists(path):
        os.remove(path)
    stats.to_netcdf(path)


def write_meanvar_folder(folder, mean_state, var_state, x_scale, y_scale, hidden_channels, log_mean, log_var):
    """MeanVarModel.save_model (mean_var_model.py:68-80): net_mean.pt, net_var.pt (CPU state dicts), x_scale.json,
    y_scale.json, model_args.json with model: 'MeanVarModel' and hidden_channels, stats_mean.nc — not written without a log:
    a net_mean read from the folder has none — and stats_var.nc"""
    os.makedirs(folder, exist_ok=True)
    for name, state in (('net_mean.pt', mean_state), ('net_var.pt', var_state)):
        torch.save({k: v.detach().cpu().clone() for k, v in state.items()}, os.path.join(folder, name))
    x_scale.write('x_scale.json', folder=folder)
    y_scale.write('y_scale.json', folder=folder)
    with open(os.path.join(folder, 'model_args.json'), 'w') as f:
        json.dump(dict(model='MeanVarModel', hidden_channels=[int(c) for c in hidden_channels]), f)
    if log_mean and log_mean.get('loss'):
        _write_log(os.path.join(folder, 'stats_mean.nc'), log_mean)
    _write_log(os.path.join(folder, 'stats_var.nc'), log_var)


def _check_fit_args(who, num_epochs, batch_size, learning_rate):
    if batch_size < 1:
        raise ValueError(f'{who}: batch_size = {batch_size}')
    if num_epochs < 1:
        raise ValueError(f'{who}: num_epochs = {num_epochs}')
    if not (math.isfinite(learning_rate) and learning_rate >= 0):
        raise ValueError(f'{who}: learning_rate = {learning_rate}')


def squared_residuals(net, X, Y, batch_size=64):
    """(Y - net(X))^2 of the eval-mode net over the device-resident sets, in batches, as a device tensor shaped like Y
    (mean_var_model.py:55-59): the last activation goes from the engine layout straight into the residuals"""
    out = torch.empty_like(Y)
    net.eval()
    with torch.no_grad():
        for s in range(0, len(X), batch_size):
            y = net.forward_engine(gather_batch(X[s:s + batch_size]))
            head_apply(y, net.n_out, net.head, T=Y[s:s + batch_size], out=out[s:s + batch_size])
    net.train()
    return out


def fit_meanvar(ds_train, ds_test, *, hidden_channels=[128, 64, 32, 32, 32, 32, 32], folder='model', num_epochs=50, batch_size=64,
                learning_rate=0.001, seed=0, device=0, orders=None, verbose=True):
    """MeanVarModel(folder, hidden_channels).fit(ds_train, ds_test, num_epochs, batch_size, learning_rate) on the device
    (mean_var_model.py:41-80), then save_model; returns MeanVarModel(folder=folder) read back from the files, with the two
    trained nets attached as trained_net_mean and trained_net_var.

    net_mean is trained with MSE on q_forcing_advection, evaluated in eval mode over both sets, and net_var (the forward ends
    in softplus) is trained with MSE on the squared residuals.  net_mean is initialised with torch's defaults under `seed`,
    net_var under `seed + 1`.  If `folder` already holds net_mean.pt it is loaded instead of trained, as the reference does; the
    folder's scales must then equal those of ds_train bit for bit (ValueError otherwise), and stats_mean.nc is not written.
    The epochs' shuffles come from numpy's global stream unless orders(epoch, n) gives them (both nets ask it from epoch 0)."""
    from ..models.mean_var_model import MeanVarModel
    num_epochs, batch_size = int(num_epochs), int(batch_size)
    _check_fit_args('fit_meanvar', num_epochs, batch_size, learning_rate)
    net_mean = FusedHeadCNN(2, 2, hidden_channels=hidden_channels, head='mse', seed=seed)
    net_var = FusedHeadCNN(2, 2, hidden_channels=hidden_channels, head='softplus_mse', seed=int(seed) + 1)
    X_train, Y_train, X_test, Y_test, x_scale, y_scale = prepare_PV_data(ds_train, ds_test)
    dev = torch.device('cuda', int(device)) if not isinstance(device, torch.device) else device
    X_train, Y_train, X_test, Y_test = (torch.as_tensor(a).to(dev) for a in (X_train, Y_train, X_test, Y_test))
    fit = dict(num_epochs=num_epochs, batch_size=batch_size, learning_rate=learning_rate, device=dev, orders=orders, verbose=verbose)
    if os.path.exists(os.path.join(folder, 'net_mean.pt')):
        for name, have in (('x_scale.json', x_scale), ('y_scale.json', y_scale)):
            old = ChannelwiseScaler().read(name, folder)
            if not (np.array_equal(old.std.reshape(-1), have.std.reshape(-1)) and np.array_equal(old.mean.reshape(-1), have.mean.reshape(-1))):
                raise ValueError(f'fit_meanvar: {os.path.join(folder, name)} is not the scale of ds_train: net_mean.pt of this '
                                 'folder was trained on other data')
        if verbose:
            print('Net mean is loaded instead of training')
        net_mean.load_state_dict(torch.load(os.path.join(folder, 'net_mean.pt'), map_location='cpu', weights_only=True))
        net_mean.to(dev)
    else:
        train(net_mean, X_train, Y_train, X_test, Y_test, **fit)
    with torch.cuda.device(dev):
        rsq_train = squared_residuals(net_mean, X_train, Y_train, batch_size)
        rsq_test = squared_residuals(net_mean, X_test, Y_test, batch_size)
    train(net_var, X_train, rsq_train, X_test, rsq_test, **fit)
    write_meanvar_folder(folder, net_mean.state_dict(), net_var.state_dict(), x_scale, y_scale, net_mean.hidden_channels,
                         net_mean.log_dict, net_var.log_dict)
    model = MeanVarModel(folder=folder, hidden_channels=list(net_mean.hidden_channels), device=device)
    model.trained_net_mean, model.trained_net_var = net_mean, net_var
    return model


def fit_ols(ds_train, ds_test, *, div=False, batch_norm=True, bias=True, final_activation='None',
            hidden_channels=[128, 64, 32, 32, 32, 32, 32], folder='model', num_epochs=50, batch_size=64, learning_rate=0.001,
            seed=0, device=0, orders=None, verbose=True):
    """OLSModel(...).fit(ds_train, ds_test, num_epochs, batch_size, learning_rate) on the device, then save_model; returns
    OLSModel(folder=folder) read back from the files.  The net is initialised with torch's Conv2d / BatchNorm2d defaults
    under `seed` (the reference's OLSModel does not call weights_init); the epochs' shuffles come from numpy's global
    stream unless orders(epoch, n) gives them."""
    from ..models.ols_model import OLSModel
    num_epochs, batch_size = int(num_epochs), int(batch_size)
    _check_fit_args('fit_ols', num_epochs, batch_size, learning_rate)
    net = TrainableAndrewCNN(2, 2, hidden_channels=hidden_channels, batch_norm=batch_norm, bias=bias, div=div,
                             final_activation=final_activation, seed=seed)
    X_train, Y_train, X_test, Y_test, x_scale, y_scale = prepare_PV_data(ds_train, ds_test)
    train(net, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, device=device, orders=orders, verbose=verbose)
    args = dict(div=bool(div), batch_norm=bool(batch_norm), bias=bool(bias), final_activation=final_activation,
                hidden_channels=list(net.hidden_channels))
    write_model_folder(folder, net.state_dict(), x_scale, y_scale, args, net.log_dict)
    model = OLSModel(**args, folder=folder, device=device)
    model.trained_net = net
    return model


def _open(pattern):
    from .simulate import dataset_backend
    xr = dataset_backend()
    return xr.open_mfdataset(pattern.strip(), combine='nested', concat_dim='run')


def main(argv=None):
    import argparse
    import ast
    parser = argparse.ArgumentParser(description='train OLSModel or MeanVarModel on the device and write its model folder')
    parser.add_argument('--model', type=str, default='OLSModel', choices=['OLSModel', 'MeanVarModel'])
    parser.add_argument('--train', type=str, required=True, help='glob of training files, concatenated along run')
    parser.add_argument('--validate', type=str, required=True)
    parser.add_argument('--test', type=str, default=None, help='glob of files for test_offline')
    parser.add_argument('--model_args', type=str, default=str({}))
    parser.add_argument('--fit_args', type=str, default=str({}))
    args = parser.parse_args(argv)
    print(args)
    model_args, fit_args = ast.literal_eval(args.model_args), ast.literal_eval(args.fit_args)
    if not isinstance(model_args, dict) or not isinstance(fit_args, dict):
        raise ValueError('--model_args and --fit_args are dict literals')
    fit = fit_ols if args.model == 'OLSModel' else fit_meanvar
    model = fit(_open(args.train), _open(args.validate), **model_args, **fit_args)
    if args.test:
        model.test_offline(_open(args.test)).to_netcdf(os.path.join(model.folder, 'offline.nc'))
    return model


if __name__ == '__main__':
    main()
