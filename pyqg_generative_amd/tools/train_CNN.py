"""Training of OLSModel on the device (reference: models/ols_model.py:35-57 fit / save_model, tools/cnn_tools.py:125-182
AndrewCNN, :402-421 prepare_PV_data, :607-700 minibatch / evaluate_test / train).

The convolutions — more than 95 % of a step's FLOPs — are the HIP kernels of csrc/conv_train.hip behind
``circular_conv2d``, a torch.autograd.Function over the three entry points of include/qgx_conv_train.h.  BatchNorm's batch
statistics, ReLU, the MSE, Adam and the learning-rate schedule are torch ops on device tensors, and autograd does their
backward.  ``fit_ols`` writes the reference's model folder (net.pt, x_scale.json, y_scale.json, model_args.json, stats.nc)
and returns ``OLSModel(folder=...)`` read back from those files.

Command line:
    python -m pyqg_generative_amd.tools.train_CNN --train 'GLOB' --validate 'GLOB' [--test 'GLOB'] \\
        --model_args "{'hidden_channels': [128, 64, 32, 32, 32, 32, 32]}" --fit_args "{'num_epochs': 50}"
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


def evaluate_test(net, X, Y, batch_size=64, acc=None):
    """evaluate_test (cnn_tools.py:624-643): eval mode, no gradients; sum over the batches of loss * n into acc[0], n into acc[1]"""
    net.eval()
    with torch.no_grad():
        for s in range(0, len(X), batch_size):
            x, y = X[s:s + batch_size], Y[s:s + batch_size]
            acc[0] += net.compute_loss(x, y)['loss'].to(torch.float64) * len(x)
            acc[1] += len(x)
    net.train()


def train(net, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, device=0, orders=None, verbose=True):
    """train (cnn_tools.py:645-700) with the data resident on the device: Adam, MultiStepLR with milestones int(E / 2),
    int(3 E / 4), int(7 E / 8) stepped per epoch, a shuffle of the samples per epoch (numpy's global stream, as minibatch
    does; orders(epoch, n) replaces it), evaluate_test in eval mode, net.log_dict with 'loss' and 'loss_test' per epoch.
    The losses are accumulated on the device and read back once per epoch."""
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
            order = torch.as_tensor(order).to(dev)
            for s in range(0, n, batch_size):
                idx = order[s:s + batch_size]
                x, y = X_train[idx], Y_train[idx]
                optimizer.zero_grad()
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
    from .simulate import dataset_backend
    os.makedirs(folder, exist_ok=True)
    torch.save({k: v.detach().cpu().clone() for k, v in state_dict.items()}, os.path.join(folder, 'net.pt'))
    x_scale.write('x_scale.json', folder=folder)
    y_scale.write('y_scale.json', folder=folder)
    with open(os.path.join(folder, 'model_args.json'), 'w') as f:
        json.dump(dict(model='OLSModel', **model_args), f)
    xr = dataset_backend()
    E = len(next(iter(log.values())))
    stats = xr.Dataset({k: (['epoch'], np.asarray(v, dtype=np.float64)) for k, v in log.items()},
                       coords={'epoch': np.arange(1, E + 1)})
    path = os.path.join(folder, 'stats.nc')
    if os.path.exists(path):
        os.remove(path)
    stats.to_netcdf(path)


def fit_ols(ds_train, ds_test, *, div=False, batch_norm=True, bias=True, final_activation='None',
            hidden_channels=[128, 64, 32, 32, 32, 32, 32], folder='model', num_epochs=50, batch_size=64, learning_rate=0.001,
            seed=0, device=0, orders=None, verbose=True):
    """OLSModel(...).fit(ds_train, ds_test, num_epochs, batch_size, learning_rate) on the device, then save_model; returns
    OLSModel(folder=folder) read back from the files.  The net is initialised with torch's Conv2d / BatchNorm2d defaults
    under `seed` (the reference's OLSModel does not call weights_init); the epochs' shuffles come from numpy's global
    stream unless orders(epoch, n) gives them."""
    from ..models.ols_model import OLSModel
    num_epochs, batch_size = int(num_epochs), int(batch_size)
    if batch_size < 1:
        raise ValueError(f'fit_ols: batch_size = {batch_size}')
    if num_epochs < 1:
        raise ValueError(f'fit_ols: num_epochs = {num_epochs}')
    if not (math.isfinite(learning_rate) and learning_rate >= 0):
        raise ValueError(f'fit_ols: learning_rate = {learning_rate}')
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
    parser = argparse.ArgumentParser(description='train OLSModel on the device and write its model folder')
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
    model = fit_ols(_open(args.train), _open(args.validate), **model_args, **fit_args)
    if args.test:
        model.test_offline(_open(args.test)).to_netcdf(os.path.join(model.folder, 'offline.nc'))
    return model


if __name__ == '__main__':
    main()
