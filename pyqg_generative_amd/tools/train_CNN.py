"""Training of OLSModel on the device (reference: models/ols_model.py:35-57 fit / save_model, tools/cnn_tools.py:125-182
AndrewCNN, :402-421 prepare_PV_data, :607-700 minibatch / evaluate_test / train).

This module holds the nets, the loop, the data preparation, the folder writers and the fits.  The device operations of a
step (the convolutions, the batch gather, the loss head) are in tools/train_ops.py, what every fit shares in
tools/train_common.py.  BatchNorm's batch statistics, ReLU, the MSE, Adam and the learning-rate schedule are torch ops on
device tensors, and autograd does their backward.  ``fit_ols(div=True)`` trains the flux-form net, ``FluxFormCNN``, whose
forward ends in the device's spectral divergence (train_ops.flux_divergence).  ``fit_ols`` writes the reference's model folder (net.pt, x_scale.json,
y_scale.json, model_args.json, stats.nc) and returns ``OLSModel(folder=...)`` read back from those files.

Training of MeanVarModel (reference: models/mean_var_model.py:14-17 VarCNN, :41-80 fit / save_model): ``fit_meanvar`` trains
net_mean, evaluates it over both sets and trains net_var on the squared residuals.  Its nets are ``FusedHeadCNN``s.

Command line:
    python -m pyqg_generative_amd.tools.train_CNN [--model OLSModel|MeanVarModel] --train 'GLOB' --validate 'GLOB' \\
        [--test 'GLOB'] --model_args "{'hidden_channels': [128, 64, 32, 32, 32, 32, 32]}" --fit_args "{'num_epochs': 50}"
"""
import json
import os
from time import time

import numpy as np
import torch
from torch import nn

from .. import weights as _weights
from .cnn_tools import ChannelwiseScaler
from .train_common import check_fit_args, command_line, cuda_device, log_epoch, print_start, save_state_dict, stacked, write_log
from .train_ops import GRIDS, circular_conv2d, flux_divergence, gather_batch, head_apply, head_loss, head_mode, to_engine_layout


def _pad(v, n):
    return v if v.shape[0] == n else torch.nn.functional.pad(v, (0, n - v.shape[0]))


class TrainableAndrewCNN(nn.Module):
    """AndrewCNN(n_in, n_out, batch_norm=, bias=, hidden_channels=) (cnn_tools.py:125-182) with the reference's state dict —
    `conv` is the same nn.Sequential of Conv2d / ReLU / BatchNorm2d modules, which hold the parameters and buffers and give
    torch's default initialisation, drawn on the CPU under `seed` — and a forward on the device kernels: activations stay
    in the engine layout (B, N, N, C8) between layers, ReLU and BatchNorm are torch expressions on them with the
    per-channel vectors padded by zeros to C8, so the pad channels stay zero."""

    FLUX_FORM = False        # FluxFormCNN: the last convolution writes 2 n_out fluxes and the divergence follows it

    def __init__(self, n_in, n_out, hidden_channels=(128, 64, 32, 32, 32, 32, 32), batch_norm=True, bias=True, div=False,
                 final_activation='None', seed=0):
        super().__init__()
        if div and not self.FLUX_FORM:
            raise NotImplementedError('div=True: a flux-form net is a FluxFormCNN, which ends in the divergence kernels; this '
                                      'class has no divergence behind its last convolution')
        if final_activation != 'None':
            raise NotImplementedError(f'final_activation={final_activation!r} has no device path')
        hidden = _weights.check_hidden_channels(hidden_channels)
        self.n_in, self.n_out, self.hidden_channels = int(n_in), int(n_out), hidden
        self.batch_norm, self.bias = bool(batch_norm), bool(bias)
        ch = [self.n_in] + hidden + [2 * self.n_out if self.FLUX_FORM else self.n_out]
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

    def _input(self, x):
        """x planar (B, n_in, N, N) with N an admitted grid, as float32"""
        if x.dim() != 4 or x.shape[1] != self.n_in or x.shape[-1] != x.shape[-2] or int(x.shape[-1]) not in GRIDS:
            raise ValueError(f'input {tuple(x.shape)}: expected (B, {self.n_in}, N, N) with N one of {GRIDS}')
        return x.to(torch.float32)

    def forward(self, x):
        """x planar (B, n_in, N, N) on the device -> planar (B, n_out, N, N)"""
        y = self.forward_engine(to_engine_layout(self._input(x)))
        return y[..., :self.n_out].permute(0, 3, 1, 2)

    def compute_loss(self, x, ytrue):
        return {'loss': nn.functional.mse_loss(self.forward(x), ytrue)}


class FluxFormCNN(TrainableAndrewCNN):
    """AndrewCNN(n_in, n_out, div=True, ...) (cnn_tools.py:100-123, 139-142, 170-175): the last convolution writes 2 n_out
    fluxes [fx of both layers, fy of both layers] and the net returns 10000 * divergence(fluxes), so its output has zero
    spatial mean by construction.  The state dict is the reference's div=True net's (a last weight of 2 n_out outputs), the
    seeded initialisation follows the parent's rule, and the divergence is train_ops.flux_divergence: the kernel body the
    generators run at inference forward, its adjoint backward.  n_out = 2 only: the kernels take the two layers' fluxes."""

    FLUX_FORM = True

    def __init__(self, n_in, n_out, hidden_channels=(128, 64, 32, 32, 32, 32, 32), batch_norm=True, bias=True,
                 final_activation='None', seed=0):
        if int(n_out) != 2:
            raise ValueError(f'n_out = {n_out}: the divergence kernels take the fluxes of 2 layers')
        super().__init__(n_in, n_out, hidden_channels=hidden_channels, batch_norm=batch_norm, bias=bias, div=True,
                         final_activation=final_activation, seed=seed)

    def forward_engine(self, a):
        """(B, N, N, c8(n_in)) -> (B, N, N, 8) with channels [y1, y2, 0, ...]"""
        return flux_divergence(super().forward_engine(a))


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
        head_mode(head)
        if not (1 <= int(n_in) <= 8 and 1 <= int(n_out) <= 8):
            raise ValueError(f'n_in = {n_in}, n_out = {n_out}: the fused ends take 1 ... 8 channels')
        super().__init__(n_in, n_out, hidden_channels=hidden_channels, seed=seed)
        self.head = head

    def forward(self, x):
        x = self._input(x)
        with torch.no_grad():
            return head_apply(self.forward_engine(gather_batch(x)), self.n_out, self.head)

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
    dev = cuda_device(device)
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if not torch.is_tensor(a) else a.to(dev, torch.float32)
    X_train, Y_train, X_test, Y_test = (as_dev(a) for a in (X_train, Y_train, X_test, Y_test))
    n = len(X_train)
    print_start(dev, n, verbose)
    net.to(dev)
    net.train()
    optimizer = torch.optim.Adam(net.parameters(), lr=learning_rate)
    E = int(num_epochs)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    if not hasattr(net, 'log_dict'):
        net.log_dict = {}
    log = net.log_dict
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
            log_epoch(log, acc.cpu().numpy(), epoch, E, t_e, t_s, verbose)       # the epoch's one host read
    return net


def extract(ds, key, who='fit_ols'):
    """extract (cnn_tools.py:398-400): ds[key] (run, time, lev, y, x) -> (run * time, lev, y, x)"""
    v = stacked(ds, key, who)
    if v.shape[-1] != v.shape[-2] or v.shape[-1] not in GRIDS:
        raise ValueError(f'{key}: a {v.shape[-2]} x {v.shape[-1]} grid; the device trains on square grids of {GRIDS}')
    if v.shape[2] != 2:
        raise ValueError(f'{key}: {v.shape[2]} levels, expected 2')
    return v.reshape((-1,) + v.shape[2:])


def channel_scaler(X):
    """ChannelwiseScaler(X) (cnn_tools.py:458-515): per-channel mean and population std in float64, cast to float32"""
    X = np.asarray(X, dtype=np.float64)
    return ChannelwiseScaler(std=X.std(axis=(0, 2, 3)).astype('float32'), mean=X.mean(axis=(0, 2, 3)).astype('float32'))


def prepare_PV_data(ds_train, ds_test, who='fit_ols'):
    """prepare_PV_data (cnn_tools.py:402-421): q and q_forcing_advection divided by the training set's channelwise std"""
    X_train, Y_train = extract(ds_train, 'q', who), extract(ds_train, 'q_forcing_advection', who)
    X_test, Y_test = extract(ds_test, 'q', who), extract(ds_test, 'q_forcing_advection', who)
    x_scale, y_scale = channel_scaler(X_train), channel_scaler(Y_train)
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    return (f32(x_scale.normalize(X_train)), f32(y_scale.normalize(Y_train)), f32(x_scale.normalize(X_test)),
            f32(y_scale.normalize(Y_test)), x_scale, y_scale)


def _write_folder(folder, states, x_scale, y_scale, model_args):
    """what both model folders hold: {file: state dict} as CPU state dicts, x_scale.json, y_scale.json, model_args.json"""
    os.makedirs(folder, exist_ok=True)
    for name, state in states.items():
        save_state_dict(os.path.join(folder, name), state)
    x_scale.write('x_scale.json', folder=folder)
    y_scale.write('y_scale.json', folder=folder)
    with open(os.path.join(folder, 'model_args.json'), 'w') as f:
        json.dump(model_args, f)


def write_model_folder(folder, state_dict, x_scale, y_scale, model_args, log):
    """OLSModel.save_model (ols_model.py:48-57): net.pt (CPU state dict), x_scale.json, y_scale.json, model_args.json with
    model: 'OLSModel' and the constructor arguments, stats.nc (log_to_xarray: one variable per key over `epoch`)"""
    _write_folder(folder, {'net.pt': state_dict}, x_scale, y_scale, dict(model='OLSModel', **model_args))
    write_log(os.path.join(folder, 'stats.nc'), log)


def write_meanvar_folder(folder, mean_state, var_state, x_scale, y_scale, hidden_channels, log_mean, log_var):
    """MeanVarModel.save_model (mean_var_model.py:68-80): net_mean.pt, net_var.pt (CPU state dicts), x_scale.json,
    y_scale.json, model_args.json with model: 'MeanVarModel' and hidden_channels, stats_mean.nc — not written without a log:
    a net_mean read from the folder has none — and stats_var.nc"""
    _write_folder(folder, {'net_mean.pt': mean_state, 'net_var.pt': var_state}, x_scale, y_scale,
                  dict(model='MeanVarModel', hidden_channels=[int(c) for c in hidden_channels]))
    if log_mean and log_mean.get('loss'):
        write_log(os.path.join(folder, 'stats_mean.nc'), log_mean)
    write_log(os.path.join(folder, 'stats_var.nc'), log_var)


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
    check_fit_args('fit_meanvar', num_epochs, batch_size, learning_rate)
    net_mean = FusedHeadCNN(2, 2, hidden_channels=hidden_channels, head='mse', seed=seed)
    net_var = FusedHeadCNN(2, 2, hidden_channels=hidden_channels, head='softplus_mse', seed=int(seed) + 1)
    X_train, Y_train, X_test, Y_test, x_scale, y_scale = prepare_PV_data(ds_train, ds_test, 'fit_meanvar')
    dev = cuda_device(device)
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
    stream unless orders(epoch, n) gives them.  div=True trains a FluxFormCNN: the folder's model_args.json says "div": true
    and the model read back runs the four-channel last layer with the device's divergence behind it."""
    from ..models.ols_model import OLSModel
    num_epochs, batch_size = int(num_epochs), int(batch_size)
    check_fit_args('fit_ols', num_epochs, batch_size, learning_rate)
    net_args = dict(hidden_channels=hidden_channels, batch_norm=batch_norm, bias=bias, final_activation=final_activation, seed=seed)
    net = FluxFormCNN(2, 2, **net_args) if div else TrainableAndrewCNN(2, 2, **net_args)
    X_train, Y_train, X_test, Y_test, x_scale, y_scale = prepare_PV_data(ds_train, ds_test, 'fit_ols')
    train(net, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, device=device, orders=orders, verbose=verbose)
    args = dict(div=bool(div), batch_norm=bool(batch_norm), bias=bool(bias), final_activation=final_activation,
                hidden_channels=list(net.hidden_channels))
    write_model_folder(folder, net.state_dict(), x_scale, y_scale, args, net.log_dict)
    model = OLSModel(**args, folder=folder, device=device)
    model.trained_net = net
    return model


def main(argv=None):
    return command_line('train OLSModel or MeanVarModel on the device and write its model folder',
                        {'OLSModel': fit_ols, 'MeanVarModel': fit_meanvar}, argv)


if __name__ == '__main__':
    main()
