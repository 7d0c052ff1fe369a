"""Training of CVAERegression on the device (reference: models/cvae_regression.py:18-52 the three nets, :54-89 fit /
save_model, :165-231 forward / compute_loss, :233-320 evaluate_prediction / loss_to_xarray / train_CVAE).

The nets are the trainable nets of tools/train_CNN.py (FluxFormCNN where div=True).  A training step is gather_batch ->
encoder -> latent_sample -> decoder -> head_loss: between the encoder's last convolution and the decoder's first, the
reparameterised sample, the KL divergence and the variance diagnostics are one call of csrc/latent_train.hip each way
(train_ops.latent_sample), the latent noise is drawn there from the Philox stream, and nothing is read back to the host within
an epoch: the decoder variance of decoder_var='adaptive' is the detached MSE as a device number.  ``fit_cvae`` writes the
reference's model folder (encoder.pt, decoder.pt, [net_mean.pt], x_scale.json, y_scale.json, model_args.json, stats.nc,
[stats_mean.nc]) and returns ``CVAERegression(folder=...)`` read back from those files.

Command line:
    python -m pyqg_generative_amd.tools.train_CVAE --train 'GLOB' --validate 'GLOB' [--test 'GLOB'] \\
        --model_args "{'regression': 'full_loss', 'folder': 'model'}" --fit_args "{'num_epochs': 200}"
"""
import math
import os
from itertools import chain
from time import time

import numpy as np
import torch
from torch import nn

from .train_common import check_fit_args, command_line, cuda_device, print_start, stacked, write_log
from .train_CNN import FluxFormCNN, TrainableAndrewCNN, _write_folder, prepare_PV_data, train
from .train_ops import gather_batch, head_apply, head_loss, latent_prior, latent_sample

KEYS = ('loss', 'loss_recon', 'loss_KL', 'MSE', 'var_latent', 'var_aggr')        # what compute_loss returns (:230-231)
SCORES = ('L2_mean', 'L2_total', 'L2_residual', 'var_ratio')                      # what evaluate_prediction returns (:243)
REGRESSIONS = ('None', 'full_loss')
_U64 = (1 << 64) - 1


def check_decoder_var(decoder_var):
    """'adaptive', 'fixed' or a positive finite number (cvae_regression.py:209-216)"""
    if decoder_var in ('adaptive', 'fixed'):
        return decoder_var
    if isinstance(decoder_var, (int, float)) and not isinstance(decoder_var, bool) and math.isfinite(decoder_var) and decoder_var > 0:
        return float(decoder_var)
    raise ValueError(f"decoder_var={decoder_var!r}: 'adaptive', 'fixed' or a positive finite number")


class TrainableCVAE(nn.Module):
    """The nets of CVAERegression(regression, decoder_var, div=, hidden_channels=) (cvae_regression.py:45-50) with the
    reference's state dicts, and its loss:

      encoder    AndrewCNN(4, 4) with the default widths, always: [x, y] -> [mu, logvar]                     initialised under seed
      decoder    AndrewCNN(4, 2, div, hidden_channels): [x, z] -> y                                          under seed + 1
      net_mean   AndrewCNN(2, 2, div) with the default widths, with regression='full_loss' only              under seed + 2

    The seeds are `seed`, `seed + 1`, `seed + 2`; the latent noise of training is the Philox stream of key `seed`, that of
    prediction the stream of key `seed + 1`.

      compute_loss(x, y, ymean, eps)           the reference's statement (:165-231) in torch expressions on planar device tensors,
                                               with eps given: what tests and a reader compare against
      indexed_loss(XY, X, T, idx, step)        the same six values for x = X[idx], y - ymean = T[idx] of device-resident sets,
                                               XY = cat([X, Y], 1): gather_batch -> encoder -> latent_sample -> decoder ->
                                               head_loss; what train_CVAE runs"""

    def __init__(self, regression='None', decoder_var='adaptive', div=False, hidden_channels=(128, 64, 32, 32, 32, 32, 32), seed=0):
        super().__init__()
        if regression not in REGRESSIONS:
            raise ValueError(f'regression={regression!r}: one of {REGRESSIONS}')
        self.regression, self.decoder_var, self.div, self.seed = regression, check_decoder_var(decoder_var), bool(div), int(seed)
        if not 0 <= self.seed < _U64:
            raise ValueError(f'seed = {seed}: 0 ... 2^64 - 2')
        net = FluxFormCNN if self.div else TrainableAndrewCNN
        self.encoder = TrainableAndrewCNN(4, 4, seed=self.seed)
        self.decoder = net(4, 2, hidden_channels=hidden_channels, seed=self.seed + 1)
        self.hidden_channels = list(self.decoder.hidden_channels)
        if regression != 'None':
            self.net_mean = net(2, 2, seed=self.seed + 2)
        self.x_scale = self.y_scale = None          # fit_cvae sets them; evaluate_prediction needs them

    def trained_parameters(self):
        """what train_CVAE's Adam steps (:280): encoder and decoder, never net_mean"""
        return chain(self.encoder.parameters(), self.decoder.parameters())

    def _recon(self, mse, N):
        """loss_recon = sum over pixels and channels, mean over the batch, of the squares / (2 var_p) = mse 2 N^2 / (2 var_p)"""
        var_p = mse.detach() if self.decoder_var == 'adaptive' else 1.0 if self.decoder_var == 'fixed' else self.decoder_var
        return mse * (2 * N * N) / (2. * var_p)

    def compute_loss(self, x, y, ymean, eps):
        mu, logvar = torch.split(self.encoder(torch.cat([x, y], dim=1)), 2, dim=1)
        std = torch.exp(0.5 * logvar)
        var = torch.square(std)
        yhat = self.decoder(torch.cat([x, eps * std + mu], dim=1))
        if self.regression != 'None':
            yhat = yhat + ymean
        mse = torch.square(yhat - y).mean()
        loss_KL = (0.5 * (torch.square(mu) + var - 1 - logvar)).sum(dim=(1, 2, 3)).mean()
        loss_recon = self._recon(mse, int(x.shape[-1]))
        with torch.no_grad():
            var_latent = var.mean()
            var_aggr = mu.var() + var_latent
        return {'loss': loss_recon + loss_KL, 'loss_recon': loss_recon, 'loss_KL': loss_KL, 'MSE': mse.detach(),
                'var_latent': var_latent, 'var_aggr': var_aggr}

    def indexed_loss(self, XY, X, T, idx, step, eps=None):
        """T = Y - Y_mean: the reference's `yhat += ymean` moved to the target.  Every value is a 0-dim float64 device tensor"""
        enc = self.encoder.forward_engine(gather_batch(XY, idx))
        dec_in, loss_KL, var_latent, var_aggr = latent_sample(enc, X, idx, self.seed, step, eps)
        mse = head_loss(self.decoder.forward_engine(dec_in), T, idx, 'mse')
        loss_recon = self._recon(mse, int(X.shape[-1]))
        return {'loss': loss_recon + loss_KL, 'loss_recon': loss_recon, 'loss_KL': loss_KL, 'MSE': mse.detach(),
                'var_latent': var_latent, 'var_aggr': var_aggr}


def _forward_all(net, X, batch_size=64):
    """net(X) of the eval-mode net over the device-resident set, in batches, planar"""
    out = torch.empty((len(X), net.n_out) + tuple(X.shape[2:]), dtype=torch.float32, device=X.device)
    net.eval()
    with torch.no_grad():
        for s in range(0, len(X), batch_size):
            head_apply(net.forward_engine(gather_batch(X[s:s + batch_size])), net.n_out, 'mse', out=out[s:s + batch_size])
    net.train()
    return out


def evaluate_prediction(net, ds, nruns=None, M=16, runs=None, device=0, batch_size=64):
    """evaluate_prediction (cvae_regression.py:233-243) with predict (:147-163) at M draws: nruns runs of ds chosen without
    replacement from numpy's global stream (runs(R, nruns) replaces the choice), M draws of the latent noise from the prior
    through the eval-mode decoder, the first sample and the mean over the M, plus net_mean, denormalized, and scored on the
    device (computational_tools.OfflineStats) -> {'L2_mean', 'L2_total', 'L2_residual': float, 'var_ratio': (lev,)}.  The
    draws are the Philox stream of key net.seed + 1, the step a counter of the calls made (net.prior_draws)."""
    from .computational_tools import OfflineStats, _scores
    dev = cuda_device(device)
    q, y = stacked(ds, 'q', 'evaluate_prediction'), stacked(ds, 'q_forcing_advection', 'evaluate_prediction')
    R = len(q)
    if nruns is not None and nruns < R:
        pick = np.asarray(np.random.choice(np.arange(R), nruns, replace=False) if runs is None else runs(R, nruns), dtype=np.int64)
        if not (pick.shape == (nruns,) and len(set(pick.tolist())) == nruns and pick.min() >= 0 and pick.max() < R):
            raise ValueError(f'runs({R}, {nruns}): not {nruns} different runs of 0 ... {R - 1}')
        q, y = q[pick], y[pick]
    shape = q.shape
    with torch.cuda.device(dev):
        X = torch.as_tensor(np.ascontiguousarray(net.x_scale.normalize(q.reshape((-1,) + shape[2:])), dtype=np.float32)).to(dev)
        first, mean = torch.empty_like(X), torch.empty_like(X)
        net.decoder.to(dev).eval()
        with torch.no_grad():
            for s in range(0, len(X), batch_size):
                x = X[s:s + batch_size]
                acc = None
                for m in range(int(M)):
                    net.prior_draws = getattr(net, 'prior_draws', 0) + 1
                    yhat = head_apply(net.decoder.forward_engine(latent_prior(x, None, net.seed + 1, net.prior_draws - 1)), 2, 'mse')
                    if m == 0:
                        first[s:s + batch_size] = yhat
                    acc = yhat if acc is None else acc + yhat
                mean[s:s + batch_size] = acc / int(M)
        net.decoder.train()
        if net.regression != 'None':
            corr = _forward_all(net.net_mean.to(dev), X, batch_size)
            first, mean = first + corr, mean + corr
        ystd = torch.as_tensor(np.asarray(net.y_scale.std, dtype=np.float32)).to(dev)
        st = OfflineStats(np.ascontiguousarray(y), (mean * ystd).reshape(shape), (first * ystd).reshape(shape),
                          device=torch.cuda.current_device())
    scores = _scores(st)
    return {k: np.asarray(scores[k].values, dtype=np.float64) if k == 'var_ratio' else float(np.asarray(scores[k].values)) for k in SCORES}


def train_CVAE(net, X_train, Y_train, num_epochs, batch_size, learning_rate, ds_train=None, ds_test=None, nruns=5, device=0,
               orders=None, runs=None, verbose=True):
    """train_CVAE (cvae_regression.py:256-320) with the data resident on the device: one Adam over the encoder's and the
    decoder's parameters, MultiStepLR with milestones int(E / 2), int(3 E / 4), int(7 E / 8) and gamma 0.1 stepped per epoch, a
    shuffle of the samples per epoch (numpy's global stream, as minibatch does; orders(epoch, n) replaces it and is checked on
    the host, since the gather kernels do not check it), Y_mean = net_mean(X_train) in eval mode with regression, else 0.
    The Philox step of a training batch's latent noise is a counter of the calls made, from 0.  The weighted means of the six
    losses are accumulated on the device and read once per epoch.  With ds_train and ds_test, evaluate_prediction scores
    nruns runs of each after every epoch.  Returns (optim_loss, log_train, log_test): {key: [per epoch]} and two lists of
    evaluate_prediction's dicts (empty without datasets)."""
    dev = cuda_device(device)
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if not torch.is_tensor(a) else a.to(dev, torch.float32)
    X, Y = as_dev(X_train), as_dev(Y_train)
    n, E, batch_size = len(X), int(num_epochs), int(batch_size)
    print_start(dev, n, verbose)
    net.to(dev)
    optim_loss, log_train, log_test = {k: [] for k in KEYS}, [], []
    t_s = time()
    with torch.cuda.device(dev):
        T = Y - _forward_all(net.net_mean, X, batch_size) if net.regression != 'None' else Y
        XY = torch.cat([X, Y], dim=1)
        net.encoder.train()
        net.decoder.train()
        optimizer = torch.optim.Adam(net.trained_parameters(), lr=learning_rate)
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
        step = 0
        for epoch in range(E):
            t_e = time()
            acc = torch.zeros((len(KEYS) + 1,), dtype=torch.float64, device=dev)
            order = np.arange(n)
            if orders is None:
                np.random.shuffle(order)
            else:
                order = np.asarray(orders(epoch, n), dtype=np.int64)
            if not (order.shape == (n,) and order.min() >= 0 and order.max() < n):
                raise ValueError(f'orders({epoch}, {n}): not {n} indices in 0 ... {n - 1}')      # the kernels do not check them
            order = torch.as_tensor(order).to(dev)
            for s in range(0, n, batch_size):
                idx = order[s:s + batch_size]
                optimizer.zero_grad()
                losses = net.indexed_loss(XY, X, T, idx, step)
                step += 1
                losses['loss'].backward()
                optimizer.step()
                acc[:-1] += torch.stack([losses[k].detach().to(torch.float64) for k in KEYS]) * len(idx)
                acc[-1] += len(idx)
            scheduler.step()
            a = acc.cpu().numpy()                                                       # the epoch's one host read of the losses
            for i, k in enumerate(KEYS):
                optim_loss[k].append(float(a[i] / a[-1]))
            if ds_train is not None and ds_test is not None:
                log_train.append(evaluate_prediction(net, ds_train, nruns, runs=runs, device=dev, batch_size=batch_size))
                log_test.append(evaluate_prediction(net, ds_test, nruns, runs=runs, device=dev, batch_size=batch_size))
            if verbose:
                t = time()
                line = '[%d/%d] [%.2f/%.2f] MSE/KL: [%.3f, %.3f] Var: [%.3f,%.3f]' % (
                    epoch + 1, E, t - t_e, (t - t_s) * (E / (epoch + 1) - 1), optim_loss['MSE'][-1], optim_loss['loss_KL'][-1],
                    optim_loss['var_latent'][-1], optim_loss['var_aggr'][-1])
                if log_train:
                    a, b = log_train[-1], log_test[-1]
                    line += ' L2_mean: [%.3f,%.3f] L2_total: [%.3f,%.3f] L2_res: [%.3f,%.3f] Var_ratio: [%.3f, %.3f]' % (
                        a['L2_mean'], b['L2_mean'], a['L2_total'], b['L2_total'], a['L2_residual'], b['L2_residual'],
                        a['var_ratio'][0], a['var_ratio'][1])
                print(line)
    return optim_loss, log_train, log_test


def loss_to_dataset(optim_loss, log_train, log_test):
    """loss_to_xarray (cvae_regression.py:245-254) -> (dataset, Epoch_opt): the six losses over `epoch` (1 ... E); L2_mean,
    L2_total, L2_residual of the training runs, and of the test runs as L2_mean_test, L2_total_test, L2_residual_test;
    L2_loss = L2_total_test + L2_residual_test and Epoch_opt, the epoch (counted from 1) of its minimum.  As the reference
    builds it, the test log's var_ratio is NOT renamed and therefore replaces the training log's: var_ratio (epoch, lev) is
    that of the test runs."""
    from .simulate import dataset_backend
    xr = dataset_backend()
    E = len(optim_loss['loss'])
    if len(log_train) != E or len(log_test) != E:
        raise ValueError(f'{E} epochs of losses, {len(log_train)} and {len(log_test)} of scores')
    ds = xr.Dataset({k: (['epoch'], np.asarray(v, dtype=np.float64)) for k, v in optim_loss.items()}, coords={'epoch': np.arange(1, E + 1)})
    for k in SCORES[:3]:
        ds[k] = (['epoch'], np.array([float(e[k]) for e in log_train]))
    for k in SCORES[:3]:
        ds[k + '_test'] = (['epoch'], np.array([float(e[k]) for e in log_test]))
    ds['var_ratio'] = (['epoch', 'lev'], np.array([np.asarray(e['var_ratio'], dtype=np.float64) for e in log_test]))
    L2_loss = np.asarray(ds['L2_total_test'].values) + np.asarray(ds['L2_residual_test'].values)
    ds['L2_loss'] = (['epoch'], L2_loss)
    epoch_opt = int(np.argmin(L2_loss)) + 1
    ds['Epoch_opt'] = epoch_opt
    return ds, epoch_opt


def write_cvae_folder(folder, net, x_scale, y_scale, optim_loss, log_train, log_test, verbose=True):
    """CVAERegression.save_model (cvae_regression.py:72-89): encoder.pt, decoder.pt, net_mean.pt with regression (CPU state
    dicts), x_scale.json, y_scale.json, model_args.json with model: 'CVAERegression' and regression, div, decoder_var,
    hidden_channels, stats.nc (loss_to_dataset), stats_mean.nc (net_mean's log) with regression.  Returns Epoch_opt; as in the
    reference, the LAST epoch's nets are the ones written."""
    states = {'encoder.pt': net.encoder.state_dict(), 'decoder.pt': net.decoder.state_dict()}
    if net.regression != 'None':
        states['net_mean.pt'] = net.net_mean.state_dict()
    _write_folder(folder, states, x_scale, y_scale, dict(model='CVAERegression', regression=net.regression, div=net.div,
                                                         decoder_var=net.decoder_var, hidden_channels=list(net.hidden_channels)))
    stats, epoch_opt = loss_to_dataset(optim_loss, log_train, log_test)
    path = os.path.join(folder, 'stats.nc')
    if os.path.exists(path):
        os.remove(path)
    stats.to_netcdf(path)
    if net.regression != 'None' and net.net_mean.log_dict.get('loss'):
        write_log(os.path.join(folder, 'stats_mean.nc'), net.net_mean.log_dict)
    if verbose:
        print('Optimal epoch:', epoch_opt)
        print('The Last epoch is used for prediction')
    return epoch_opt


def fit_cvae(ds_train, ds_test, *, regression='None', decoder_var='adaptive', div=False, hidden_channels=[128, 64, 32, 32, 32, 32, 32],
             folder='model', num_epochs=200, num_epochs_regression=50, batch_size=64, learning_rate=2e-4, nruns=5, seed=0, device=0,
             orders=None, runs=None, verbose=True):
    """CVAERegression(regression, decoder_var, folder, div, hidden_channels).fit(ds_train, ds_test, num_epochs,
    num_epochs_regression, batch_size, learning_rate, nruns) on the device (cvae_regression.py:54-89), then save_model; returns
    CVAERegression(folder=folder) read back from the files, with the trained nets attached as trained_encoder, trained_decoder
    and (with regression) trained_net_mean.

    With regression='full_loss', net_mean is first trained with MSE for num_epochs_regression epochs at learning rate 0.001
    (always: the reference's CVAE does not read a net_mean from the folder).  The nets are initialised with torch's defaults
    under seed, seed + 1 and seed + 2 (TrainableCVAE); the epochs' shuffles and the choice of the nruns scored runs come from
    numpy's global stream unless orders(epoch, n) and runs(R, nruns) give them."""
    from ..models.cvae_regression import CVAERegression
    num_epochs, num_epochs_regression, batch_size = int(num_epochs), int(num_epochs_regression), int(batch_size)
    check_fit_args('fit_cvae', num_epochs, batch_size, learning_rate)
    net = TrainableCVAE(regression, decoder_var, div, hidden_channels, seed)
    if regression != 'None':
        check_fit_args('fit_cvae', num_epochs_regression, batch_size, 0.001)
    X_train, Y_train, X_test, Y_test, net.x_scale, net.y_scale = prepare_PV_data(ds_train, ds_test, 'fit_cvae')
    dev = cuda_device(device)
    X_train, Y_train, X_test, Y_test = (torch.as_tensor(a).to(dev) for a in (X_train, Y_train, X_test, Y_test))
    if regression != 'None':
        train(net.net_mean, X_train, Y_train, X_test, Y_test, num_epochs_regression, batch_size, 0.001, device=dev, orders=orders,
              verbose=verbose)
    logs = train_CVAE(net, X_train, Y_train, num_epochs, batch_size, learning_rate, ds_train=ds_train, ds_test=ds_test, nruns=nruns,
                      device=dev, orders=orders, runs=runs, verbose=verbose)
    write_cvae_folder(folder, net, net.x_scale, net.y_scale, *logs, verbose=verbose)
    model = CVAERegression(regression=regression, folder=folder, div=net.div, decoder_var=net.decoder_var,
                           hidden_channels=list(net.hidden_channels), device=device)
    model.trained_encoder, model.trained_decoder = net.encoder, net.decoder
    if regression != 'None':
        model.trained_net_mean = net.net_mean
    return model


def main(argv=None):
    return command_line('train CVAERegression on the device and write its model folder', {'CVAERegression': fit_cvae}, argv)


if __name__ == '__main__':
    main()
