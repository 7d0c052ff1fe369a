"""Training of CGANRegression on the device (reference: models/cgan_regression.py:22-66 the nets, :68-107 fit / save_model,
:197-222 gradient_penalty, :224-245 evaluate_prediction / loss_to_xarray, :247-344 train_CGAN; tools/cnn_tools.py:54-65
weights_init, :212-244 DCGAN_discriminator).

The generator is a trainable net of tools/train_CNN.py (FluxFormCNN where div=True) on ``circular_conv2d``, which is
differentiable once: G needs no more.  The discriminator's four stride-2 layers are ``train_ops.strided_conv2d``, the kernels of
csrc/dconv_train.hip behind three autograd.Functions whose backwards are each other, so the gradient penalty's second derivative
through D runs on the same three kernels.  The data, the epoch's order and its interpolation weights are resident on the device,
the latent noise is drawn there from the Philox stream (two steps per batch), and the four losses are accumulated there and
read once per epoch.  ``fit_cgan`` writes the reference's model folder (G.pt, D.pt, [net_mean.pt], x_scale.json, y_scale.json,
model_args.json, stats.nc) and returns ``CGANRegression(folder=...)`` read back from those files.  ``fit_cgan_unet`` is the same
fit of ``CGANRegression(generator='DeepInversion')``: G is the U-Net of tools/train_UNet.py on ``train_ops.unet_conv2d``
(csrc/uconv_train.hip); the loop, D and the folder are the same.

Command line:
    python -m pyqg_generative_amd.tools.train_CGAN --train 'GLOB' --validate 'GLOB' [--test 'GLOB'] \\
        --model_args "{'regression': 'full_loss', 'folder': 'model'}" --fit_args "{'num_epochs': 200}"
    --model CGANRegression-Unet (the reference's sweep name) trains the U-Net generator; the default is CGANRegression.
"""
import os
from time import time

import numpy as np
import torch
from torch import nn

from .cnn_tools import ChannelwiseScaler
from .train_common import check_fit_args, command_line, cuda_device, print_start, stacked
from .train_CNN import FluxFormCNN, TrainableAndrewCNN, _write_folder, prepare_PV_data, train
from .train_CVAE import _forward_all
from .train_UNet import UNET_GRIDS, TrainableUNet
from .train_ops import GRIDS, data_gradient_only, gather_batch, head_apply, latent_prior, strided_conv2d

LAMBDA_DRIFT = 1e-3                                                               # cgan_regression.py:18-19
LAMBDA_GP = 10
G_EVERY = 5                                                                       # a generator step where i % 5 == 0 (:308)
KEYS = ('D_loss', 'D_grad', 'D_drift', 'G_loss')                                  # what the loop logs (:315-321)
SCORES = ('L2_mean', 'L2_total', 'L2_residual', 'var_ratio')                      # what evaluate_prediction returns (:234)
REGRESSIONS = ('None', 'full_loss', 'residual_loss')
_U64 = (1 << 64) - 1


def weights_init(m):
    """the DCGAN initialisation the reference applies to G and D (cnn_tools.py:54-65): convolution weights N(0, 0.02),
    BatchNorm weights N(1, 0.02) and biases 0; convolution biases keep torch's default"""
    if isinstance(m, nn.Conv2d):
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif isinstance(m, nn.BatchNorm2d):
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


def _seeded_init(module, seed):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        module.apply(weights_init)
    return module


class TrainableDiscriminator(nn.Sequential):
    """DCGAN_discriminator(6, ndf, nx, bn='None') (cnn_tools.py:212-244): the reference's own nn.Sequential — four
    Conv2d(cin, cout, 4, stride=2, padding=1, bias=False) with LeakyReLU(0.2), 6 -> ndf -> 2 ndf -> 4 ndf -> 8 ndf, Identity in
    the norm slots, and a Conv2d(8 ndf, 1, nx / 16) that reduces the (nx / 16)^2 image to one number — so the state dict has the
    reference's keys 0.weight, 2.weight, 5.weight, 8.weight, 11.weight, initialised by weights_init under `seed`.  The inherited
    forward is the reference's, on planar tensors through torch (what tests compare against); ``forward_engine`` evaluates the
    same function on the device kernels.  There is no norm layer, so samples are independent: batches may be concatenated."""

    STRIDED = (0, 2, 5, 8)

    def __init__(self, nx, ndf=64, seed=0):
        nx, ndf = int(nx), int(ndf)
        if nx not in GRIDS:
            raise ValueError(f'nx = {nx}: one of {GRIDS}')
        if not 1 <= ndf <= 64:
            raise ValueError(f'ndf = {ndf}: 1 ... 64 (the widest layer has 8 ndf channels, the kernels take 512)')
        with torch.random.fork_rng(devices=[]):                 # the constructors draw torch's defaults: not from the global stream
            layers = [nn.Conv2d(6, ndf, 4, 2, 1, bias=False), nn.LeakyReLU(0.2)]
            for m in (1, 2, 4):
                layers += [nn.Conv2d(ndf * m, ndf * 2 * m, 4, 2, 1, bias=False), nn.Identity(), nn.LeakyReLU(0.2)]
            layers.append(nn.Conv2d(ndf * 8, 1, nx // 16, 1, 0, bias=False))
        super().__init__(*layers)
        self.nx, self.ndf = nx, ndf
        _seeded_init(self, seed)

    def forward_engine(self, a):
        """a (B, nx, nx, 8) in the engine layout, channels [x1, x2, ya1, ya2, yb1, yb2, 0, 0] -> (B,).  LeakyReLU is written as
        y * slope(y) with the slopes (1 or 0.2) a constant of the graph: the same values and the same derivative as
        F.leaky_relu, whose double backward would hand every layer's forward node a gradient of zeros — one data-gradient and
        one weight-gradient launch per layer spent on zeros in every gradient-penalty step.  The last layer is a torch
        contraction of the (B, nx / 16, nx / 16, 8 ndf) activation with 11.weight."""
        if a.dim() != 4 or tuple(a.shape[1:]) != (self.nx, self.nx, 8):
            raise ValueError(f'input {tuple(a.shape)}: expected (B, {self.nx}, {self.nx}, 8)')
        for l in self.STRIDED:
            y = strided_conv2d(a, self[l].weight)
            with torch.no_grad():
                slope = torch.where(y > 0, 1.0, 0.2)
            a = y * slope
        return torch.einsum('bijc,cij->b', a[..., :8 * self.ndf], self[11].weight[0])


def critic_input(xe, ya, yb):
    """[x, ya, yb] of engine-layout tensors (B, N, N, >= 2 channels each, the first two taken) -> (B, N, N, 8)"""
    return torch.cat([xe[..., :2], ya[..., :2], yb[..., :2], torch.zeros_like(xe[..., :2])], dim=-1)


class TrainableCGAN(nn.Module):
    """The nets of CGANRegression(regression, nx, generator='Andrew', div=, hidden_channels=) (cgan_regression.py:50-63):

      G          AndrewCNN(4, 2, div, hidden_channels): [x, z] -> y         weights_init under seed
      D          DCGAN_discriminator(6, bn='None', nx): [x, ya, yb] -> one number (minibatch discrimination over two
                 forcings)                                                   weights_init under seed + 1
      net_mean   AndrewCNN(2, 2, div) with the default widths, with regression 'full_loss' or 'residual_loss' only; torch's
                 default initialisation under seed + 2

    The latent noise of training is the Philox stream of key `seed`, that of prediction the stream of key `seed + 1`.
    `ndf` (the reference fixes 64) exists so that tests can be small."""

    def __init__(self, regression='None', nx=64, div=False, hidden_channels=(128, 64, 32, 32, 32, 32, 32), seed=0,
                 generator='Andrew', ndf=64):
        super().__init__()
        if generator == 'DeepInversion':
            raise NotImplementedError("generator='DeepInversion': the U-Net generator is trained by TrainableUNetCGAN and "
                                      "fit_cgan_unet; this class and fit_cgan train generator='Andrew'")
        if generator != 'Andrew':
            raise ValueError(f'generator={generator!r}: not implemented')
        self._build(regression, nx, div, hidden_channels, seed, generator, ndf)

    def _build(self, regression, nx, div, hidden_channels, seed, generator, ndf):
        if regression not in REGRESSIONS:
            raise ValueError(f'regression={regression!r}: one of {REGRESSIONS}')
        self.regression, self.nx, self.div, self.seed, self.generator = regression, int(nx), bool(div), int(seed), generator
        if not 0 <= self.seed < _U64 - 1:
            raise ValueError(f'seed = {seed}: 0 ... 2^64 - 3')
        net = FluxFormCNN if self.div else TrainableAndrewCNN
        if generator == 'DeepInversion':
            if self.nx not in UNET_GRIDS:
                raise ValueError(f'nx = {nx}: the U-Net generator runs on one of {UNET_GRIDS}')
            self.G = TrainableUNet(self.seed)
            self.hidden_channels = list(hidden_channels)
        else:
            self.G = _seeded_init(net(4, 2, hidden_channels=hidden_channels, seed=self.seed), self.seed)
            self.hidden_channels = list(self.G.hidden_channels)
        self.D = TrainableDiscriminator(self.nx, ndf, self.seed + 1)
        if regression != 'None':
            self.net_mean = net(2, 2, seed=self.seed + 2)
        self.x_scale = self.y_scale = None          # fit_cgan sets them; evaluate_prediction needs them

    def critic_losses(self, xe, ye, f1, f2, eps, coin):
        """The discriminator's three losses of one batch (cgan_regression.py:297-304 and gradient_penalty, :197-222), on
        engine-layout tensors (B, N, N, 8): xe the PV, ye the target, f1 and f2 the two fakes (detached here), eps (B,) the
        interpolation weights and coin (0 or 1) which of the two `true` concatenations the penalty interpolates from.
        Dtrue1, Dtrue2 and Dfake are one batch of 3 B; the interpolate is a batch of its own, since only its input asks for
        a gradient.  -> {'D_loss', 'D_grad', 'D_drift'}, differentiable in D's weights — D_grad through the second
        derivative of the strided convolutions."""
        B = xe.shape[0]
        f1, f2 = f1.detach(), f2.detach()
        true1, true2, fake = critic_input(xe, ye, f2), critic_input(xe, f1, ye), critic_input(xe, f1, f2)
        Dtrue1, Dtrue2, Dfake = self.D.forward_engine(torch.cat([true1, true2, fake], dim=0)).split(B)
        D_loss = -0.5 * (Dtrue1.mean() + Dtrue2.mean()) + Dfake.mean()
        D_drift = LAMBDA_DRIFT * (Dtrue1 ** 2).mean()
        e = eps.reshape(B, 1, 1, 1)
        yinterp = (e * (true1 if int(coin) == 0 else true2)[..., 2:6] + (1 - e) * fake[..., 2:6]).detach().requires_grad_(True)
        Dinterp = self.D.forward_engine(torch.cat([xe[..., :2], yinterp, torch.zeros_like(xe[..., :2])], dim=-1))
        with data_gradient_only():                  # only yinterp is asked for: no weight gradient of this pass is used
            dDdy, = torch.autograd.grad(Dinterp.sum(), yinterp, create_graph=True)
        D_grad = LAMBDA_GP * torch.mean((torch.linalg.norm(dDdy.reshape(B, -1), 2, dim=1) - 1) ** 2)
        return {'D_loss': D_loss, 'D_grad': D_grad, 'D_drift': D_drift}

    def generator_loss(self, xe, f1, f2):
        """G_loss = -mean D([x, yfake1, yfake2]) (:310), differentiable in the fakes"""
        return -self.D.forward_engine(critic_input(xe, f1, f2)).mean()


class TrainableUNetCGAN(TrainableCGAN):
    """The nets of CGANRegression(regression, nx, generator='DeepInversion', div=, hidden_channels=): TrainableCGAN with
    G = TrainableUNet (tools/train_UNet.py: DeepInversionGenerator(4, 2) on ``unet_conv2d``, weights_init under seed — which in
    the reference reaches the ConvTranspose2d weights too).  nx is one of the grids the U-Net's device inference admits (32,
    48, 64, 96, 128); `div` reaches net_mean alone, as in the reference (the U-Net has no flux form); `hidden_channels` is
    recorded for model_args.json and not used.  D, net_mean, the losses and train_CGAN are TrainableCGAN's."""

    def __init__(self, regression='None', nx=64, div=False, hidden_channels=(128, 64, 32, 32, 32, 32, 32), seed=0, ndf=64):
        nn.Module.__init__(self)
        self._build(regression, nx, div, hidden_channels, seed, 'DeepInversion', ndf)


def run_epoch(batches, critic_step, generator_step, acc):
    """The order of an epoch (cgan_regression.py:283-321): for batch i, critic_step(i, batch) — the three D losses, after its
    optimizer has stepped — then, where i % 5 == 0, generator_step(i, batch) -> G_loss, against the discriminator just updated;
    on the other batches the logged G_loss keeps its last value.  Each batch adds its four losses times its size, and its
    size, to acc (5,), without a host read."""
    G_loss = None
    for i, batch in enumerate(batches):
        losses = critic_step(i, batch)
        if i % G_EVERY == 0:
            G_loss = generator_step(i, batch)
        n = len(batch)
        acc[:-1] += torch.stack([losses[k].detach().to(torch.float64) for k in KEYS[:3]] + [G_loss.detach().to(torch.float64)]) * n
        acc[-1] += n
    return acc


def draw_mixes(steps, batch_size):
    """an epoch's interpolation weights (steps, batch_size) in [0, 1) and coins (steps,) in {0, 1} from numpy's global stream"""
    return np.random.rand(steps, batch_size).astype(np.float32), np.random.randint(0, 2, steps)


def evaluate_prediction(net, ds, nruns=None, M=16, runs=None, device=0, batch_size=64):
    """evaluate_prediction (cgan_regression.py:224-234) with predict (:173-189) at M draws: nruns runs of ds chosen without
    replacement from numpy's global stream (runs(R, nruns) replaces the choice), M draws of the latent noise through the
    eval-mode G, the first sample and the mean over the M, plus net_mean with a regression, denormalized, and scored on the
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
        net.G.to(dev).eval()
        with torch.no_grad():
            for s in range(0, len(X), batch_size):
                x = X[s:s + batch_size]
                acc = None
                for m in range(int(M)):
                    net.prior_draws = getattr(net, 'prior_draws', 0) + 1
                    yhat = head_apply(net.G.forward_engine(latent_prior(x, None, net.seed + 1, net.prior_draws - 1)), 2, 'mse')
                    if m == 0:
                        first[s:s + batch_size] = yhat
                    acc = yhat if acc is None else acc + yhat
                mean[s:s + batch_size] = acc / int(M)
        net.G.train()
        if net.regression != 'None':
            corr = _forward_all(net.net_mean.to(dev), X, batch_size)
            first, mean = first + corr, mean + corr
        ystd = torch.as_tensor(np.asarray(net.y_scale.std, dtype=np.float32)).to(dev)
        st = OfflineStats(np.ascontiguousarray(y), (mean * ystd).reshape(shape), (first * ystd).reshape(shape),
                          device=torch.cuda.current_device())
    scores = _scores(st)
    return {k: np.asarray(scores[k].values, dtype=np.float64) if k == 'var_ratio' else float(np.asarray(scores[k].values)) for k in SCORES}


def train_CGAN(net, X_train, Y_train, num_epochs, batch_size, learning_rate, ds_train=None, ds_test=None, nruns=5, device=0,
               orders=None, mixes=None, runs=None, verbose=True):
    """train_CGAN (cgan_regression.py:247-344) with the data resident on the device: two Adams with betas (0.5, 0.999), two
    MultiStepLR with milestones int(E / 2), int(3 E / 4), int(7 E / 8) and gamma 0.5 stepped per epoch; per batch a
    discriminator step on error = D_loss + D_grad + D_drift and, where i % 5 == 0, a generator step after it (run_epoch).
    Y_mean = net_mean(X_train) in eval mode with a regression: 'residual_loss' subtracts it from the target, 'full_loss'
    adds it to both fakes.  G's input is latent_prior(X, idx, seed, step), the Philox step a counter of the draws made, two per
    batch; on batches without a generator step the two generator forwards run under no_grad (BatchNorm's running statistics
    update either way).  Per epoch, the shuffle comes from numpy's global stream (orders(epoch, n) replaces it), then the
    interpolation weights and coins of gradient_penalty (draw_mixes; mixes(epoch, steps, batch_size) replaces the draw); both
    are checked on the host and uploaded once.  The weighted means of the four losses are accumulated on the device and read
    once per epoch.  With ds_train and ds_test, evaluate_prediction scores nruns runs of each after every epoch.  Returns
    (optim_loss, log_train, log_test)."""
    dev = cuda_device(device)
    as_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if not torch.is_tensor(a) else a.to(dev, torch.float32)
    X, Y = as_dev(X_train), as_dev(Y_train)
    n, E, batch_size = len(X), int(num_epochs), int(batch_size)
    if X.dim() != 4 or int(X.shape[-1]) != net.nx or X.shape != Y.shape or X.shape[1] != 2:
        raise ValueError(f'X {tuple(X.shape)}, Y {tuple(Y.shape)}: expected two (n, 2, {net.nx}, {net.nx})')
    print_start(dev, n, verbose)
    net.to(dev)
    optim_loss, log_train, log_test = {k: [] for k in KEYS}, [], []
    steps = (n + batch_size - 1) // batch_size
    t_s = time()
    with torch.cuda.device(dev):
        Y_mean = _forward_all(net.net_mean, X, batch_size) if net.regression != 'None' else None
        T = Y - Y_mean if net.regression == 'residual_loss' else Y
        net.G.train()
        net.D.train()
        optimizerD = torch.optim.Adam(net.D.parameters(), lr=learning_rate, betas=(0.5, 0.999))
        optimizerG = torch.optim.Adam(net.G.parameters(), lr=learning_rate, betas=(0.5, 0.999))
        milestones = [int(E / 2), int(E * 3 / 4), int(E * 7 / 8)]
        schedulerD = torch.optim.lr_scheduler.MultiStepLR(optimizerD, milestones=milestones, gamma=0.5)
        schedulerG = torch.optim.lr_scheduler.MultiStepLR(optimizerG, milestones=milestones, gamma=0.5)
        draws = [0]
        fakes = {}

        def generate(idx):
            a = net.G.forward_engine(latent_prior(X, idx, net.seed, draws[0]))
            draws[0] += 1
            return a if net.regression != 'full_loss' else a + gather_batch(Y_mean, idx)

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
            eps, coins = draw_mixes(steps, batch_size) if mixes is None else mixes(epoch, steps, batch_size)
            eps, coins = np.asarray(eps, dtype=np.float32), np.asarray(coins, dtype=np.int64)
            if eps.shape != (steps, batch_size) or coins.shape != (steps,) or not np.isin(coins, (0, 1)).all():
                raise ValueError(f'mixes({epoch}, {steps}, {batch_size}): expected weights ({steps}, {batch_size}) and coins ({steps},) of 0 and 1')
            order, eps = torch.as_tensor(order).to(dev), torch.as_tensor(eps).to(dev)

            def critic_step(i, idx):
                xe, ye = gather_batch(X, idx), gather_batch(T, idx)
                net.D.zero_grad()
                if i % G_EVERY == 0:
                    f1, f2 = generate(idx), generate(idx)
                else:
                    with torch.no_grad():
                        f1, f2 = generate(idx), generate(idx)
                fakes['now'] = (xe, f1, f2)
                losses = net.critic_losses(xe, ye, f1, f2, eps[i, :len(idx)], coins[i])
                (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()
                optimizerD.step()
                return losses

            def generator_step(i, idx):
                net.G.zero_grad()
                G_loss = net.generator_loss(*fakes['now'])
                with data_gradient_only():          # D's weights are not stepped on this loss, and D.zero_grad() precedes their next use
                    G_loss.backward()
                optimizerG.step()
                return G_loss

            run_epoch([order[s:s + batch_size] for s in range(0, n, batch_size)], critic_step, generator_step, acc)
            fakes.clear()
            schedulerD.step()
            schedulerG.step()
            a = acc.cpu().numpy()                                                       # the epoch's one host read of the losses
            for i, k in enumerate(KEYS):
                optim_loss[k].append(float(a[i] / a[-1]))
            if ds_train is not None and ds_test is not None:
                log_train.append(evaluate_prediction(net, ds_train, nruns, runs=runs, device=dev, batch_size=batch_size))
                log_test.append(evaluate_prediction(net, ds_test, nruns, runs=runs, device=dev, batch_size=batch_size))
            if verbose:
                t = time()
                line = '[%d/%d] [%.2f/%.2f] D_loss: %.2f G_loss: %.2f' % (
                    epoch + 1, E, t - t_e, (t - t_s) * (E / (epoch + 1) - 1), optim_loss['D_loss'][-1], optim_loss['G_loss'][-1])
                if log_train:
                    a, b = log_train[-1], log_test[-1]
                    line += ' L2_mean: [%.3f,%.3f] L2_total: [%.3f,%.3f] L2_res: [%.3f,%.3f]' % (
                        a['L2_mean'], b['L2_mean'], a['L2_total'], b['L2_total'], a['L2_residual'], b['L2_residual'])
                print(line)
    return optim_loss, log_train, log_test


def loss_to_dataset(optim_loss, log_train, log_test):
    """loss_to_xarray (cgan_regression.py:236-245) -> (dataset, Epoch_opt): the four losses over `epoch` (1 ... E); L2_mean,
    L2_total, L2_residual of the training runs, and of the test runs as L2_mean_test, L2_total_test, L2_residual_test;
    loss = L2_total_test + L2_residual_test and Epoch_opt, the epoch (counted from 1) of its minimum.  As the reference builds
    it, the test log's var_ratio is NOT renamed and therefore replaces the training log's: var_ratio (epoch, lev) is that of
    the test runs."""
    from .simulate import dataset_backend
    xr = dataset_backend()
    E = len(optim_loss['D_loss'])
    if len(log_train) != E or len(log_test) != E:
        raise ValueError(f'{E} epochs of losses, {len(log_train)} and {len(log_test)} of scores')
    ds = xr.Dataset({k: (['epoch'], np.asarray(v, dtype=np.float64)) for k, v in optim_loss.items()}, coords={'epoch': np.arange(1, E + 1)})
    for k in SCORES[:3]:
        ds[k] = (['epoch'], np.array([float(e[k]) for e in log_train]))
    for k in SCORES[:3]:
        ds[k + '_test'] = (['epoch'], np.array([float(e[k]) for e in log_test]))
    ds['var_ratio'] = (['epoch', 'lev'], np.array([np.asarray(e['var_ratio'], dtype=np.float64) for e in log_test]))
    loss = np.asarray(ds['L2_total_test'].values) + np.asarray(ds['L2_residual_test'].values)
    ds['loss'] = (['epoch'], loss)
    epoch_opt = int(np.argmin(loss)) + 1
    ds['Epoch_opt'] = epoch_opt
    return ds, epoch_opt


def write_cgan_folder(folder, net, x_scale, y_scale, optim_loss, log_train, log_test, verbose=True):
    """CGANRegression.save_model (cgan_regression.py:89-107): G.pt, D.pt, net_mean.pt with a regression (CPU state dicts),
    x_scale.json, y_scale.json, model_args.json with model: 'CGANRegression' and regression, nx, generator, div,
    hidden_channels, stats.nc (loss_to_dataset).  Returns Epoch_opt; as in the reference, the LAST epoch's nets are written."""
    states = {'G.pt': net.G.state_dict(), 'D.pt': net.D.state_dict()}
    if net.regression != 'None':
        states['net_mean.pt'] = net.net_mean.state_dict()
    _write_folder(folder, states, x_scale, y_scale, dict(model='CGANRegression', regression=net.regression, nx=net.nx,
                                                         generator=net.generator, div=net.div,
                                                         hidden_channels=list(net.hidden_channels)))
    stats, epoch_opt = loss_to_dataset(optim_loss, log_train, log_test)
    path = os.path.join(folder, 'stats.nc')
    if os.path.exists(path):
        os.remove(path)
    stats.to_netcdf(path)
    if verbose:
        print('Optimal epoch is ', epoch_opt)
        print('The Last epoch is used for prediction')
    return epoch_opt


def _fit(who, net, ds_train, ds_test, regression, folder, num_epochs, num_epochs_regression, batch_size, learning_rate, nruns,
         device, orders, mixes, runs, verbose):
    """the body of fit_cgan and fit_cgan_unet (`who`, for messages) for the nets `net` (a TrainableCGAN): net_mean read or
    trained, train_CGAN, the folder, and the model read back from it"""
    from ..models.cgan_regression import CGANRegression
    num_epochs, num_epochs_regression, batch_size = int(num_epochs), int(num_epochs_regression), int(batch_size)
    if regression != 'None':
        check_fit_args(who, num_epochs_regression, batch_size, 0.001)
    X_train, Y_train, X_test, Y_test, net.x_scale, net.y_scale = prepare_PV_data(ds_train, ds_test, who)
    if X_train.shape[-1] != net.nx:
        raise ValueError(f'{who}: the datasets are on a {X_train.shape[-1]} x {X_train.shape[-1]} grid, nx = {net.nx}')
    dev = cuda_device(device)
    X_train, Y_train, X_test, Y_test = (torch.as_tensor(a).to(dev) for a in (X_train, Y_train, X_test, Y_test))
    if regression != 'None':
        if os.path.exists(os.path.join(folder, 'net_mean.pt')):
            for name, have in (('x_scale.json', net.x_scale), ('y_scale.json', net.y_scale)):
                old = ChannelwiseScaler().read(name, folder)
                if not (np.array_equal(old.std.reshape(-1), have.std.reshape(-1)) and np.array_equal(old.mean.reshape(-1), have.mean.reshape(-1))):
                    raise ValueError(f'{who}: {os.path.join(folder, name)} is not the scale of ds_train: net_mean.pt of this '
                                     'folder was trained on other data')
            if verbose:
                print('Net mean is loaded instead of training')
            net.net_mean.load_state_dict(torch.load(os.path.join(folder, 'net_mean.pt'), map_location='cpu', weights_only=True))
            net.net_mean.to(dev)
            net.mean_loaded = True
        else:
            train(net.net_mean, X_train, Y_train, X_test, Y_test, num_epochs_regression, batch_size, 0.001, device=dev, orders=orders,
                  verbose=verbose)
            net.mean_loaded = False
    logs = train_CGAN(net, X_train, Y_train, num_epochs, batch_size, learning_rate, ds_train=ds_train, ds_test=ds_test, nruns=nruns,
                      device=dev, orders=orders, mixes=mixes, runs=runs, verbose=verbose)
    write_cgan_folder(folder, net, net.x_scale, net.y_scale, *logs, verbose=verbose)
    model = CGANRegression(regression=regression, nx=net.nx, generator=net.generator, folder=folder, div=net.div,
                           hidden_channels=list(net.hidden_channels), device=device)
    model.trained_G, model.trained_D, model.trained = net.G, net.D, net
    if regression != 'None':
        model.trained_net_mean = net.net_mean
    return model


def fit_cgan(ds_train, ds_test, *, regression='None', nx=64, generator='Andrew', div=False,
             hidden_channels=[128, 64, 32, 32, 32, 32, 32], folder='model', num_epochs=200, num_epochs_regression=50, batch_size=64,
             learning_rate=2e-4, nruns=5, seed=0, device=0, orders=None, mixes=None, runs=None, verbose=True, ndf=64):
    """CGANRegression(regression, nx, generator, folder, div, hidden_channels).fit(ds_train, ds_test, num_epochs,
    num_epochs_regression, batch_size, learning_rate, nruns) on the device (cgan_regression.py:68-107), then save_model;
    returns CGANRegression(folder=folder) read back from the files, with the trained nets attached as trained_G, trained_D and
    (with a regression) trained_net_mean.

    With a regression, net_mean is read from `folder` if net_mean.pt is there — the folder's scales must then equal those of
    ds_train bit for bit — and is otherwise trained with MSE for num_epochs_regression epochs at learning rate 0.001, as the
    reference does.  G and D are initialised by weights_init under seed and seed + 1, net_mean by torch's defaults under
    seed + 2; the epochs' shuffles, interpolation weights and coins and the choice of the nruns scored runs come from numpy's
    global stream unless orders(epoch, n), mixes(epoch, steps, batch_size) and runs(R, nruns) give them."""
    check_fit_args('fit_cgan', int(num_epochs), int(batch_size), learning_rate)
    net = TrainableCGAN(regression, nx, div, hidden_channels, seed, generator=generator, ndf=ndf)
    return _fit('fit_cgan', net, ds_train, ds_test, regression, folder, num_epochs, num_epochs_regression, batch_size, learning_rate,
                nruns, device, orders, mixes, runs, verbose)


def fit_cgan_unet(ds_train, ds_test, *, regression='None', nx=64, div=False, hidden_channels=[128, 64, 32, 32, 32, 32, 32],
                  folder='model', num_epochs=200, num_epochs_regression=50, batch_size=64, learning_rate=2e-4, nruns=5, seed=0,
                  device=0, orders=None, mixes=None, runs=None, verbose=True, ndf=64):
    """fit_cgan for CGANRegression(generator='DeepInversion'): the same loop (train_CGAN), the same folder with generator:
    'DeepInversion' in model_args.json, and CGANRegression(generator='DeepInversion', folder=folder) read back from the files,
    with the trained nets attached as fit_cgan attaches them.  The generator is TrainableUNet: its convolutions, their data
    and weight gradients are the kernels of csrc/uconv_train.hip; BatchNorm, LeakyReLU, pooling and Adam are torch's.  nx is
    32, 48, 64, 96 or 128; div reaches net_mean alone; hidden_channels is recorded and not used."""
    check_fit_args('fit_cgan_unet', int(num_epochs), int(batch_size), learning_rate)
    net = TrainableUNetCGAN(regression, nx, div, hidden_channels, seed, ndf=ndf)
    return _fit('fit_cgan_unet', net, ds_train, ds_test, regression, folder, num_epochs, num_epochs_regression, batch_size,
                learning_rate, nruns, device, orders, mixes, runs, verbose)


def main(argv=None):
    return command_line('train CGANRegression on the device and write its model folder',
                        {'CGANRegression': fit_cgan, 'CGANRegression-Unet': fit_cgan_unet}, argv)


if __name__ == '__main__':
    main()
