"""GPU: training of CGANRegression on the device (tools/train_CGAN.py over csrc/dconv_train.hip, csrc/conv_train.hip,
csrc/latent_train.hip, csrc/train_head.hip and csrc/fluxdiv_train.hip) against the reference's statement restated on torch CPU
modules (tests/cgan_restatement.py).

The yardstick is the project's: the float32 torch CPU evaluation of the SAME statement from the same state dicts.  The device
may deviate from the float64 evaluation by at most MARGIN = 8 times what that evaluation deviates, per tensor, relative to its
largest magnitude, with a floor of 2^-22 so that an unusually lucky CPU evaluation does not fail a correct kernel.
Shape: 16 x 16, ndf = 4, a generator of hidden_channels [5, 3], batch 3.

Measured on an MI355X (device, float32 torch CPU; relative to the tensor's largest magnitude): see DESIGN.md 3.23."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import cgan_restatement as gr

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 8.0, 2.0 ** -22
HIDDEN, N, B, NDF = [5, 3], 16, 3, 4
KINK = 64 * 2.0 ** -24                      # no LeakyReLU input nearer to zero than this, relative to its layer's largest


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _engine(a):
    return torch.as_tensor(cr.to_layout(np.asarray(a, np.float32))).to(_dev())


def _compare(got, r64, r32, what):
    failures = []
    assert list(got) == list(r64) == list(r32)
    print(f'\n  {what}')
    for k in r64:
        assert np.shape(got[k]) == np.shape(r64[k]), k
        dev, cpu = _rel(got[k], r64[k]), _rel(r32[k], r64[k])
        print(f'  {k:28s} device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu if cpu else float("inf"):.2f}')
        if not dev <= max(MARGIN * cpu, FLOOR):
            failures.append((k, dev, cpu))
    assert not failures, failures


def _critic_case(seed):
    rs = np.random.RandomState(seed)
    x, y, f1, f2 = (rs.randn(B, 2, N, N).astype(np.float32) for _ in range(4))
    return x, y, f1, f2, rs.rand(B).astype(np.float32)


@pytest.mark.parametrize('coin', [0, 1])
def test_second_derivative_through_the_discriminator(coin):
    """D_loss, D_drift, D_grad, and the gradients of D_grad ALONE and of error = D_loss + D_grad + D_drift with respect to
    every weight of D, with the fakes, the interpolation weights and the coin given.  The gradient of D_grad with respect to
    0.weight is nonzero: a once-differentiable convolution has no graph to give it."""
    from pyqg_generative_amd.tools.train_CGAN import TrainableCGAN
    from pyqg_generative_amd.tools import train_ops as T
    net = TrainableCGAN('None', N, False, HIDDEN, seed=31, ndf=NDF)
    sd = {k: v.clone() for k, v in net.D.state_dict().items()}
    x, y, f1, f2, eps = _critic_case(50 + coin)

    def collect(losses, params):
        names = list(sd)
        out = {k: np.array([float(losses[k].detach())]) for k in ('D_loss', 'D_drift', 'D_grad')}
        gp = torch.autograd.grad(losses['D_grad'], params, retain_graph=True)
        err = torch.autograd.grad(losses['D_loss'] + losses['D_grad'] + losses['D_drift'], params)
        for name, g in zip(names, gp):
            out[f'dD_grad/d{name}'] = g.detach().cpu().numpy().astype(np.float64)
        for name, g in zip(names, err):
            out[f'derror/d{name}'] = g.detach().cpu().numpy().astype(np.float64)
        return out

    def on_cpu(dtype):
        D = gr.torch_discriminator(N, NDF, dtype, sd)
        t = lambda a: torch.tensor(a, dtype=dtype)
        return D, collect(gr.critic_losses(D, t(x), t(y), t(f1), t(f2), t(eps), coin), list(D.parameters()))
    (D64, r64), (_, r32) = on_cpu(torch.float64), on_cpu(torch.float32)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    e = t64(eps).reshape(B, 1, 1, 1)
    true_cat = torch.cat([t64(y), t64(f2)], 1) if coin == 0 else torch.cat([t64(f1), t64(y)], 1)
    evaluations = [torch.cat([t64(x), t64(y), t64(f2)], 1), torch.cat([t64(x), t64(f1), t64(y)], 1), torch.cat([t64(x), t64(f1), t64(f2)], 1),
                   torch.cat([t64(x), e * true_cat + (1 - e) * torch.cat([t64(f1), t64(f2)], 1)], 1)]
    nearest = gr.leaky_inputs_nearest_to_zero(D64, evaluations)
    print(f'\n  the LeakyReLU input nearest to zero, relative to its layer: {nearest:.2e} (at least {KINK:.2e})')
    assert nearest >= KINK

    net.to(_dev()).train()
    before = dict(T.DCONV_LAUNCHES)
    losses = net.critic_losses(_engine(x), _engine(y), _engine(f1), _engine(f2), torch.tensor(eps).to(_dev()), coin)
    got = collect(losses, list(net.D.parameters()))
    print('  launches of the losses and two gradient calls:', {k: T.DCONV_LAUNCHES[k] - before[k] for k in before})
    assert np.abs(got['dD_grad/d0.weight']).max() > 0 and np.abs(r64['dD_grad/d0.weight']).max() > 0
    _compare(got, r64, r32, f'critic losses and their gradients, coin {coin}')


def test_launch_counts_of_one_discriminator_step_and_one_generator_step():
    """per strided layer (four of them).  The losses: one forward of the 3 B batch, one of the interpolate, and the
    interpolate's data gradient (its weight gradient is not asked for: data_gradient_only).  error.backward(): the 3 B batch's
    weight gradient and, but for the first layer, whose input asks for none, its data gradient; and the derivative of the
    interpolate's data gradient — a forward (with respect to dy) and a weight gradient (with respect to w).
    A generator step: a forward and a data gradient, no weight gradient."""
    from pyqg_generative_amd.tools.train_CGAN import TrainableCGAN
    from pyqg_generative_amd.tools import train_ops as T
    net = TrainableCGAN('None', N, False, HIDDEN, seed=32, ndf=NDF).to(_dev()).train()
    x, y, f1, f2, eps = _critic_case(60)
    count = lambda before: [T.DCONV_LAUNCHES[k] - before[k] for k in ('forward', 'backward_data', 'backward_weight')]
    before = dict(T.DCONV_LAUNCHES)
    losses = net.critic_losses(_engine(x), _engine(y), _engine(f1), _engine(f2), torch.tensor(eps).to(_dev()), 0)
    assert count(before) == [8, 4, 0]
    (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()
    assert count(before) == [12, 7, 8]
    assert all(p.grad is not None and bool(p.grad.abs().max() > 0) for p in net.D.parameters())
    before = dict(T.DCONV_LAUNCHES)
    fakes = [_engine(f).requires_grad_(True) for f in (f1, f2)]
    with T.data_gradient_only():
        net.generator_loss(_engine(x), *fakes).backward()
    assert count(before) == [4, 4, 0]
    assert all(bool(f.grad[..., :2].abs().max() > 0) and not bool(f.grad[..., 2:].any()) for f in fakes)


def _noise_of(net, X, orders, E, batch):
    """the latent noise train_CGAN will draw, read back from latent_prior at the same (seed, step): two steps per batch"""
    from pyqg_generative_amd.tools.train_ops import latent_prior
    Xd = torch.as_tensor(X).to(_dev())
    out, step = [], 0
    for epoch in range(E):
        order = torch.as_tensor(np.asarray(orders(epoch, len(X)), dtype=np.int64)).to(_dev())
        for s in range(0, len(X), batch):
            for _ in range(2):
                a = latent_prior(Xd, order[s:s + batch], net.seed, step)
                assert torch.equal(a[..., :2], Xd[order[s:s + batch]].permute(0, 2, 3, 1))
                out.append(a[..., 2:4].permute(0, 3, 1, 2).cpu().numpy())
                step += 1
    return out


@pytest.mark.parametrize('regression', ['None', 'full_loss'])
def test_trajectory_of_ten_steps_through_train_CGAN(regression):
    """train_CGAN's loop: 15 samples in batches of 3 over 2 epochs — ten discriminator steps, two generator steps (batch 0 of
    each epoch), the schedule's decay between them — against the same loop in float32 torch on the CPU from the same initial
    state, orders, mixes and latent noise.  The deviation of the parameters' displacement from the float64 loop's is measured
    against the float32 CPU loop's own."""
    from pyqg_generative_amd.tools.train_CGAN import TrainableCGAN, train_CGAN
    from pyqg_generative_amd.tools import train_ops as T
    net = TrainableCGAN(regression, N, False, HIDDEN, seed=33, ndf=NDF)
    states = {name: {k: v.clone() for k, v in getattr(net, name).state_dict().items()} for name in ('G', 'D')}
    rs = np.random.RandomState(70)
    n, E, rate = 15, 2, 2e-3
    X, Y = rs.randn(n, 2, N, N).astype(np.float32), rs.randn(n, 2, N, N).astype(np.float32)
    orders = cr.fixed_orders(80)
    mix = {e: (np.random.RandomState(90 + e).rand(5, B).astype(np.float32), np.random.RandomState(95 + e).randint(0, 2, 5)) for e in range(E)}
    mixes = lambda epoch, steps, batch: mix[epoch]
    assert {int(c) for e in mix for c in mix[e][1]} == {0, 1}
    noise = _noise_of(net, X, orders, E, B)
    assert len(noise) == 20

    def displacement(G, D):
        parts = []
        for name, m in (('G', G), ('D', D)):
            sd = m.state_dict()
            parts += [(sd[k].detach().cpu().to(torch.float64) - states[name][k].to(torch.float64)).reshape(-1).numpy()
                      for k in states[name] if k.endswith(('.weight', '.bias'))]
        return np.concatenate(parts)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        G, D = gr.generator(HIDDEN, dtype, states['G']), gr.torch_discriminator(N, NDF, dtype, states['D'])
        Y_mean = None
        if regression != 'None':
            mean = cr.torch_net(2, 2, [128, 64, 32, 32, 32, 32, 32], True, True, dtype, net.net_mean.state_dict()).eval()
            with torch.no_grad():
                Y_mean = mean(torch.as_tensor(X).to(dtype))
        log = gr.reference_loop(G, D, X, Y, Y_mean, regression, E, B, rate, orders, mixes, lambda step: noise[step])
        ref[dtype] = (displacement(G, D), log)
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    before = dict(T.DCONV_LAUNCHES)
    optim_loss, log_train, log_test = train_CGAN(net, X, Y, E, B, rate, device=0, orders=orders, mixes=mixes, verbose=False)
    # ten discriminator steps and two generator steps, per strided layer
    assert [T.DCONV_LAUNCHES[k] - before[k] for k in ('forward', 'backward_data', 'backward_weight')] == [10 * 12 + 2 * 4, 10 * 7 + 2 * 4, 10 * 8]
    assert log_train == [] and log_test == [] and tuple(optim_loss) == gr.KEYS
    assert int(net.G.state_dict()['conv.2.num_batches_tracked']) == 20           # two forwards per batch, with or without a graph
    dd = displacement(net.G, net.D)
    dev, cpu = _rel(dd, d64), _rel(d32, d64)
    print(f'\n  {regression}: displacement after ten steps: device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu:.2f}')
    assert np.abs(d64).max() > 1e-3                                               # the parameters moved
    assert dev <= max(MARGIN * cpu, FLOOR)
    log64, log32 = ref[torch.float64][1], ref[torch.float32][1]
    for k in gr.KEYS:
        got, l64, l32 = (np.asarray(v, np.float64) for v in (optim_loss[k], log64[k], log32[k]))
        assert got.shape == (E,)
        d, r = np.abs(got - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
        print(f'  {k:10s} worst over epochs: device {d.max():.2e}   float32 torch CPU {r.max():.2e}')
        assert (d <= np.maximum(MARGIN * r, 1e-5)).all(), (k, d.tolist(), r.tolist())
    # hooks the kernels could not check are refused on the host
    with pytest.raises(ValueError, match='orders'):
        train_CGAN(net, X, Y, 1, B, rate, device=0, orders=lambda epoch, n: np.arange(1, n + 1), mixes=mixes, verbose=False)
    with pytest.raises(ValueError, match='mixes'):
        train_CGAN(net, X, Y, 1, B, rate, device=0, orders=orders, mixes=lambda e, s, b: (np.zeros((s, b)), np.full(s, 2)), verbose=False)


FILES = ['D.pt', 'G.pt', 'model_args.json', 'stats.nc', 'x_scale.json', 'y_scale.json']


@pytest.mark.parametrize('regression,div', [('None', False), ('full_loss', True)], ids=['plain', 'full_loss-div'])
def test_fit_cgan_end_to_end(tmp_path, regression, div):
    """fit_cgan on conv_train_restatement.fit_dataset's 2 runs x 6 times at 16 x 16: hidden_channels [8], ndf 4, batch 4, two
    epochs, fixed orders and mixes, one scored run per epoch chosen by the hook.  No convergence threshold: a GAN's losses are
    not monotone, and none can be derived here."""
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.train_CGAN import fit_cgan
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation, dataset_backend
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    f = cr.FIT
    E, hidden = 2, f['hidden_channels']
    ds_train, ds_test = cr.fit_dataset(1), cr.fit_dataset(2)
    folder = str(tmp_path / 'model')
    mixes = lambda epoch, steps, batch: (np.random.RandomState(7 + epoch).rand(steps, batch).astype(np.float32),
                                         np.random.RandomState(9 + epoch).randint(0, 2, steps))
    fit = dict(regression=regression, nx=f['N'], div=div, hidden_channels=hidden, folder=folder, num_epochs=E, num_epochs_regression=1,
               batch_size=f['batch_size'], learning_rate=2e-3, nruns=1, seed=f['seed'], orders=cr.fixed_orders(50), mixes=mixes,
               runs=lambda R, k: np.arange(R)[::-1][:k], verbose=False, ndf=NDF)
    state = np.random.get_state()
    model = fit_cgan(ds_train, ds_test, **fit)
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))       # every draw came from a hook
    assert isinstance(model, CGANRegression)
    assert sorted(os.listdir(folder)) == sorted(FILES + (['net_mean.pt'] if regression != 'None' else []))
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='CGANRegression', regression=regression, nx=f['N'],
                                                                            generator='Andrew', div=div, hidden_channels=hidden)
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, CGANRegression) and loaded.hidden_channels == hidden and loaded.div == div

    # predict with fixed noise = the trained G's eval-mode forward on the same latent draw
    qt = np.asarray(ds_test['q'].values).reshape(-1, 2, f['N'], f['N'])
    X = (qt / loaded.x_scale.std).astype('float32')
    z = np.random.RandomState(8).randn(*X.shape).astype('float32')
    G = model.trained_G.eval()
    with torch.no_grad():
        want = G(torch.tensor(np.concatenate([X, z], 1)).to(_dev())).cpu().numpy().astype(np.float64)
        got = loaded.generate(torch.tensor(X).to(_dev()), torch.tensor(z).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
        if regression != 'None':
            mean = model.trained_net_mean.eval()
            corr = mean(torch.tensor(X).to(_dev())).cpu().numpy().astype(np.float64)
            mean.train()
    G.train()
    want = want * loaded.y_scale.std
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    if regression != 'None':
        want = want + corr * loaded.y_scale.std
    snap = loaded.predict_snapshot(type('M', (), {'q': qt[3].astype(np.float64)})(), z[3:4])
    assert np.abs(snap - want[3]).max() <= 2e-5 * np.abs(want).max()

    # the log: every variable, finite, Epoch_opt in 1 ... E
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    val = lambda k: np.asarray(stats[k].values)
    for k in list(gr.KEYS) + ['L2_mean', 'L2_total', 'L2_residual', 'L2_mean_test', 'L2_total_test', 'L2_residual_test', 'loss']:
        assert val(k).shape == (E,) and np.isfinite(val(k)).all(), k
    assert val('var_ratio').shape == (E, 2) and np.isfinite(val('var_ratio')).all()
    assert 1 <= int(val('Epoch_opt')) <= E and int(val('Epoch_opt')) == int(np.argmin(val('loss'))) + 1
    print(f"\n  D_loss {val('D_loss')}, D_grad {val('D_grad')}, G_loss {val('G_loss')}, loss {val('loss')}")

    # online: one parameterized step
    Ns = 32
    q0 = np.random.RandomState(4).randn(2, Ns, Ns) * np.array([8e-6, 1e-6]).reshape(2, 1, 1)
    params = EDDY_PARAMS.nx(Ns)._update({'tmax': 14400., 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=loaded, sampling='constant', nsteps=1), q_init=q0, sampling_freq=14400.)
    qq = np.asarray(out['q'].values)
    assert qq.shape[-3:] == (2, Ns, Ns) and np.isfinite(qq).all() and np.abs(qq[-1] - q0).max() > 0

    # a second fit into the folder, which now holds net_mean.pt, loads it instead of training it
    if regression != 'None':
        first = {k: v.detach().cpu().clone() for k, v in model.trained_net_mean.state_dict().items()}
        assert model.trained.mean_loaded is False and len(model.trained_net_mean.log_dict['loss']) == 1
        again = fit_cgan(ds_train, ds_test, **dict(fit, num_epochs=1))
        assert again.trained.mean_loaded is True and not again.trained_net_mean.log_dict
        assert all(torch.equal(first[k], v.detach().cpu()) for k, v in again.trained_net_mean.state_dict().items())


def test_command_line_trains_a_folder(tmp_path):
    """python -m pyqg_generative_amd.tools.train_CGAN, in process: one file per run, one epoch with regression='residual_loss'
    and the shuffles, mixes and scored runs of numpy's global stream (put back afterwards)"""
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools import train_CGAN, xr_lite
    from pyqg_generative_amd.tools.simulate import load_parameterization
    dims = ['run', 'time', 'lev', 'y', 'x']
    for name, seed in (('train', 1), ('val', 2)):
        q, y = cr.fit_fields(seed)
        for r in range(len(q)):
            xr_lite.Dataset({'q': (dims, q[r:r + 1]), 'q_forcing_advection': (dims, y[r:r + 1])},
                            coords={'time': (('time',), np.arange(q.shape[1], dtype='float32') * 1000.)}).to_netcdf(str(tmp_path / f'{name}_{r}.nc'))
    folder = str(tmp_path / 'model')
    state = np.random.get_state()
    try:
        model = train_CGAN.main(['--train', str(tmp_path / 'train_*.nc'), '--validate', str(tmp_path / 'val_*.nc'),
                                 '--model_args', repr({'hidden_channels': [8], 'folder': folder, 'regression': 'residual_loss', 'nx': 16}),
                                 '--fit_args', repr({'num_epochs': 1, 'num_epochs_regression': 1, 'batch_size': 4, 'nruns': 1,
                                                     'verbose': False, 'ndf': NDF})])
    finally:
        np.random.set_state(state)
    assert isinstance(model, CGANRegression) and isinstance(load_parameterization(folder).param, CGANRegression)
    assert sorted(os.listdir(folder)) == sorted(FILES + ['net_mean.pt'])
    assert json.load(open(os.path.join(folder, 'model_args.json')))['regression'] == 'residual_loss'
    assert len(model.trained_net_mean.log_dict['loss']) == 1
