"""GPU: training of flux-form nets, AndrewCNN(div=True), on the device (tools/train_CNN.py: FluxFormCNN, train, fit_ols(div=True)
over csrc/conv_train.hip and csrc/fluxdiv_train.hip) against the reference's div=True net restated on torch CPU modules in float64
(tests/flux_train_restatement.py::flux_torch_net).

As in tests/test_gpu_cnn_training.py the yardstick is the float32 torch CPU evaluation of the SAME state dict: the device may
deviate from float64 by at most MARGIN = 8 times what that evaluation deviates (per tensor, relative to its largest magnitude) —
a sequential fmaf chain against the library's 16-lane blocked sums is expected to differ by up to sqrt(16) = 4 x, with 2 x
headroom on top.  Two gradients of a flux-form net are zero in exact arithmetic, the last convolution's bias and the bias of
the BatchNorm in front of it (a constant flux has no divergence): there every evaluation is rounding noise around a float64
value that is itself rounding noise, and the printed relative deviations are large numbers on both sides."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import flux_train_restatement as fr

pytestmark = pytest.mark.gpu

MARGIN = 8.0
HIDDEN, N, B = [5, 3], 16, 4


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _batch(seed, n=B):
    """inputs, and targets as a flux-form net can produce them: every plane has zero mean"""
    rs = np.random.RandomState(seed)
    x, y = rs.randn(n, 2, N, N), rs.randn(n, 2, N, N)
    return x.astype(np.float32), (y - y.mean(axis=(-2, -1), keepdims=True)).astype(np.float32)


def _one_step(net, x, y):
    """train-mode forward, loss, backward -> {name: array}: the loss, every parameter's gradient, the running statistics"""
    net.train()
    net.zero_grad()
    loss = net.compute_loss(x, y)['loss']
    loss.backward()
    out = {'loss': np.array([float(loss.detach())])}
    for k, p in net.named_parameters():
        out['grad ' + k] = p.grad.detach().cpu().numpy().astype(np.float64)
    for k, v in net.state_dict().items():
        if 'running' in k:
            out[k] = v.detach().cpu().numpy().astype(np.float64)
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1
    return out


@pytest.mark.parametrize('batch_norm', [True, False], ids=['bn', 'nobn'])
def test_whole_net_loss_gradients_and_running_statistics(batch_norm):
    from pyqg_generative_amd.tools.train_CNN import FluxFormCNN
    from pyqg_generative_amd.tools.train_ops import FLUX_LAUNCHES
    net = FluxFormCNN(2, 2, HIDDEN, batch_norm=batch_norm, bias=True, seed=21)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, y = _batch(31)
    r64 = _one_step(fr.flux_torch_net(2, HIDDEN, batch_norm, True, torch.float64, sd), torch.tensor(x, dtype=torch.float64),
                    torch.tensor(y, dtype=torch.float64))
    r32 = _one_step(fr.flux_torch_net(2, HIDDEN, batch_norm, True, torch.float32, sd), torch.tensor(x), torch.tensor(y))
    net.to(_dev())
    before = dict(FLUX_LAUNCHES)
    got = _one_step(net, torch.tensor(x).to(_dev()), torch.tensor(y).to(_dev()))
    assert [FLUX_LAUNCHES[k] - before[k] for k in ('forward', 'backward')] == [1, 1]
    assert list(got) == list(r64) and len(got) == 1 + 6 + (4 if batch_norm else 0) + (4 if batch_norm else 0)
    assert got['grad conv.6.weight' if batch_norm else 'grad conv.4.weight'].shape == (4, 3, 3, 3)
    print()
    worst = {}
    for k in r64:
        assert got[k].shape == r64[k].shape
        dev, cpu = _rel(got[k], r64[k]), _rel(r32[k], r64[k])
        worst[k] = (dev, cpu)
        print(f'  {k:28s} device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu if cpu else float("inf"):.2f}')
    for k, (dev, cpu) in worst.items():
        assert dev <= MARGIN * cpu, (k, dev, cpu)
    # the output has zero mean by construction, in train and in eval mode
    net.eval()
    with torch.no_grad():
        out = net(torch.tensor(x).to(_dev())).cpu().numpy().astype(np.float64)
    assert out.shape == (B, 2, N, N) and np.abs(out.mean(axis=(-2, -1))).max() < 1e-6 * np.abs(out).max()


def test_trajectory_of_ten_adam_steps():
    """train()'s loop itself: 8 samples in batches of 4 over 5 epochs (ten steps, the schedule's three decays included), the
    batch order fixed; the deviation is that of the parameters' displacement from the float64 torch loop"""
    from pyqg_generative_amd.tools.train_CNN import FluxFormCNN, train
    from pyqg_generative_amd.tools.train_ops import FLUX_LAUNCHES
    net = FluxFormCNN(2, 2, HIDDEN, batch_norm=True, bias=True, seed=22)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, y = _batch(32, 8)
    xt, yt = _batch(33, 4)
    orders = cr.fixed_orders(70)
    E, lr = 5, 1e-3

    def displacement(after):
        return np.concatenate([(after[k].detach().cpu().to(torch.float64) - sd[k].to(torch.float64)).reshape(-1).numpy()
                               for k in sd if k.endswith(('.weight', '.bias'))])        # the parameters, not the buffers
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = fr.flux_torch_net(2, HIDDEN, True, True, dtype, sd)
        log = cr.reference_loop(m, x, y, xt, yt, E, 4, lr, orders)
        ref[dtype] = (displacement(m.state_dict()), log)
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    before = dict(FLUX_LAUNCHES)
    train(net, x, y, xt, yt, E, 4, lr, device=0, orders=orders, verbose=False)
    assert [FLUX_LAUNCHES[k] - before[k] for k in ('forward', 'backward')] == [15, 10]      # ten training, five test batches
    assert int(net.state_dict()['conv.2.num_batches_tracked']) == 10
    dd = displacement(net.state_dict())
    dev, cpu = _rel(dd, d64), _rel(d32, d64)
    print(f'\n  displacement after ten steps: device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu:.2f}')
    assert np.abs(d64).max() > 1e-3                    # the parameters moved
    assert dev <= MARGIN * cpu
    log64 = ref[torch.float64][1]
    assert len(net.log_dict['loss']) == E and len(net.log_dict['loss_test']) == E
    np.testing.assert_allclose(net.log_dict['loss'], log64['loss'], rtol=1e-4)
    np.testing.assert_allclose(net.log_dict['loss_test'], log64['loss_test'], rtol=1e-4)


def test_fit_ols_div_end_to_end(tmp_path):
    """fit_ols(div=True) on conv_train_restatement.fit_dataset's fields (2 runs x 6 times at 16 x 16; the target, a zero-sum
    stencil of q, has zero mean, as a flux-form net's output must), hidden_channels [5, 3], batch 4, learning rate 0.01, 8 epochs,
    fixed orders: the folder, the loaders, predict against the trained net, conservation, one online step, and the losses.

    The loss criterion is that of test_gpu_meanvar_training.py: every epoch's loss and loss_test must agree with the float64 CPU
    fit of the restated net from the same seeded state dict within 8 x the float32 CPU fit's own deviation at that epoch, floored
    at 1e-5 relative.  That float64 fit brings loss_test from 0.9533 to 0.4900 on this data, a factor 0.514 (asserted below to
    fall; the float32 CPU fit deviates from it by 1.1e-7 at the most, so the floor is what binds)."""
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.tools.train_CNN import fit_ols, FluxFormCNN, prepare_PV_data
    from pyqg_generative_amd.tools.train_ops import FLUX_LAUNCHES
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation, dataset_backend
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    f = cr.FIT
    E, seed = 8, f['seed']
    ds_train, ds_test = cr.fit_dataset(1), cr.fit_dataset(2)
    orders = cr.fixed_orders(50)
    folder = str(tmp_path / 'model')
    before = dict(FLUX_LAUNCHES)
    model = fit_ols(ds_train, ds_test, div=True, hidden_channels=HIDDEN, folder=folder, num_epochs=E, batch_size=f['batch_size'],
                    learning_rate=f['learning_rate'], seed=seed, orders=orders, verbose=False)
    n = f['runs'] * f['times']
    batches = -(-n // f['batch_size'])
    assert [FLUX_LAUNCHES[k] - before[k] for k in ('forward', 'backward')] == [2 * E * batches, E * batches]
    assert isinstance(model, OLSModel) and model.div is True and isinstance(model.trained_net, FluxFormCNN)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'stats.nc', 'x_scale.json', 'y_scale.json']
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(
        model='OLSModel', div=True, batch_norm=True, bias=True, final_activation='None', hidden_channels=HIDDEN)
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, OLSModel) and loaded.div is True and loaded.hidden_channels == HIDDEN
    q, y = cr.fit_fields(1)
    np.testing.assert_array_equal(loaded.x_scale.std.reshape(-1), q.std(axis=(0, 1, 3, 4)).astype('float32'))
    np.testing.assert_array_equal(loaded.y_scale.std.reshape(-1), y.std(axis=(0, 1, 3, 4)).astype('float32'))
    # predict = the trained net's eval-mode forward, to the generic engine's tolerance; the forcing conserves PV
    net = model.trained_net
    net.eval()
    qt = cr.fit_fields(2)[0]
    X = (qt.reshape(-1, 2, f['N'], f['N']) / loaded.x_scale.std).astype('float32')
    with torch.no_grad():
        want = net(torch.tensor(X).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
    got = np.asarray(loaded.predict(ds_test)['q_forcing_advection'].values).reshape(want.shape)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    assert np.abs(got.mean(axis=(-2, -1))).max() < 1e-6 * np.abs(got).max()

    # the log against the float64 CPU fit of the restated net from the same seeded state dict
    sd = FluxFormCNN(2, 2, HIDDEN, seed=seed).state_dict()
    data = prepare_PV_data(ds_train, ds_test)[:4]
    cpu = {dtype: cr.reference_loop(fr.flux_torch_net(2, HIDDEN, True, True, dtype, sd), *data, E, f['batch_size'],
                                    f['learning_rate'], orders) for dtype in (torch.float64, torch.float32)}
    lt = cpu[torch.float64]['loss_test']
    print(f'\n  float64 CPU fit, loss_test: first {lt[0]:.4f}, last {lt[-1]:.4f}, factor {lt[-1] / lt[0]:.3f}')
    assert lt[-1] < lt[0]
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    failures = []
    for key in ('loss', 'loss_test'):
        have = np.asarray(stats[key].values)
        assert have.shape == (E,) and np.array_equal(have, net.log_dict[key]) and np.isfinite(have).all()
        l64, l32 = np.asarray(cpu[torch.float64][key]), np.asarray(cpu[torch.float32][key])
        dev, ref = np.abs(have - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
        print(f'  {key:9s} worst over epochs: device {dev.max():.2e}   float32 torch CPU {ref.max():.2e}   '
              f'worst device / max(8 x CPU, 1e-5) {np.max(dev / np.maximum(MARGIN * ref, 1e-5)):.2f}')
        if not (dev <= np.maximum(MARGIN * ref, 1e-5)).all():
            failures.append((key, dev.tolist(), ref.tolist()))
    assert not failures, failures

    # online: one parameterized step
    Ns = 32
    q0 = np.random.RandomState(4).randn(2, Ns, Ns) * np.array([8e-6, 1e-6]).reshape(2, 1, 1)
    params = EDDY_PARAMS.nx(Ns)._update({'tmax': 14400., 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=loaded, sampling='constant', nsteps=1), q_init=q0, sampling_freq=14400.)
    qq = np.asarray(out['q'].values)
    assert qq.shape[-3:] == (2, Ns, Ns) and np.isfinite(qq).all() and np.abs(qq[-1] - q0).max() > 0


def test_command_line_trains_a_flux_form_folder(tmp_path):
    """python -m pyqg_generative_amd.tools.train_CNN with --model_args {'div': True}, in process: one netCDF file per run, two
    epochs with the shuffles of numpy's global stream (put back afterwards)"""
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.tools import train_CNN, xr_lite
    from pyqg_generative_amd.tools.simulate import load_parameterization
    dims = ['run', 'time', 'lev', 'y', 'x']
    for name, seed in (('train', 1), ('val', 2)):
        q, y = cr.fit_fields(seed)
        for r in range(len(q)):
            xr_lite.Dataset({'q': (dims, q[r:r + 1]), 'q_forcing_advection': (dims, y[r:r + 1])}).to_netcdf(str(tmp_path / f'{name}_{r}.nc'))
    folder = str(tmp_path / 'model')
    state = np.random.get_state()
    try:
        model = train_CNN.main(['--train', str(tmp_path / 'train_*.nc'), '--validate', str(tmp_path / 'val_*.nc'),
                                '--model_args', repr({'div': True, 'hidden_channels': [8], 'folder': folder}),
                                '--fit_args', repr({'num_epochs': 2, 'batch_size': 4, 'learning_rate': 0.01, 'verbose': False})])
    finally:
        np.random.set_state(state)
    assert isinstance(model, OLSModel) and model.div is True
    assert isinstance(model.trained_net, train_CNN.FluxFormCNN)
    assert json.load(open(os.path.join(folder, 'model_args.json')))['div'] is True
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, OLSModel) and loaded.div is True
    assert len(model.trained_net.log_dict['loss']) == 2 and np.isfinite(model.trained_net.log_dict['loss_test']).all()
