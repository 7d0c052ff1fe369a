"""GPU: training of MeanVarModel's two nets on the device (tools/train_CNN.py: FusedHeadCNN, train, fit_meanvar over
csrc/train_head.hip and csrc/conv_train.hip) against the reference's nets restated on torch CPU modules in float64
(tests/head_restatement.py: var_net, two_stage_fit).

As in tests/test_gpu_cnn_training.py the yardstick is the float32 torch CPU evaluation of the SAME state dict: the device may
deviate from float64 by at most MARGIN = 8 times what that evaluation deviates (per tensor, relative to its largest magnitude)."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import head_restatement as hr

pytestmark = pytest.mark.gpu

MARGIN = 8.0
HIDDEN, N, B = [5, 3], 16, 4


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _batch(seed, n=B):
    """inputs, and targets as a variance net sees them: squares"""
    rs = np.random.RandomState(seed)
    return rs.randn(n, 2, N, N).astype(np.float32), (rs.randn(n, 2, N, N) ** 2).astype(np.float32)


def _one_step(net, loss_of):
    """train-mode forward, loss, backward -> {name: array}: the loss, every parameter's gradient, the running statistics"""
    net.train()
    net.zero_grad()
    loss = loss_of(net)['loss']
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


def _compare(got, r64, r32, what):
    assert list(got) == list(r64) and len(got) == 1 + 6 + 4 + 4
    print(f'\n  {what}')
    worst = {}
    for k in r64:
        assert got[k].shape == r64[k].shape
        worst[k] = (_rel(got[k], r64[k]), _rel(r32[k], r64[k]))
        print(f'  {k:28s} device {worst[k][0]:.2e}   float32 torch CPU {worst[k][1]:.2e}')
    for k, (dev, cpu) in worst.items():
        assert dev <= MARGIN * cpu, (what, k, dev, cpu)
    return worst


def test_one_step_of_a_softplus_net_and_the_indexed_loss():
    """compute_loss (torch expressions at both ends) and indexed_loss (the kernels at both ends) of one state dict: the loss,
    every parameter's gradient and the running statistics against float64, and against each other"""
    from pyqg_generative_amd.tools.train_CNN import FusedHeadCNN
    from pyqg_generative_amd.tools.train_ops import HEAD_LAUNCHES
    sd = {k: v.clone() for k, v in FusedHeadCNN(2, 2, HIDDEN, head='softplus_mse', seed=21).state_dict().items()}
    X, T = _batch(31, 7)
    idx = np.array([5, 0, 6, 2])
    x, y = X[idx], T[idx]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        xt, yt = torch.tensor(x, dtype=dtype), torch.tensor(y, dtype=dtype)
        ref[dtype] = _one_step(hr.var_net(2, 2, HIDDEN, dtype, sd), lambda net: net.compute_loss(xt, yt))
    r64, r32 = ref[torch.float64], ref[torch.float32]

    def device_net():
        net = FusedHeadCNN(2, 2, HIDDEN, head='softplus_mse', seed=99)
        net.load_state_dict(sd)
        return net.to(_dev())
    xd, yd = torch.tensor(x).to(_dev()), torch.tensor(y).to(_dev())
    plain = _one_step(device_net(), lambda net: net.compute_loss(xd, yd))
    worst = _compare(plain, r64, r32, 'compute_loss: torch expressions at both ends')
    Xd, Td, idxd = torch.tensor(X).to(_dev()), torch.tensor(T).to(_dev()), torch.tensor(idx).to(_dev())
    before = dict(HEAD_LAUNCHES)
    fused = _one_step(device_net(), lambda net: net.indexed_loss(Xd, Td, idxd))
    assert [HEAD_LAUNCHES[k] - before[k] for k in ('gather', 'loss', 'grad', 'apply')] == [1, 1, 1, 0]
    _compare(fused, r64, r32, 'indexed_loss: the kernels at both ends')
    for k, (_, cpu) in worst.items():
        assert np.abs(fused[k] - plain[k]).max() <= MARGIN * cpu * np.abs(r64[k]).max(), k
    # the inference surface: planar softplus(conv(x)) in eval mode, from the engine layout
    net = device_net()
    net.eval()
    m64 = hr.var_net(2, 2, HIDDEN, torch.float64, sd).eval()
    m32 = hr.var_net(2, 2, HIDDEN, torch.float32, sd).eval()
    with torch.no_grad():
        want, cpu = m64(torch.tensor(x, dtype=torch.float64)).numpy(), m32(torch.tensor(x)).numpy()
        got = net(xd)
    assert got.shape == (4, 2, N, N) and got.is_contiguous() and not got.requires_grad and float(got.min()) > 0
    assert _rel(got.cpu().numpy(), want) <= MARGIN * _rel(cpu, want)


def test_trajectory_of_ten_adam_steps_through_train():
    """train()'s loop with a net that offers the indexed loss: 8 samples in batches of 4 over 5 epochs, the batch order fixed;
    every training and test batch goes through the kernels"""
    from pyqg_generative_amd.tools.train_CNN import FusedHeadCNN, train
    from pyqg_generative_amd.tools.train_ops import HEAD_LAUNCHES
    net = FusedHeadCNN(2, 2, HIDDEN, head='softplus_mse', seed=22)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, y = _batch(32, 8)
    xt, yt = _batch(33, 4)
    orders = cr.fixed_orders(70)
    E, lr = 5, 1e-3

    def displacement(after):
        return np.concatenate([(after[k].detach().cpu().to(torch.float64) - sd[k].to(torch.float64)).reshape(-1).numpy()
                               for k in sd if k.endswith(('.weight', '.bias'))])
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = hr.var_net(2, 2, HIDDEN, dtype, sd)
        log = cr.reference_loop(m, x, y, xt, yt, E, 4, lr, orders)
        ref[dtype] = (displacement(m.state_dict()), log)
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    before = dict(HEAD_LAUNCHES)
    train(net, x, y, xt, yt, E, 4, lr, device=0, orders=orders, verbose=False)
    assert [HEAD_LAUNCHES[k] - before[k] for k in ('gather', 'loss', 'grad', 'apply')] == [15, 15, 10, 0]
    assert int(net.state_dict()['conv.2.num_batches_tracked']) == 10
    dd = displacement(net.state_dict())
    dev, cpu = _rel(dd, d64), _rel(d32, d64)
    print(f'\n  displacement after ten steps: device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu:.2f}')
    assert np.abs(d64).max() > 1e-3
    assert dev <= MARGIN * cpu
    log64 = ref[torch.float64][1]
    assert len(net.log_dict['loss']) == E and len(net.log_dict['loss_test']) == E
    np.testing.assert_allclose(net.log_dict['loss'], log64['loss'], rtol=1e-4)
    np.testing.assert_allclose(net.log_dict['loss_test'], log64['loss_test'], rtol=1e-4)
    # an order the kernels could not check is refused on the host
    with pytest.raises(ValueError, match='orders'):
        train(net, x, y, xt, yt, 1, 4, lr, device=0, orders=lambda epoch, n: np.arange(1, n + 1), verbose=False)


def test_command_line_trains_a_folder_that_test_offline_accepts(tmp_path):
    """python -m pyqg_generative_amd.tools.train_CNN --model MeanVarModel, in process: one file per run, two epochs with the
    shuffles of numpy's global stream (put back afterwards), --test writing offline.nc"""
    from pyqg_generative_amd.models import MeanVarModel
    from pyqg_generative_amd.tools import train_CNN, xr_lite
    from pyqg_generative_amd.tools.simulate import load_parameterization, dataset_backend
    dims = ['run', 'time', 'lev', 'y', 'x']
    for name, seed in (('train', 1), ('val', 2), ('test', 5)):
        _, q, y = hr.noisy_fit_dataset(seed)
        for r in range(len(q)):
            fields = {'q': (dims, q[r:r + 1]), 'q_forcing_advection': (dims, y[r:r + 1])}
            if name == 'test':
                fields['psi'] = (dims, 1e8 * q[r:r + 1])
            xr_lite.Dataset(fields, coords={'time': (('time',), np.arange(q.shape[1], dtype='float32') * 1000.)}).to_netcdf(
                str(tmp_path / f'{name}_{r}.nc'))
    folder = str(tmp_path / 'model')
    state = np.random.get_state()
    try:
        model = train_CNN.main(['--model', 'MeanVarModel', '--train', str(tmp_path / 'train_*.nc'), '--validate', str(tmp_path / 'val_*.nc'),
                                '--test', str(tmp_path / 'test_*.nc'), '--model_args', repr({'hidden_channels': [8], 'folder': folder}),
                                '--fit_args', repr({'num_epochs': 2, 'batch_size': 4, 'learning_rate': 0.01, 'verbose': False})])
    finally:
        np.random.set_state(state)
    assert isinstance(model, MeanVarModel) and isinstance(load_parameterization(folder).param, MeanVarModel)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net_mean.pt', 'net_var.pt', 'offline.nc', 'stats_mean.nc', 'stats_var.nc',
                                          'x_scale.json', 'y_scale.json']
    assert len(model.trained_net_var.log_dict['loss']) == 2 and np.isfinite(model.trained_net_var.log_dict['loss_test']).all()
    offline = dataset_backend().open_dataset(os.path.join(folder, 'offline.nc'))
    gen = np.asarray(offline['q_forcing_advection_gen'].values)
    assert gen.shape == (2, 6, 2, 16, 16) and np.isfinite(gen).all() and np.abs(gen).max() > 0


def test_fit_meanvar_end_to_end(tmp_path):
    """fit_meanvar on 2 runs x 6 times at 16 x 16: conv_train_restatement.fit_dataset's fields with heteroscedastic noise on the
    target, hidden_channels [8], batch 4, learning rate 0.01, 12 epochs, fixed orders.

    The criterion is not that net_var's loss falls by some factor: its target, a squared residual, is chi-square noisy, and the
    float64 CPU restatement of this very fit brings net_var's loss_test only from 0.7230 to 0.5366, a factor 0.742 (printed
    below; the float32 loop agrees to seven digits).  Instead every epoch's loss and loss_test of both nets must agree with that float64 fit,
    started from the same two seeded state dicts, within 8 x the float32 CPU fit's own deviation at that epoch, floored at 1e-5
    relative."""
    from pyqg_generative_amd.models import MeanVarModel
    from pyqg_generative_amd.tools.train_CNN import fit_meanvar, FusedHeadCNN, prepare_PV_data
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation, dataset_backend
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    f = cr.FIT
    E, hidden, seed = 12, f['hidden_channels'], f['seed']
    (ds_train, q, y), (ds_test, qt, _) = hr.noisy_fit_dataset(1), hr.noisy_fit_dataset(2)
    orders = cr.fixed_orders(50)
    folder = str(tmp_path / 'model')
    kw = dict(hidden_channels=hidden, folder=folder, num_epochs=E, batch_size=f['batch_size'], learning_rate=f['learning_rate'],
              seed=seed, orders=orders, verbose=False)
    model = fit_meanvar(ds_train, ds_test, **kw)
    assert isinstance(model, MeanVarModel)
    files = ['model_args.json', 'net_mean.pt', 'net_var.pt', 'stats_mean.nc', 'stats_var.nc', 'x_scale.json', 'y_scale.json']
    assert sorted(os.listdir(folder)) == files
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='MeanVarModel', hidden_channels=hidden)
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, MeanVarModel) and loaded.hidden_channels == hidden
    np.testing.assert_array_equal(loaded.x_scale.std.reshape(-1), q.std(axis=(0, 1, 3, 4)).astype('float32'))
    np.testing.assert_array_equal(loaded.y_scale.std.reshape(-1), y.std(axis=(0, 1, 3, 4)).astype('float32'))

    # predict = the trained nets' eval-mode forward
    net_mean, net_var = model.trained_net_mean, model.trained_net_var
    net_mean.eval(), net_var.eval()
    X = (qt.reshape(-1, 2, f['N'], f['N']) / loaded.x_scale.std).astype('float32')
    with torch.no_grad():
        want_mean = net_mean(torch.tensor(X).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
        want_var = net_var(torch.tensor(X).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std.astype(np.float64) ** 2
    pred = loaded.predict(ds_test, seed=1)
    got_mean = np.asarray(pred['q_forcing_advection_mean'].values).reshape(want_mean.shape)
    got_var = np.asarray(pred['q_forcing_advection_var'].values).reshape(want_var.shape)
    assert np.abs(got_mean - want_mean).max() <= 2e-5 * np.abs(want_mean).max()
    assert np.abs(got_var - want_var).max() <= 2e-5 * np.abs(want_var).max()
    assert (got_var > 0).all() and (want_var > 0).all()

    # the logs against the two-stage fit on the CPU, from the same two initial states
    mean0 = FusedHeadCNN(2, 2, hidden, head='mse', seed=seed).state_dict()
    var0 = FusedHeadCNN(2, 2, hidden, head='softplus_mse', seed=seed + 1).state_dict()
    data = prepare_PV_data(ds_train, ds_test)[:4]
    cpu = {dtype: hr.two_stage_fit(mean0, var0, hidden, *data, E, f['batch_size'], f['learning_rate'], orders, dtype)[:2]
           for dtype in (torch.float64, torch.float32)}
    lv = cpu[torch.float64][1]['loss_test']
    print(f'\n  float64 CPU fit, net_var loss_test: first {lv[0]:.4f}, last {lv[-1]:.4f}, factor {lv[-1] / lv[0]:.3f}')
    failures = []
    for i, (name, net) in enumerate((('mean', net_mean), ('var', net_var))):
        stats = dataset_backend().open_dataset(os.path.join(folder, f'stats_{name}.nc'))
        for key in ('loss', 'loss_test'):
            got = np.asarray(stats[key].values)
            assert got.shape == (E,) and np.array_equal(got, net.log_dict[key]) and np.isfinite(got).all()
            l64, l32 = np.asarray(cpu[torch.float64][i][key]), np.asarray(cpu[torch.float32][i][key])
            dev, ref = np.abs(got - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
            print(f'  net_{name} {key:9s} worst over epochs: device {dev.max():.2e}   float32 torch CPU {ref.max():.2e}   '
                  f'worst device / max(8 x CPU, 1e-5) {np.max(dev / np.maximum(MARGIN * ref, 1e-5)):.2f}')
            if not (dev <= np.maximum(MARGIN * ref, 1e-5)).all():
                failures.append((name, key, dev.tolist(), ref.tolist()))
    assert not failures, failures

    # online: one parameterized step
    Ns = 32
    q0 = np.random.RandomState(4).randn(2, Ns, Ns) * np.array([8e-6, 1e-6]).reshape(2, 1, 1)
    params = EDDY_PARAMS.nx(Ns)._update({'tmax': 14400., 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=loaded, sampling='constant', nsteps=1), q_init=q0, sampling_freq=14400.)
    qq = np.asarray(out['q'].values)
    assert qq.shape[-3:] == (2, Ns, Ns) and np.isfinite(qq).all() and np.abs(qq[-1] - q0).max() > 0

    # a second call on the folder: net_mean is read, only net_var is trained, and it comes out bit for bit
    read = lambda name: torch.load(os.path.join(folder, name), map_location='cpu', weights_only=True)
    first = {name: read(name) for name in ('net_mean.pt', 'net_var.pt')}
    stats_mean = open(os.path.join(folder, 'stats_mean.nc'), 'rb').read()
    again = fit_meanvar(ds_train, ds_test, **kw)
    assert not again.trained_net_mean.log_dict.get('loss') and len(again.trained_net_var.log_dict['loss']) == E
    assert sorted(os.listdir(folder)) == files and open(os.path.join(folder, 'stats_mean.nc'), 'rb').read() == stats_mean
    for name, sd in first.items():
        back = read(name)
        assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items()), name
    # a folder whose net_mean was trained on other data is refused
    with pytest.raises(ValueError, match='scale'):
        fit_meanvar(hr.noisy_fit_dataset(3)[0], ds_test, **kw)
