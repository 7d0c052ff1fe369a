"""GPU: training of AndrewCNN nets on the device (tools/train_CNN.py over csrc/conv_train.hip): a whole net's loss, gradients
and running statistics, a ten-step Adam trajectory, and fit_ols end to end, against the reference's net restated on torch CPU
modules (tests/conv_train_restatement.py::torch_net) in float64.

The yardstick of the first two is the float32 torch CPU evaluation of the SAME net: the device result may deviate from float64
by at most MARGIN = 8 times what that evaluation deviates (per tensor, relative to the tensor's largest magnitude).  A sequential
fmaf chain (the matrix cores' exact-f32 sum) against the library's 16-lane blocked sums is expected to differ by up to
sqrt(16) = 4 x, with 2 x headroom on top."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr

pytestmark = pytest.mark.gpu

MARGIN = 8.0
HIDDEN, N, B = [5, 3], 16, 4


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _batch(seed, n=B):
    rs = np.random.RandomState(seed)
    return rs.randn(n, 2, N, N).astype(np.float32), rs.randn(n, 2, N, N).astype(np.float32)


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
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN
    net = TrainableAndrewCNN(2, 2, HIDDEN, batch_norm=batch_norm, bias=True, seed=21)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x, y = _batch(31)
    r64 = _one_step(cr.torch_net(2, 2, HIDDEN, batch_norm, True, torch.float64, sd), torch.tensor(x, dtype=torch.float64),
                    torch.tensor(y, dtype=torch.float64))
    r32 = _one_step(cr.torch_net(2, 2, HIDDEN, batch_norm, True, torch.float32, sd), torch.tensor(x), torch.tensor(y))
    net.to(_dev())
    got = _one_step(net, torch.tensor(x).to(_dev()), torch.tensor(y).to(_dev()))
    assert list(got) == list(r64) and len(got) == 1 + 6 + (4 if batch_norm else 0) + (4 if batch_norm else 0)
    print()
    worst = {}
    for k in r64:
        assert got[k].shape == r64[k].shape
        dev, cpu = _rel(got[k], r64[k]), _rel(r32[k], r64[k])
        worst[k] = (dev, cpu)
        print(f'  {k:28s} device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu if cpu else float("inf"):.2f}')
    for k, (dev, cpu) in worst.items():
        assert dev <= MARGIN * cpu, (k, dev, cpu)


def test_trajectory_of_ten_adam_steps():
    """train()'s loop itself: 8 samples in batches of 4 over 5 epochs (ten steps, the schedule's three decays included), the
    batch order fixed; the deviation is that of the parameters' displacement from the float64 torch loop"""
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN, train
    net = TrainableAndrewCNN(2, 2, HIDDEN, batch_norm=True, bias=True, seed=22)
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
        m = cr.torch_net(2, 2, HIDDEN, True, True, dtype, sd)
        log = cr.reference_loop(m, x, y, xt, yt, E, 4, lr, orders)
        ref[dtype] = (displacement(m.state_dict()), log)
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    train(net, x, y, xt, yt, E, 4, lr, device=0, orders=orders, verbose=False)
    assert int(net.state_dict()['conv.2.num_batches_tracked']) == 10
    dd = displacement(net.state_dict())
    dev, cpu = _rel(dd, d64), _rel(d32, d64)
    print(f'\n  displacement after ten steps: device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu:.2f}')
    assert np.abs(d64).max() > 1e-3                    # the parameters moved
    assert dev <= MARGIN * cpu
    log64 = ref[torch.float64][1]
    assert log64['loss'][-1] < log64['loss'][0]
    assert len(net.log_dict['loss']) == E and len(net.log_dict['loss_test']) == E
    np.testing.assert_allclose(net.log_dict['loss'], log64['loss'], rtol=1e-4)
    np.testing.assert_allclose(net.log_dict['loss_test'], log64['loss_test'], rtol=1e-4)


def test_circular_conv2d_surface():
    """through torch.autograd with and without a gradient for x: no data-gradient launch for an input that needs none"""
    from pyqg_generative_amd.tools import train_ops as T
    cin, cout, k = 5, 7, 3
    x, w, b, dy = cr.case_data(cin, cout, k, 2, N, 5, integer=True)
    want_dw, want_db = cr.backward_weight(x, dy, cin, cout, k)
    for needs in (False, True):
        xd = torch.tensor(x).to(_dev()).requires_grad_(needs)
        wd, bd = (torch.tensor(a).to(_dev()).requires_grad_(True) for a in (w, b))
        before = dict(T.LAUNCHES)
        y = T.circular_conv2d(xd, wd, bd)
        assert np.array_equal(y.detach().cpu().numpy().astype(np.float64), cr.forward(x, w, b))
        y.backward(torch.tensor(dy).to(_dev()))
        assert T.LAUNCHES['forward'] - before['forward'] == 1 and T.LAUNCHES['backward_weight'] - before['backward_weight'] == 1
        assert T.LAUNCHES['backward_data'] - before['backward_data'] == (1 if needs else 0)
        assert np.array_equal(wd.grad.cpu().numpy().astype(np.float64), want_dw)
        assert np.array_equal(bd.grad.cpu().numpy().astype(np.float64), want_db)
        if needs:
            assert np.array_equal(xd.grad.cpu().numpy().astype(np.float64), cr.backward_data(dy, w))
        else:
            assert xd.grad is None
    # no bias: two inputs, no db
    xd, wd = torch.tensor(x).to(_dev()), torch.tensor(w).to(_dev()).requires_grad_(True)
    T.circular_conv2d(xd, wd).backward(torch.tensor(dy).to(_dev()))
    assert np.array_equal(wd.grad.cpu().numpy().astype(np.float64), want_dw)
    # a layout the engine does not take is refused by the facade
    with pytest.raises(ValueError, match='engine layout'):
        T.circular_conv2d(torch.zeros(2, 5, N, N, device=_dev()), wd)
    # the workspace is cached per shape
    n = len(T._WORK)
    T.circular_conv2d(xd, wd)
    assert len(T._WORK) == n


def test_fit_ols_end_to_end(tmp_path):
    """fit_ols on 2 runs x 6 times at 16 x 16 (q Gaussian, the target a fixed circular 3 x 3 stencil of q), hidden_channels [8],
    batch 4, learning rate 0.01: the folder, the loaders, predict against the trained net, one online step, and the loss.

    The epoch count.  The reference's loop restated in float32 torch on the CPU (conv_train_restatement.reference_loop), on this
    dataset, seed and batch order, brings loss_test from 0.795 after the first epoch to 0.297 of that after 6 epochs and to 0.177
    after 8: 8 is the count at which that loop alone reaches a quarter, and the device must reach a half."""
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.tools.train_CNN import fit_ols
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation, dataset_backend
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    f = cr.FIT
    E = 8
    ds_train, ds_test = cr.fit_dataset(1), cr.fit_dataset(2)
    folder = str(tmp_path / 'model')
    model = fit_ols(ds_train, ds_test, hidden_channels=f['hidden_channels'], folder=folder, num_epochs=E, batch_size=f['batch_size'],
                    learning_rate=f['learning_rate'], seed=f['seed'], orders=cr.fixed_orders(50), verbose=False)
    assert isinstance(model, OLSModel)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'stats.nc', 'x_scale.json', 'y_scale.json']
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(
        model='OLSModel', div=False, batch_norm=True, bias=True, final_activation='None', hidden_channels=f['hidden_channels'])
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, OLSModel) and loaded.hidden_channels == f['hidden_channels']
    # the scalers are the training set's channelwise std
    q, y = cr.fit_fields(1)
    np.testing.assert_array_equal(loaded.x_scale.std.reshape(-1), q.std(axis=(0, 1, 3, 4)).astype('float32'))
    np.testing.assert_array_equal(loaded.y_scale.std.reshape(-1), y.std(axis=(0, 1, 3, 4)).astype('float32'))
    # predict = the trained net's eval-mode forward, to the generic engine's tolerance
    net = model.trained_net
    net.eval()
    qt = cr.fit_fields(2)[0]
    X = (qt.reshape(-1, 2, f['N'], f['N']) / loaded.x_scale.std).astype('float32')
    with torch.no_grad():
        want = net(torch.tensor(X).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
    got = np.asarray(loaded.predict(ds_test)['q_forcing_advection'].values).reshape(want.shape)
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    # the log: stats.nc holds what train() logged, and the test loss fell below half its first value
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    lt = np.asarray(stats['loss_test'].values)
    assert lt.shape == (E,) and np.array_equal(lt, net.log_dict['loss_test']) and np.isfinite(lt).all()
    assert np.asarray(stats['loss'].values).shape == (E,)
    print(f'\n  loss_test per epoch: {np.round(lt, 4).tolist()}   last / first = {lt[-1] / lt[0]:.3f}')
    assert lt[-1] < 0.5 * lt[0]
    # online: one parameterized step
    Ns = 32
    q0 = np.random.RandomState(4).randn(2, Ns, Ns) * np.array([8e-6, 1e-6]).reshape(2, 1, 1)
    params = EDDY_PARAMS.nx(Ns)._update({'tmax': 14400., 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=loaded, sampling='constant', nsteps=1), q_init=q0, sampling_freq=14400.)
    qq = np.asarray(out['q'].values)
    assert qq.shape[-3:] == (2, Ns, Ns) and np.isfinite(qq).all() and np.abs(qq[-1] - q0).max() > 0
