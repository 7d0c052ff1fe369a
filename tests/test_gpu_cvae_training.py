"""GPU: training of CVAERegression on the device (tools/train_CVAE.py: TrainableCVAE, train_CVAE, fit_cvae over
csrc/latent_train.hip, csrc/train_head.hip, csrc/conv_train.hip and csrc/fluxdiv_train.hip) against the reference's three nets
and loss restated on torch CPU modules in float64 (tests/latent_restatement.py: TorchCVAE, reference_loop).

As in tests/test_gpu_cnn_training.py the yardstick is the float32 torch CPU evaluation of the SAME state dicts: the device may
deviate from float64 by at most MARGIN = 8 times what that evaluation deviates (per tensor, relative to its largest magnitude).
Shape: 16 x 16, batch 4, a decoder of hidden_channels [5, 3] (the encoder always has the default widths), eps given."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import latent_restatement as lr

pytestmark = pytest.mark.gpu

MARGIN = 8.0
HIDDEN, N, B = [5, 3], 16, 4


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _sets(seed, n, div=False):
    """X, Y, Y_mean planar (n, 2, N, N) float32; Y and Y_mean are multiples of 2^-10, so that T = Y - Y_mean is exact; with div
    every plane of Y - Y_mean has zero mean up to that grid, as a flux-form net can produce it"""
    rs = np.random.RandomState(seed)
    X, T, M = rs.randn(n, 2, N, N), rs.randn(n, 2, N, N), rs.randn(n, 2, N, N)
    if div:
        T, M = T - T.mean(axis=(-2, -1), keepdims=True), M - M.mean(axis=(-2, -1), keepdims=True)
    q = lambda a: (np.round(a * 1024) / 1024).astype(np.float32)
    T, M = q(T), q(M)
    return X.astype(np.float32), T + M, M


def _states(net):
    return {k: {a: b.clone() for a, b in getattr(net, k).state_dict().items()} for k in ('encoder', 'decoder', 'net_mean') if hasattr(net, k)}


def _collect(losses, modules):
    out = {k: np.array([float(losses[k].detach())]) for k in lr.KEYS}
    for name, m in modules:
        for k, p in m.named_parameters():
            out[f'grad {name}.{k}'] = p.grad.detach().cpu().numpy().astype(np.float64)
    return out


def _cpu_step(states, cfg, x, y, ymean, eps, dtype):
    """-> ({name: array}, the smallest magnitude among the inputs of every ReLU of encoder and decoder)"""
    decoder_var, regression, div = cfg
    model = lr.TorchCVAE(regression, decoder_var, div, HIDDEN, dtype, states)
    nearest = []
    for m in model.modules():
        m.train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.ReLU):
                mod.register_forward_hook(lambda _, inp, out: nearest.append(float(inp[0].detach().abs().min())))
    t = lambda a: torch.tensor(a, dtype=dtype)
    losses = model.compute_loss(t(x), t(y), t(ymean), t(eps))
    losses['loss'].backward()
    assert len(nearest) == 7 + len(HIDDEN)
    return _collect(losses, (('encoder', model.encoder), ('decoder', model.decoder))), min(nearest)


CONFIGS = [('adaptive', 'None', False), ('fixed', 'full_loss', False), (0.1, 'None', False), ('adaptive', 'None', True)]
# A gradient is compared at a point where the loss is differentiable WITHIN ROUNDING only if no input of a ReLU is within
# rounding of zero: a float32 convolution output is a sum of up to K = 128 * 25 = 3200 products of O(1) batch-normalised
# activations, which deviates by about sqrt(K) = 57 roundings of 2^-24; an element nearer to zero than that may come out
# on the other side in another float32 evaluation, and one flipped element of a 32-channel layer moves that layer's bias
# gradient by about 1 / sqrt(1024) = 3 %.  The encoder's 370 000 ReLU inputs put the nearest one at 1e-6 ... 5e-6 typically, so
# the data seeds are those of range(31, 43) whose float64 evaluation keeps all of them 64 * 2^-24 = 3.8e-6 away (34 without
# div: 5.4e-6, 32 with: 4.9e-6), and the test asserts that before it compares anything.
KINK = 64 * 2.0 ** -24
DATA_SEED = {False: 34, True: 32}


@pytest.mark.parametrize('cfg', CONFIGS, ids=['adaptive', 'fixed-full_loss', '0.1', 'adaptive-div'])
def test_one_step_of_the_indexed_loss(cfg):
    """the six values and every parameter gradient of indexed_loss (the kernels) against the float64 torch evaluation of the
    reference's statement on the same state dicts; the six values of compute_loss (torch expressions on the device) against
    those of indexed_loss"""
    from pyqg_generative_amd.tools.train_CVAE import TrainableCVAE
    from pyqg_generative_amd.tools import train_ops as T
    decoder_var, regression, div = cfg
    net = TrainableCVAE(regression, decoder_var, div, HIDDEN, seed=21)
    states = _states(net)
    X, Y, Y_mean = _sets(DATA_SEED[div], 7, div)
    idx = np.array([5, 0, 6, 2])
    eps = np.random.RandomState(41).randn(B, 2, N, N).astype(np.float32)
    ref = {dtype: _cpu_step(states, cfg, X[idx], Y[idx], Y_mean[idx], eps, dtype) for dtype in (torch.float64, torch.float32)}
    (r64, nearest), (r32, _) = ref[torch.float64], ref[torch.float32]
    print(f'\n  the ReLU input nearest to zero: {nearest:.2e} (at least {KINK:.2e})')
    assert nearest >= KINK
    if decoder_var == 'adaptive':
        assert r64['loss_recon'][0] == pytest.approx(N * N, rel=1e-13)

    def device_net():
        m = TrainableCVAE(regression, decoder_var, div, HIDDEN, seed=99)
        for k, sd in states.items():
            getattr(m, k).load_state_dict(sd)
        return m.to(_dev()).train()
    up = lambda a: torch.tensor(a).to(_dev())
    Xd, Yd, Md, idxd, epsd = up(X), up(Y), up(Y_mean), up(idx), up(eps)
    Td = Yd - Md if regression != 'None' else Yd
    assert np.array_equal(Td.cpu().numpy().astype(np.float64), (Y.astype(np.float64) - Y_mean) if regression != 'None' else Y)
    m = device_net()
    before = (dict(T.LATENT_LAUNCHES), dict(T.HEAD_LAUNCHES))
    losses = m.indexed_loss(torch.cat([Xd, Yd], 1), Xd, Td, idxd, 0, epsd)
    assert list(losses) == lr.KEYS and all(v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda for v in losses.values())
    losses['loss'].backward()
    assert [T.LATENT_LAUNCHES[k] - before[0][k] for k in ('forward', 'backward', 'prior')] == [1, 1, 0]
    assert [T.HEAD_LAUNCHES[k] - before[1][k] for k in ('gather', 'loss', 'grad', 'apply')] == [1, 1, 1, 0]
    fused = _collect(losses, (('encoder', m.encoder), ('decoder', m.decoder)))
    m = device_net()
    losses = m.compute_loss(Xd[idxd], Yd[idxd], Md[idxd], epsd)
    losses['loss'].backward()
    plain = _collect(losses, (('encoder', m.encoder), ('decoder', m.decoder)))
    if decoder_var == 'adaptive':
        assert fused['loss_recon'][0] == N * N
    failures = []
    assert list(fused) == list(r64) == list(plain)
    print(f'\n  {cfg} indexed_loss: the kernels')
    for k in r64:
        assert fused[k].shape == r64[k].shape
        dev, cpu = _rel(fused[k], r64[k]), _rel(r32[k], r64[k])
        print(f'  {k:32s} device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu if cpu else (0.0 if dev == 0 else float("inf")):.2f}')
        if decoder_var == 'adaptive' and k == 'loss_recon':
            continue            # the identity N^2, which the device gives exactly (above); float64 torch is within 2^-52 of it
        if not dev <= MARGIN * cpu:
            failures.append((k, dev, cpu))
    assert not failures, failures
    # compute_loss, the same statement in torch expressions on the device: a second float32 evaluation of the six values.  A
    # float32 sum of up to 3200 products deviates by about 64 roundings, 4e-6, and there are two evaluations: 1e-5
    print(f'  {cfg} compute_loss (torch expressions on the device) against indexed_loss, and against float64:')
    for k in lr.KEYS:
        print(f'  {k:32s} {abs(plain[k][0] - fused[k][0]) / abs(fused[k][0]):.2e}   {_rel(plain[k], r64[k]):.2e}')
        assert abs(plain[k][0] - fused[k][0]) <= 1e-5 * abs(fused[k][0]), k
    for k in r64:
        if k.startswith('grad'):
            assert plain[k].shape == r64[k].shape and np.isfinite(plain[k]).all()


def test_trajectory_of_ten_adam_steps_through_train_CVAE():
    """train_CVAE's loop: 8 samples in batches of 4 over 5 epochs (ten steps, the schedule's three decays included), the batch
    order fixed, the latent noise drawn in the kernels; the CPU loops take the oracle's Philox normals of the same (seed, step)"""
    from pyqg_generative_amd.tools.train_CVAE import TrainableCVAE, train_CVAE
    from pyqg_generative_amd.tools import train_ops as T
    net = TrainableCVAE('None', 'adaptive', False, HIDDEN, seed=22)
    states = _states(net)
    X, Y, _ = _sets(32, 8)
    orders = cr.fixed_orders(70)
    E, rate = 5, 1e-3

    def displacement(model):
        return np.concatenate([(getattr(model, name).state_dict()[k].detach().cpu().to(torch.float64) - sd[k].to(torch.float64)).reshape(-1).numpy()
                               for name, sd in states.items() for k in sd if k.endswith(('.weight', '.bias'))])
    ref = {}
    for dtype in (torch.float64, torch.float32):
        model = lr.TorchCVAE('None', 'adaptive', False, HIDDEN, dtype, states)
        log = lr.reference_loop(model, X, Y, 0 * Y, E, B, rate, orders, net.seed)
        ref[dtype] = (displacement(model), log)
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    before = (dict(T.LATENT_LAUNCHES), dict(T.HEAD_LAUNCHES))
    optim_loss, log_train, log_test = train_CVAE(net, X, Y, E, B, rate, device=0, orders=orders, verbose=False)
    assert [T.LATENT_LAUNCHES[k] - before[0][k] for k in ('forward', 'backward', 'prior')] == [10, 10, 0]
    assert [T.HEAD_LAUNCHES[k] - before[1][k] for k in ('gather', 'loss', 'grad', 'apply')] == [10, 10, 10, 0]
    assert log_train == [] and log_test == [] and list(optim_loss) == lr.KEYS
    assert int(net.encoder.state_dict()['conv.2.num_batches_tracked']) == 10
    dd = displacement(net)
    dev, cpu = _rel(dd, d64), _rel(d32, d64)
    print(f'\n  displacement after ten steps: device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu:.2f}')
    assert np.abs(d64).max() > 1e-3                    # the parameters moved
    assert dev <= MARGIN * cpu
    # the epochs' logged means: within 8 x the float32 CPU loop's own deviation, floored at 1e-5 relative (the rule of
    # tests/test_gpu_meanvar_training.py's end-to-end fit)
    log64, log32 = ref[torch.float64][1], ref[torch.float32][1]
    for k in lr.KEYS:
        got, l64, l32 = (np.asarray(v, np.float64) for v in (optim_loss[k], log64[k], log32[k]))
        assert got.shape == (E,)
        d, r = np.abs(got - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
        print(f'  {k:10s} worst over epochs: device {d.max():.2e}   float32 torch CPU {r.max():.2e}')
        assert (d <= np.maximum(MARGIN * r, 1e-5)).all(), (k, d.tolist(), r.tolist())
    assert optim_loss['loss_recon'] == [float(N * N)] * E
    # an order the kernels could not check is refused on the host
    with pytest.raises(ValueError, match='orders'):
        train_CVAE(net, X, Y, 1, B, rate, device=0, orders=lambda epoch, n: np.arange(1, n + 1), verbose=False)


FILES = ['decoder.pt', 'encoder.pt', 'model_args.json', 'stats.nc', 'x_scale.json', 'y_scale.json']


def test_fit_cvae_end_to_end(tmp_path):
    """fit_cvae on conv_train_restatement.fit_dataset's 2 runs x 6 times at 16 x 16: decoder hidden_channels [8], batch 4,
    learning rate 0.01, three epochs, fixed orders, one scored run per epoch chosen by the hook"""
    from pyqg_generative_amd.models import CVAERegression
    from pyqg_generative_amd.tools.train_CVAE import fit_cvae
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation, dataset_backend
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    f = cr.FIT
    E, hidden = 3, f['hidden_channels']
    ds_train, ds_test = cr.fit_dataset(1), cr.fit_dataset(2)
    folder = str(tmp_path / 'model')
    asked = []

    def runs(R, k):
        asked.append((R, k))
        return np.arange(R)[::-1][:k]
    model = fit_cvae(ds_train, ds_test, hidden_channels=hidden, folder=folder, num_epochs=E, batch_size=f['batch_size'],
                     learning_rate=f['learning_rate'], nruns=1, seed=f['seed'], orders=cr.fixed_orders(50), runs=runs, verbose=False)
    assert isinstance(model, CVAERegression) and asked == [(2, 1)] * (2 * E)
    assert sorted(os.listdir(folder)) == FILES
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='CVAERegression', regression='None', div=False,
                                                                            decoder_var='adaptive', hidden_channels=hidden)
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, CVAERegression) and loaded.hidden_channels == hidden

    # predict = the trained decoder's eval-mode forward on the same latent draw
    qt = np.asarray(ds_test['q'].values).reshape(-1, 2, f['N'], f['N'])
    X = (qt / loaded.x_scale.std).astype('float32')
    z = np.random.RandomState(8).randn(*X.shape).astype('float32')
    dec = model.trained_decoder.eval()
    with torch.no_grad():
        want = dec(torch.tensor(np.concatenate([X, z], 1)).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
        got = loaded.generate(torch.tensor(X).to(_dev()), torch.tensor(z).to(_dev())).cpu().numpy().astype(np.float64) * loaded.y_scale.std
    dec.train()
    assert np.abs(want).max() > 0 and np.abs(got - want).max() <= 2e-5 * np.abs(want).max()
    snap = loaded.predict_snapshot(type('M', (), {'q': qt[3].astype(np.float64)})(), z[3:4])
    assert np.abs(snap - want[3]).max() <= 2e-5 * np.abs(want).max()
    pred = loaded.predict(ds_test, M=2, seed=1)
    assert np.isfinite(np.asarray(pred['q_forcing_advection'].values)).all()

    # the log: MSE falls, loss_recon is the pixel count in every epoch, the scores are finite
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    val = lambda k: np.asarray(stats[k].values)
    for k in lr.KEYS + ['L2_mean', 'L2_total', 'L2_residual', 'L2_mean_test', 'L2_total_test', 'L2_residual_test', 'L2_loss']:
        assert val(k).shape == (E,) and np.isfinite(val(k)).all(), k
    assert val('var_ratio').shape == (E, 2) and np.isfinite(val('var_ratio')).all()
    print(f"\n  MSE per epoch {val('MSE')}, loss_KL {val('loss_KL')}, L2_loss {val('L2_loss')}, Epoch_opt {int(val('Epoch_opt'))}")
    assert val('MSE')[-1] < val('MSE')[0]
    np.testing.assert_allclose(val('loss_recon'), f['N'] ** 2, rtol=1e-12)
    np.testing.assert_allclose(val('loss'), val('loss_recon') + val('loss_KL'), rtol=1e-12)
    assert int(val('Epoch_opt')) == int(np.argmin(val('L2_loss'))) + 1

    # online: one parameterized step
    Ns = 32
    q0 = np.random.RandomState(4).randn(2, Ns, Ns) * np.array([8e-6, 1e-6]).reshape(2, 1, 1)
    params = EDDY_PARAMS.nx(Ns)._update({'tmax': 14400., 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=loaded, sampling='constant', nsteps=1), q_init=q0, sampling_freq=14400.)
    qq = np.asarray(out['q'].values)
    assert qq.shape[-3:] == (2, Ns, Ns) and np.isfinite(qq).all() and np.abs(qq[-1] - q0).max() > 0


def test_command_line_trains_a_folder_with_regression(tmp_path):
    """python -m pyqg_generative_amd.tools.train_CVAE, in process: one file per run, two epochs with regression='full_loss' and
    the shuffles of numpy's global stream (put back afterwards)"""
    from pyqg_generative_amd.models import CVAERegression
    from pyqg_generative_amd.tools import train_CVAE, xr_lite
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
        model = train_CVAE.main(['--train', str(tmp_path / 'train_*.nc'), '--validate', str(tmp_path / 'val_*.nc'),
                                 '--model_args', repr({'hidden_channels': [8], 'folder': folder, 'regression': 'full_loss', 'decoder_var': 0.1}),
                                 '--fit_args', repr({'num_epochs': 2, 'num_epochs_regression': 1, 'batch_size': 4, 'learning_rate': 0.01,
                                                     'nruns': 1, 'verbose': False})])
    finally:
        np.random.set_state(state)
    assert isinstance(model, CVAERegression) and isinstance(load_parameterization(folder).param, CVAERegression)
    assert sorted(os.listdir(folder)) == sorted(FILES + ['net_mean.pt', 'stats_mean.nc'])
    assert json.load(open(os.path.join(folder, 'model_args.json')))['decoder_var'] == 0.1
    assert len(model.trained_net_mean.log_dict['loss']) == 1
