"""CPU: the latent step of include/qgx_latent_train.h — the restatement against torch autograd of the loss as the reference
writes it, the declarations against the bindings, the partition against the workspace size, every refusal before any device
call — and the host side of CVAERegression's training in tools/train_CVAE.py: the nets' state dicts, the identity
loss_recon = N^2 under decoder_var='adaptive', the folder writer, fit_cvae's refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import latent_restatement as lr


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', [None, [4, 0, 4]], ids=['rows', 'idx'])
def test_restatement_is_torch_autograd(idx):
    B, N, n = 3, 8, 5
    enc, x, eps, w = lr.case_data(B, N, n, 7)
    et = torch.tensor(cr.from_layout(enc, 4), dtype=torch.float64, requires_grad=True)
    z, loss_KL, var_latent, var_aggr = lr.latent_torch(et, torch.tensor(eps, dtype=torch.float64))
    dec_in = torch.cat([torch.tensor(x, dtype=torch.float64)[lr.rows(idx, B)], z], 1)
    gout = 0.375
    wt = torch.tensor(cr.from_layout(w, 4), dtype=torch.float64)
    ((wt * dec_in).sum() + gout * loss_KL).backward()
    got = lr.latent_forward(enc, x, idx, eps)
    assert got['dec_in'].shape == (B, N, N, 8) and not got['dec_in'][..., 4:].any()
    np.testing.assert_allclose(cr.from_layout(got['dec_in'], 4), dec_in.detach().numpy(), rtol=1e-14, atol=1e-300)
    np.testing.assert_array_equal(cr.from_layout(got['dec_in'], 4)[:, :2], x[lr.rows(idx, B)].astype(np.float64))
    np.testing.assert_allclose(got['stats'], [float(v.detach()) for v in (loss_KL, var_latent, var_aggr)], rtol=1e-13)
    assert (got['stat_bounds'] > 0).all() and (got['A_dec_in'] >= np.abs(got['dec_in']) * (got['A_dec_in'] > 0)).all()
    # the gradient: torch's, but for the float32 rounding of the scale, which the restatement states on its own
    s = lr.scale(gout, B)
    assert s == np.float32(gout / B) and s.dtype == np.float32
    d_enc, A = lr.latent_backward(enc, eps, w, gout)
    assert d_enc.shape == (B, N, N, 8) and not d_enc[..., 4:].any() and (A >= np.abs(d_enc) - 1e-300).all()
    # with a scale that float32 holds exactly the two agree to float64 rounding
    assert float(np.float32(0.375 / 3)) == 0.125
    np.testing.assert_allclose(cr.from_layout(d_enc, 4), et.grad.numpy(), rtol=1e-12, atol=1e-14)
    # the prior: z is eps, and there are no statistics
    prior = lr.latent_forward(None, x, idx, eps)
    assert 'stats' not in prior
    np.testing.assert_array_equal(cr.from_layout(prior['dec_in'], 4)[:, 2:], eps.astype(np.float64))


def test_normals_are_the_oracles_counter_layout():
    from oracle.samplers_ref import philox_normal
    e = lr.normals(11, 5, 3, 16)
    assert e.shape == (3, 2, 16, 16) and e.dtype == np.float32
    flat = philox_normal(11, 2, 5, 512)[0]
    assert e[2, 1, 3, 7] == flat[256 + 3 * 16 + 7] and e[2, 0, 15, 15] == flat[255]
    assert not np.array_equal(e[0], e[1]) and not np.array_equal(e, lr.normals(11, 6, 3, 16))


@pytest.mark.parametrize('decoder_var,regression', [('adaptive', 'None'), ('fixed', 'full_loss'), (0.1, 'None')])
def test_loss_recon_is_the_pixel_count_under_adaptive(decoder_var, regression):
    """two channels: loss_recon = mse 2 N^2 / (2 var_p) = N^2 with var_p = mse, exactly; the reference's statement on torch CPU
    modules and TrainableCVAE's expression agree"""
    from pyqg_generative_amd.tools.train_CVAE import TrainableCVAE
    N, B, hidden = 16, 2, [5, 3]
    net = TrainableCVAE(regression, decoder_var, False, hidden, seed=4)
    states = {k: getattr(net, k).state_dict() for k in ('encoder', 'decoder') + (('net_mean',) if regression != 'None' else ())}
    model = lr.TorchCVAE(regression, decoder_var, False, hidden, torch.float64, states)
    rs = np.random.RandomState(2)
    x, y, ymean, eps = (torch.tensor(rs.randn(B, 2, N, N)) for _ in range(4))
    losses = model.compute_loss(x, y, ymean, eps)
    assert list(losses) == lr.KEYS and all(np.isfinite(float(v.detach())) for v in losses.values())
    mse = losses['MSE']
    value = {k: float(v.detach()) for k, v in losses.items()}
    want = {'adaptive': float(N * N), 'fixed': float(mse) * N * N}.get(decoder_var, float(mse) * N * N / 0.1)
    assert value['loss_recon'] == pytest.approx(want, rel=1e-13)
    assert float(net._recon(mse, N)) == pytest.approx(want, rel=1e-13)
    if decoder_var == 'adaptive':
        assert float(net._recon(torch.tensor(0.37, dtype=torch.float64), N)) == N * N
        assert net._recon(mse.clone().requires_grad_(True), N).grad_fn is not None        # the gradient flows through mse / var_p
    assert value['loss'] == pytest.approx(value['loss_recon'] + value['loss_KL'], rel=1e-14)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def _workspace_bytes(B, N):
    from pyqg_generative_amd._lib import lib
    n = C.c_size_t(0)
    return lib.qgx_latent_workspace(B, N, C.byref(n)), n.value


def test_restated_plan_gives_the_librarys_workspace_size_and_the_declared_regimes():
    grids = [(B, N) for B, N, _ in lr.LATENT_REGIMES]
    grids += [(B, N) for N in lr_grids() for B in (1, 2, 3, 9, 23, 64, 65, 130, 257, 1025, 2 ** 29 // (N * N))]
    grids += [(B, N) for N in lr_grids() for q in (8, 64, 256, 512) for B in (q * 1024 // (N * N), q * 1024 // (N * N) + 1) if B >= 1]
    for B, N in grids:
        rc, n = _workspace_bytes(B, N)
        assert rc == 0 and n == lr.latent_workspace_bytes(B, N), (B, N)
        p = lr.latent_plan(B, N)
        assert (p['nb'] - 1) * p['qpb'] < p['nq'] <= p['nb'] * p['qpb'] and p['nb'] <= 256 and p['qpb'] % 256 == 0 and p['nq'] * 4 == B * N * N
    for (B, N, _), regime in lr.LATENT_REGIMES.items():
        plan = lr.latent_plan(B, N)
        assert {key: plan[key] for key in regime} == regime, (B, N)
    # the shipped step, batch 64 at 64 x 64, is on the boundary: one more image and a lane takes a second quad
    assert lr.latent_plan(64, 64)['passes'] == 1 and lr.latent_plan(65, 64)['passes'] == 2


def lr_grids():
    return (16, 32, 48, 64, 96, 128)


# ---- declarations and bindings -----------------------------------------------------------------------------------------------
NAMES = ['qgx_latent_backward', 'qgx_latent_forward', 'qgx_latent_workspace']


def test_header_declares_what_latent_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_latent_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_latent_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.LATENT_TRAIN_SYMBOLS) == NAMES
    for name, _, args in _lib.LATENT_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    others = (_lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS + _lib.CONV_TRAIN_SYMBOLS + _lib.HEAD_TRAIN_SYMBOLS
              + _lib.FLUX_TRAIN_SYMBOLS)
    assert not {n for n, _, _ in _lib.LATENT_TRAIN_SYMBOLS} & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'latent_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_latent_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert re.search(r"0 <= idx\[b\] < n is the CALLER'S DUTY", text)
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'fit_cvae' in open(os.path.join(ROOT, doc)).read()


# ---- refusals, each without a device -----------------------------------------------------------------------------------------
GOOD = dict(B=3, N=16, n=5)
BAD_FIELDS = [('N', v) for v in (0, 8, 17, 24, 192, 256, -16)] + [('B', v) for v in (0, -1, 2 ** 29 // 256 + 1, 2 ** 62)] + \
             [('n', v) for v in (0, -4)]
FAKE, ODD = C.c_void_p(4096), C.c_void_p(4100)
BIG = 1 << 40


def _calls(lib, s):
    """name -> (pointer names, optional ones, call(pointers, work))"""
    B, N, n = s['B'], s['N'], s['n']
    return {
        'qgx_latent_forward': (['enc_dev', 'x_dev', 'idx_dev', 'eps_dev', 'dec_in_dev', 'stats_dev'], {'enc_dev', 'idx_dev', 'eps_dev'},
                               lambda p, work=(FAKE, BIG): lib.qgx_latent_forward(*p[:4], 1, 2, p[4], p[5], B, N, n, *work, None)),
        'qgx_latent_backward': (['enc_dev', 'eps_dev', 'd_dec_in_dev', 'gout_kl_dev', 'd_enc_dev'], {'eps_dev'},
                                lambda p, work=None: lib.qgx_latent_backward(*p[:2], 1, 2, *p[2:], B, N, None)),
    }


@pytest.mark.parametrize('field,value', BAD_FIELDS)
def test_every_out_of_range_field_is_refused(field, value):
    from pyqg_generative_amd._lib import lib
    s = dict(GOOD, **{field: value})
    if field in ('B', 'N'):
        n = C.c_size_t(0)
        assert lib.qgx_latent_workspace(s['B'], s['N'], C.byref(n)) == -1
        assert field.encode() in lib.qgx_last_error()
    for name, (ptrs, _, call) in _calls(lib, s).items():
        if field == 'n' and name == 'qgx_latent_backward':
            continue                                  # the backward reads no planar set
        assert call([FAKE] * len(ptrs)) == -1, name
        msg = lib.qgx_last_error()
        assert name.encode() in msg and f'{field} = '.encode() in msg, msg


def test_rows_without_idx_null_pointers_misalignment_and_a_short_workspace_are_refused():
    from pyqg_generative_amd._lib import lib
    assert lib.qgx_latent_workspace(3, 16, None) == -1 and b'bytes' in lib.qgx_last_error()
    # n < B is fine with an index vector and refused without one
    ptrs, _, call = _calls(lib, dict(GOOD, n=2))['qgx_latent_forward']
    assert call([None if q == 'idx_dev' else FAKE for q in ptrs]) == -1 and b'n = 2' in lib.qgx_last_error()
    rc, need = _workspace_bytes(GOOD['B'], GOOD['N'])
    assert rc == 0 and need == 256
    for name, (ptrs, optional, call) in _calls(lib, GOOD).items():
        for i, p in enumerate(ptrs):
            for bad in (None, ODD):
                if bad is None and p in optional:
                    continue
                args = [FAKE] * len(ptrs)
                args[i] = bad
                assert call(args) == -1, (name, p)
                msg = lib.qgx_last_error()
                assert name.encode() in msg and p.encode() in msg, msg
    ptrs, _, call = _calls(lib, GOOD)['qgx_latent_forward']
    good = [FAKE] * len(ptrs)
    assert call(good, (None, need)) == -1 and b'work_dev' in lib.qgx_last_error()
    assert call(good, (ODD, need)) == -1 and b'work_dev' in lib.qgx_last_error()
    assert call(good, (FAKE, need - 1)) == -1 and b'work_bytes' in lib.qgx_last_error()
    assert call(good, (FAKE, 0)) == -1


def test_facade_refusals_without_a_device():
    from pyqg_generative_amd.tools import train_ops as T
    x = torch.zeros(3, 2, 16, 16)
    with pytest.raises(ValueError, match='X'):
        T.latent_prior(x, None, 0, 0)                 # a CPU tensor
    with pytest.raises(ValueError, match='X'):
        T.latent_sample(torch.zeros(3, 16, 16, 8), x, None, 0, 0)
    assert set(T.LATENT_LAUNCHES) == {'forward', 'backward', 'prior'}


# ---- TrainableCVAE -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('div', [False, True], ids=['plain', 'div'])
@pytest.mark.parametrize('hidden', [[5, 3], lr.DEFAULT_HIDDEN])
def test_state_dicts_are_the_reference_nets(div, hidden):
    from pyqg_generative_amd.tools.train_CVAE import TrainableCVAE
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN, FluxFormCNN
    net = TrainableCVAE('full_loss', 'adaptive', div, hidden, seed=3)
    want = {'encoder': cr.torch_net(4, 4, lr.DEFAULT_HIDDEN, True, True, torch.float32),
            'decoder': cr.torch_net(4, 4 if div else 2, hidden, True, True, torch.float32),
            'net_mean': cr.torch_net(2, 4 if div else 2, lr.DEFAULT_HIDDEN, True, True, torch.float32)}
    for name, ref in want.items():
        sd = getattr(net, name).state_dict()
        assert list(sd) == list(ref.state_dict()), name
        assert all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in ref.state_dict().items()), name
    assert type(net.encoder) is TrainableAndrewCNN and type(net.decoder) is (FluxFormCNN if div else TrainableAndrewCNN)
    assert net.hidden_channels == list(hidden) and net.encoder.hidden_channels == lr.DEFAULT_HIDDEN
    # the seeds: seed, seed + 1, seed + 2
    assert 'seed + 1' in TrainableCVAE.__doc__ and 'seed + 2' in TrainableCVAE.__doc__
    kind = FluxFormCNN if div else TrainableAndrewCNN
    for name, fresh in (('encoder', TrainableAndrewCNN(4, 4, seed=3)), ('decoder', kind(4, 2, hidden_channels=hidden, seed=4)),
                        ('net_mean', kind(2, 2, seed=5))):
        sd = getattr(net, name).state_dict()
        assert all(torch.equal(sd[k], v) for k, v in fresh.state_dict().items()), name
    assert not hasattr(TrainableCVAE('None', 'fixed', div, hidden), 'net_mean')
    # Adam steps the encoder and the decoder only
    assert len(list(net.trained_parameters())) == len(list(net.encoder.parameters())) + len(list(net.decoder.parameters()))


def test_cvae_refusals():
    from pyqg_generative_amd.tools import train_CVAE, train_CNN
    for reg in ('residual_loss', None, 'full'):
        with pytest.raises(ValueError, match='regression'):
            train_CVAE.fit_cvae(None, None, regression=reg)
    for dv in ('adapt', 0, -0.1, float('inf'), float('nan'), None, True):
        with pytest.raises(ValueError, match='decoder_var'):
            train_CVAE.fit_cvae(None, None, decoder_var=dv)
    for kw, match in ((dict(batch_size=0), 'batch_size'), (dict(num_epochs=0), 'num_epochs'), (dict(learning_rate=float('nan')), 'learning_rate'),
                      (dict(learning_rate=-1.0), 'learning_rate'), (dict(hidden_channels=[300]), 'hidden_channels'),
                      (dict(regression='full_loss', num_epochs_regression=0), 'num_epochs')):
        with pytest.raises(ValueError, match=match):
            train_CVAE.fit_cvae(None, None, **kw)
    assert train_CVAE.check_decoder_var(0.1) == 0.1 and train_CVAE.check_decoder_var('fixed') == 'fixed'
    with pytest.raises(SystemExit):
        train_CVAE.main(['--train', 'a'])
    # train_CNN's command line keeps refusing other models, and TrainableAndrewCNN gains no indexed loss
    with pytest.raises(SystemExit):
        train_CNN.main(['--train', 'a', '--validate', 'b', '--model', 'CVAERegression'])
    assert not hasattr(train_CNN.TrainableAndrewCNN, 'indexed_loss')


# ---- the folder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regression', ['None', 'full_loss'])
def test_cvae_folder_round_trip(tmp_path, regression):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_CNN import channel_scaler
    from pyqg_generative_amd.tools.train_CVAE import TrainableCVAE, write_cvae_folder, loss_to_dataset, KEYS
    from pyqg_generative_amd.tools.simulate import dataset_backend
    hidden, E = [5, 3], 4
    net = TrainableCVAE(regression, 0.1, False, hidden, seed=11)
    rs = np.random.RandomState(5)
    X = rs.randn(6, 2, 16, 16) * np.array([8e-6, 1e-6]).reshape(1, 2, 1, 1) + 1e-7
    Y = rs.randn(6, 2, 16, 16) * np.array([7e-12, 2e-13]).reshape(1, 2, 1, 1)
    xs, ys = channel_scaler(X), channel_scaler(Y)
    optim = {k: list(rs.rand(E)) for k in KEYS}
    score = lambda: dict(L2_mean=rs.rand(), L2_total=rs.rand(), L2_residual=rs.rand(), var_ratio=rs.rand(2))
    log_train, log_test = [score() for _ in range(E)], [score() for _ in range(E)]
    log_test[2].update(L2_total=0.001, L2_residual=0.002)                  # the minimum of L2_loss: epoch 3
    if regression != 'None':
        net.net_mean.log_dict.update(loss=[0.9, 0.5], loss_test=[1.0, 0.625])
    folder = str(tmp_path / 'model')
    assert write_cvae_folder(folder, net, xs, ys, optim, log_train, log_test, verbose=False) == 3
    files = ['decoder.pt', 'encoder.pt', 'model_args.json', 'stats.nc', 'x_scale.json', 'y_scale.json']
    if regression != 'None':
        files = sorted(files + ['net_mean.pt', 'stats_mean.nc'])
    assert sorted(os.listdir(folder)) == files
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='CVAERegression', regression=regression, div=False,
                                                                            decoder_var=0.1, hidden_channels=hidden)
    for name in files:
        if name.endswith('.pt'):
            back = torch.load(os.path.join(folder, name), map_location='cpu', weights_only=True)
            sd = getattr(net, name[:-3]).state_dict()
            assert list(back) == list(sd) and all(torch.equal(back[k], v) for k, v in sd.items())
    # what CVAERegression(folder=...) reads the folder with
    nets, x_std, y_std = weights.load_folder(folder, 'vae', hidden_channels=hidden, regression=regression != 'None')
    assert len(nets) == (2 if regression != 'None' else 1)
    np.testing.assert_array_equal(x_std, xs.std.reshape(-1))
    np.testing.assert_array_equal(y_std, ys.std.reshape(-1))
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    np.testing.assert_array_equal(np.asarray(stats['epoch'].values), np.arange(1, E + 1))
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(stats[k].values), optim[k])
    for k in ('L2_mean', 'L2_total', 'L2_residual'):
        np.testing.assert_array_equal(np.asarray(stats[k].values), [e[k] for e in log_train])
        np.testing.assert_array_equal(np.asarray(stats[k + '_test'].values), [e[k] for e in log_test])
    # the test log's var_ratio is not renamed, so it replaces the train log's
    assert np.asarray(stats['var_ratio'].values).shape == (E, 2) and 'var_ratio_test' not in stats
    np.testing.assert_array_equal(np.asarray(stats['var_ratio'].values), [e['var_ratio'] for e in log_test])
    L2 = np.asarray(stats['L2_loss'].values)
    np.testing.assert_array_equal(L2, np.asarray(stats['L2_total_test'].values) + np.asarray(stats['L2_residual_test'].values))
    assert int(np.asarray(stats['Epoch_opt'].values)) == 3 == int(np.argmin(L2)) + 1 and np.asarray(stats['Epoch_opt'].values).shape == ()
    if regression != 'None':
        mean = dataset_backend().open_dataset(os.path.join(folder, 'stats_mean.nc'))
        np.testing.assert_array_equal(np.asarray(mean['loss'].values), [0.9, 0.5])
    with pytest.raises(ValueError, match='epochs'):
        loss_to_dataset(optim, log_train[:-1], log_test)
