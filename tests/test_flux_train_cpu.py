"""CPU: the training of flux-form nets (include/qgx_flux_train.h, tools/train_CNN.py::FluxFormCNN) — the adjoint of the spectral
divergence against torch autograd of the reference's rfftn form, the dot-product identity, the sensitivity of white cotangents to
the Nyquist rule, the declarations against the bindings, every refusal before any device call, and the host side: FluxFormCNN's
state dict and seeds, the folder writer with div=True."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import div_restatement as dr
import flux_train_restatement as fr


# ---- the adjoint -------------------------------------------------------------------------------------------------------------
def _rel(a, truth):
    return float(np.abs(np.asarray(a, np.float64) - truth).max() / np.abs(truth).max())


@pytest.mark.parametrize('N', fr.GRIDS)
def test_adjoint_is_float64_autograd_of_the_rfftn_form(N):
    B = 3
    F, g = fr.white(B, 4, N, 100 + N), fr.white(B, 2, N, 200 + N)
    y, want = fr.autograd_pair(F, g, torch.float64)
    assert _rel(dr.divergence_plane(F), y) <= 1e-12
    got = fr.divergence_adjoint(g)
    assert got.shape == (B, 4, N, N) and _rel(got, want) <= 1e-12
    assert _rel(fr.divergence_adjoint_per_layer(g), want) <= 1e-12
    # Hx and Hy vanish at (0, 0): every gradient plane has zero mean
    assert np.abs(got.mean(axis=(-2, -1))).max() <= 1e-12 * np.abs(got).max()


@pytest.mark.parametrize('N', fr.GRIDS)
def test_dot_product_identity(N):
    F, g = fr.white(3, 4, N, 300 + N).astype(np.float64), fr.white(3, 2, N, 400 + N).astype(np.float64)
    DF, DTg = dr.divergence_plane(F), fr.divergence_adjoint(g)
    lhs, rhs = float((DF * g).sum()), float((F * DTg).sum())
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(DF) * np.linalg.norm(g)
    assert np.linalg.norm(DF) > 0 and np.linalg.norm(DTg) > 0


@pytest.mark.parametrize('N', fr.GRIDS)
@pytest.mark.parametrize('rule', ['naive_row', 'zero_row'])
def test_white_cotangents_are_sensitive_to_the_nyquist_rule(N, rule):
    g = fr.white(3, 2, N, 200 + N)
    want = fr.divergence_adjoint(g)
    dev = _rel(fr.divergence_adjoint(g, rule), want)
    assert dev > 0.05, (N, rule, dev)


def test_restated_net_is_the_plain_net_plus_the_divergence():
    net = fr.flux_torch_net(2, [5, 3], True, True, torch.float64)
    plain = cr.torch_net(2, 4, [5, 3], True, True, torch.float64, net.state_dict())
    assert list(net.state_dict()) == list(plain.state_dict())
    x = torch.randn(2, 2, 16, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    net.eval(), plain.eval()
    with torch.no_grad():
        y = net(x)
        assert y.shape == (2, 2, 16, 16)
        want = 10000. * dr.divergence_rfftn(plain(x).numpy(), 'float64')
        assert np.array_equal(y.numpy(), want)
        assert torch.equal(net.compute_loss(x, x)['loss'], torch.nn.functional.mse_loss(y, x))


# ---- declarations and bindings -----------------------------------------------------------------------------------------------
NAMES = ['qgx_fluxdiv_backward', 'qgx_fluxdiv_forward']


def test_header_declares_what_flux_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_flux_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_flux_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.FLUX_TRAIN_SYMBOLS) == NAMES
    for name, _, args in _lib.FLUX_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    assert re.search(r'QGX_FLUX_PLANAR = 0, QGX_FLUX_ENGINE = 1', code) and (_lib.FLUX_PLANAR, _lib.FLUX_ENGINE) == (0, 1)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
        assert getattr(_lib.lib, name).argtypes is not None                 # bound by the loop of _load
    others = (_lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS + _lib.CONV_TRAIN_SYMBOLS
              + _lib.HEAD_TRAIN_SYMBOLS)
    assert not {n for n, _, _ in _lib.FLUX_TRAIN_SYMBOLS} & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'fluxdiv_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    hdrs = re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_flux_train.h' in hdrs and 'fluxdiv_core.hpp' in hdrs
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'FluxFormCNN' in open(os.path.join(ROOT, doc)).read()


# ---- refusals, each without a device -----------------------------------------------------------------------------------------
FAKE, ODD = C.c_void_p(4096), C.c_void_p(4100)
CALLS = {'qgx_fluxdiv_forward': ('F_dev', 'y_dev'), 'qgx_fluxdiv_backward': ('dy_dev', 'dF_dev')}


def _call(name, a=FAKE, b=FAKE, B=3, N=16, layout=1):
    from pyqg_generative_amd._lib import lib
    rc = getattr(lib, name)(a, b, B, N, layout, None)
    return rc, lib.qgx_last_error()


@pytest.mark.parametrize('name', sorted(CALLS))
def test_every_refusal(name):
    first, second = CALLS[name]
    for layout in (0, 1):
        for bad in (None, ODD):
            rc, msg = _call(name, a=bad, layout=layout)
            assert rc == -1 and name.encode() in msg and first.encode() in msg, msg
            rc, msg = _call(name, b=bad, layout=layout)
            assert rc == -1 and name.encode() in msg and second.encode() in msg, msg
        for B in (0, -1, 2 ** 30, 2 ** 31, 2 ** 62):
            rc, msg = _call(name, B=B, layout=layout)
            assert rc == -1 and name.encode() in msg and f'B = {B}'.encode() in msg, msg
        for N in (0, 8, 17, 24, 80, 192, 256, -16):
            rc, msg = _call(name, N=N, layout=layout)
            assert rc == -1 and name.encode() in msg and f'N = {N}'.encode() in msg, msg
    for layout in (-1, 2, 7):
        rc, msg = _call(name, layout=layout)
        assert rc == -1 and name.encode() in msg and f'layout = {layout}'.encode() in msg, msg
    assert 2 * (2 ** 30 - 1) <= 2 ** 31 - 1 < 2 * 2 ** 30          # the largest B admitted is 2^30 - 1


# ---- FluxFormCNN on the host -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden', [[8], [5, 3], [128, 64, 32, 32, 32, 32, 32]])
@pytest.mark.parametrize('batch_norm,bias', [(True, True), (False, True), (True, False)])
def test_state_dict_is_the_reference_div_nets(hidden, batch_norm, bias):
    from pyqg_generative_amd.tools.train_CNN import FluxFormCNN
    net = FluxFormCNN(2, 2, hidden, batch_norm=batch_norm, bias=bias, seed=3)
    sd = net.state_dict()
    ref = fr.flux_torch_net(2, hidden, batch_norm, bias, torch.float32).state_dict()
    assert list(sd) == list(ref)
    assert all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in ref.items())
    last = [k for k in sd if k.endswith('.weight') and sd[k].dim() == 4][-1]
    assert tuple(sd[last].shape) == (4, hidden[-1], 3, 3) and net.n_out == 2


def test_seeds_reproduce_and_leave_the_global_stream_alone():
    from pyqg_generative_amd.tools.train_CNN import FluxFormCNN, TrainableAndrewCNN
    assert tuple(FluxFormCNN(2, 2, [8]).state_dict()['conv.3.weight'].shape) == (4, 8, 3, 3)       # conv, ReLU, BatchNorm, conv
    torch.manual_seed(123)
    before = torch.random.get_rng_state()
    a, b, c = (FluxFormCNN(2, 2, [5, 3], seed=s).state_dict() for s in (7, 7, 8))
    assert torch.equal(torch.random.get_rng_state(), before)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a['conv.0.weight'], c['conv.0.weight'])
    # the parent's rule: the layers are drawn in order under the seed, so all layers before the last are the plain net's
    plain = TrainableAndrewCNN(2, 2, [5, 3], seed=7).state_dict()
    assert list(plain) == list(a)
    assert all(torch.equal(a[k], plain[k]) for k in a if not k.startswith('conv.6.'))
    assert tuple(plain['conv.6.weight'].shape) == (2, 3, 3, 3) and tuple(a['conv.6.weight'].shape) == (4, 3, 3, 3)


def test_flux_form_refusals():
    from pyqg_generative_amd.tools import train_CNN
    with pytest.raises(NotImplementedError, match='FluxFormCNN'):
        train_CNN.TrainableAndrewCNN(2, 2, [8], div=True)
    with pytest.raises(NotImplementedError, match='div'):
        train_CNN.TrainableAndrewCNN(2, 2, [8], div=True)
    with pytest.raises(NotImplementedError, match='final_activation'):
        train_CNN.FluxFormCNN(2, 2, [8], final_activation='nn.Tanh()')
    with pytest.raises(ValueError, match='n_out'):
        train_CNN.FluxFormCNN(2, 3, [8])
    with pytest.raises(ValueError, match='hidden_channels'):
        train_CNN.FluxFormCNN(2, 2, [300])
    with pytest.raises(ValueError, match='batch_size'):
        train_CNN.fit_ols(None, None, div=True, batch_size=0)
    assert 'div=True' in train_CNN.fit_ols.__doc__
    # the fused-head nets stay as they were: MeanVarModel has no div
    assert not train_CNN.FusedHeadCNN.FLUX_FORM and not hasattr(train_CNN.FluxFormCNN, 'indexed_loss')


def test_ops_refuse_what_is_not_the_engine_layout():
    from pyqg_generative_amd.tools import train_ops as T
    assert sorted(T.FLUX_LAUNCHES) == ['backward', 'forward']
    with pytest.raises(ValueError, match='engine layout'):
        T.flux_divergence(torch.zeros(2, 16, 16, 8))                  # not on the device
    with pytest.raises(ValueError, match='engine layout'):
        T.flux_divergence(torch.zeros(2, 4, 16, 16))


# ---- the folder --------------------------------------------------------------------------------------------------------------
def test_model_folder_round_trip_with_div(tmp_path):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_CNN import FluxFormCNN, write_model_folder, channel_scaler
    hidden = [5, 3]
    net = FluxFormCNN(2, 2, hidden, seed=11)
    rs = np.random.RandomState(5)
    X = rs.randn(6, 2, 16, 16) * np.array([8e-6, 1e-6]).reshape(1, 2, 1, 1) + 1e-7
    Y = rs.randn(6, 2, 16, 16) * np.array([7e-12, 2e-13]).reshape(1, 2, 1, 1)
    xs, ys = channel_scaler(X), channel_scaler(Y)
    args = dict(div=True, batch_norm=True, bias=True, final_activation='None', hidden_channels=hidden)
    log = {'loss': [0.9, 0.5, 0.25], 'loss_test': [1.0, 0.625, 0.375]}
    folder = str(tmp_path / 'model')
    write_model_folder(folder, net.state_dict(), xs, ys, args, log)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'stats.nc', 'x_scale.json', 'y_scale.json']
    back = json.load(open(os.path.join(folder, 'model_args.json')))
    assert back == dict(model='OLSModel', **args) and back['div'] is True
    sd = torch.load(os.path.join(folder, 'net.pt'), map_location='cpu', weights_only=True)
    assert list(sd) == list(net.state_dict()) and all(torch.equal(sd[k], v) for k, v in net.state_dict().items())
    # the four-channel last layer as the inference side packs it
    got = weights.net_from_state_dict_arch(sd, 2, hidden, True, True, True)
    assert got['conv_w'][-1].shape == (4, 3, 3, 3)
    np.testing.assert_array_equal(got['conv_w'][-1], net.state_dict()['conv.6.weight'].numpy())
