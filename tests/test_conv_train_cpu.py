"""CPU: the differentiable circular convolution of include/qgx_conv_train.h — the restatement against torch autograd, the
declarations against the bindings, every refusal before any device call — and the host side of tools/train_CNN.py: the
state dict of TrainableAndrewCNN against the reference's, the learning-rate schedule, the model-folder writer."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import train_plan_restatement as tp

SHAPES = [(2, 5, 5), (5, 2, 3), (8, 32, 3), (33, 7, 3)]


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout,k', SHAPES)
def test_restatement_is_torch_autograd(cin, cout, k):
    import torch.nn.functional as F
    B, N, p = 2, 8, k // 2
    x, w, b, dy = cr.case_data(cin, cout, k, B, N, 100 + cin, integer=False)
    xt = torch.tensor(cr.from_layout(x, cin), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(xt, (p, p, p, p), mode='circular'), wt, bt)
    y.backward(torch.tensor(cr.from_layout(dy, cout), dtype=torch.float64))
    got_y, got_dx = cr.forward(x, w, b), cr.backward_data(dy, w)
    got_dw, got_db = cr.backward_weight(x, dy, cin, cout, k)
    tol = dict(rtol=0, atol=1e-12 * cin * cout * k * k)
    np.testing.assert_allclose(cr.from_layout(got_y, cout), y.detach().numpy(), **tol)
    np.testing.assert_allclose(cr.from_layout(got_dx, cin), xt.grad.numpy(), **tol)
    np.testing.assert_allclose(got_dw, wt.grad.numpy(), rtol=0, atol=1e-12 * B * N * N)
    np.testing.assert_allclose(got_db, bt.grad.numpy(), rtol=0, atol=1e-12 * B * N * N)
    # the layout: C8 channels per pixel, the pad channels zero
    assert got_y.shape == (B, N, N, cr.c8(cout)) and got_dx.shape == (B, N, N, cr.c8(cin))
    assert not got_y[..., cout:].any() and not got_dx[..., cin:].any()
    # no bias: the convolution alone
    np.testing.assert_allclose(cr.forward(x, w), got_y - cr.to_layout(np.broadcast_to(b.reshape(1, -1, 1, 1).astype(np.float64), (B, cout, N, N))), **tol)


@pytest.mark.parametrize('cin,cout,k', SHAPES)
def test_data_gradient_is_the_forward_with_flipped_transposed_weights(cin, cout, k):
    x, w, b, dy = cr.case_data(cin, cout, k, 2, 8, 200 + cin, integer=True)
    wf = cr.flip_transpose(w)
    assert wf.shape == (cin, cout, k, k) and wf[1 % cin, 1 % cout, 0, k - 1] == w[1 % cout, 1 % cin, k - 1, 0]
    # integers: both sides are exact
    np.testing.assert_array_equal(cr.backward_data(dy, w), cr.forward(dy, wf))


def test_integer_cases_are_exact_in_float32():
    """every product and partial sum of the GPU test's integer cases stays below 2^24 in magnitude"""
    for (cin, cout, k), (B, N) in [((256, 1, 3), (3, 16)), ((70, 40, 5), (2, 48)), ((1, 256, 3), (34, 16)), ((40, 70, 5), (3, 16))]:
        assert 9 * cin * k * k + 3 < 2 ** 24 and 9 * cout * k * k < 2 ** 24 and 9 * B * N * N < 2 ** 24
    for cin, cout, k, B, N in _gpu_cases():
        assert 9 * cin * k * k + 3 < 2 ** 24 and 9 * cout * k * k < 2 ** 24 and 9 * B * N * N < 2 ** 24


# ---- the weight gradient's plan --------------------------------------------------------------------------------------
def _gpu_cases():
    """every case of tests/test_gpu_conv_train.py, old and new (the module asks for no device when it is imported)"""
    import test_gpu_conv_train as g
    return list(g.CASES)


def _library_bytes(cin, cout, k, B, N):
    from pyqg_generative_amd._lib import lib
    n = C.c_size_t(0)
    assert lib.qgx_conv2d_workspace(B, N, cin, cout, k, C.byref(n)) == 0
    return n.value


def test_restated_plan_gives_the_librarys_workspace_size_for_every_gpu_case():
    """the workspace holds S x pairs x k^2 x 1024 floats of partial sums and nb x cout8 of bias block sums: its size, which the
    library computes without a device, pins the restated plan's S and nb (tests/train_plan_restatement.py)"""
    cases = _gpu_cases()
    assert len(cases) >= 27 and set(tp.CONV_REGIMES) <= set(cases)
    for case in cases:
        cin, cout, k, B, N = case
        assert _library_bytes(*case) == tp.conv_workspace_bytes(B, N, cin, cout, k), case


def test_restated_plan_gives_the_librarys_workspace_size_on_a_sweep():
    n = 0
    for N in tp.GRIDS:
        for k in (3, 5):
            for B in (1, 2, 3, 9, 23, 64, 130):
                for cin in (1, 8, 33, 70, 256):
                    for cout in (1, 8, 33, 70, 256):
                        assert _library_bytes(cin, cout, k, B, N) == tp.conv_workspace_bytes(B, N, cin, cout, k), (cin, cout, k, B, N)
                        n += 1
    assert n == 6 * 2 * 7 * 25


def test_declared_regimes_hold_in_the_restated_plan():
    """each GPU case that is there for a regime is in it; and the plan's own invariants over the sweep: every unit in exactly
    one share, every pixel in exactly one block, the patches within the LDS a workgroup may ask for"""
    for case, regime in tp.CONV_REGIMES.items():
        cin, cout, k, B, N = case
        plan = tp.wgrad_plan(B, N, cin, cout, k)
        assert {key: plan[key] for key in regime} == regime, case
    for N in tp.GRIDS:
        for k in (3, 5):
            for B in (1, 2, 3, 9, 23, 64, 130):
                for c in (1, 33, 256):
                    p = tp.wgrad_plan(B, N, c, c, k)
                    assert N % p['R'] == 0 and p['U'] * p['R'] == B * N and p['lds'] <= 160 * 1024
                    assert (p['S'] - 1) * p['ups'] < p['U'] <= p['S'] * p['ups'] and 1 <= p['last_units'] <= p['ups']
                    assert (p['nb'] - 1) * p['ppb'] < B * N * N <= p['nb'] * p['ppb'] and p['nb'] <= 256 and p['ppb'] >= 64
                    assert 1 <= p['G'] and p['G'] * cr.c8(c) <= 256
    # the shipped shape at batch 64 on 64 x 64 runs deep in the regime the new cases enter
    p = tp.wgrad_plan(64, 64, 128, 64, 3)
    assert (p['R'], p['ups'], p['ppb']) == (2, 32, 1024)


# ---- declarations and bindings ---------------------------------------------------------------------------------------
def test_header_declares_what_conv_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_conv_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_conv_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.CONV_TRAIN_SYMBOLS)
    assert declared == ['qgx_conv2d_backward_data', 'qgx_conv2d_backward_weight', 'qgx_conv2d_forward', 'qgx_conv2d_workspace']
    for name, _, args in _lib.CONV_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    others = _lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS
    assert not {n for n, _, _ in _lib.CONV_TRAIN_SYMBOLS} & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'conv_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_conv_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'fit_ols' in open(os.path.join(ROOT, doc)).read()


GOOD = dict(B=3, N=16, cin=5, cout=7, k=3)
BAD_FIELDS = [('N', v) for v in (0, 8, 17, 24, 192, 256, -16)] + [('B', v) for v in (0, -1, 2 ** 29 // 256 + 1, 2 ** 62)] + \
             [('cin', v) for v in (0, 257, -3)] + [('cout', v) for v in (0, 257, -3)] + [('k', v) for v in (0, 1, 2, 4, 7, -3)]


def _workspace_bytes(**kw):
    from pyqg_generative_amd._lib import lib
    s = dict(GOOD, **kw)
    n = C.c_size_t(0)
    rc = lib.qgx_conv2d_workspace(s['B'], s['N'], s['cin'], s['cout'], s['k'], C.byref(n))
    return rc, n.value


def test_workspace_is_a_function_of_the_shape_alone():
    rc, n = _workspace_bytes()
    assert rc == 0 and n > 0 and n % 16 == 0
    assert _workspace_bytes() == (0, n)
    # the workload's widest layer: partial sums of some tens of MB, not more
    rc, big = _workspace_bytes(B=64, N=64, cin=128, cout=64, k=5)
    assert rc == 0 and 2 ** 20 < big < 2 ** 27
    # the largest admitted grid and widths
    assert _workspace_bytes(B=1, N=128, cin=256, cout=256, k=5)[0] == 0


@pytest.mark.parametrize('field,value', BAD_FIELDS)
def test_every_out_of_range_field_is_refused(field, value):
    from pyqg_generative_amd._lib import lib
    fake = C.c_void_p(4096)       # never dereferenced: every call below must be refused first
    s = dict(GOOD, **{field: value})
    shape = (s['B'], s['N'], s['cin'], s['cout'], s['k'])
    n = C.c_size_t(0)
    assert lib.qgx_conv2d_workspace(*shape, C.byref(n)) == -1
    assert field.encode() in lib.qgx_last_error()
    big = 1 << 40
    for rc in (lib.qgx_conv2d_forward(fake, fake, fake, fake, *shape, fake, big, None),
               lib.qgx_conv2d_backward_data(fake, fake, fake, *shape, fake, big, None),
               lib.qgx_conv2d_backward_weight(fake, fake, fake, fake, *shape, fake, big, None)):
        assert rc == -1
        assert field.encode() in lib.qgx_last_error()


def test_null_pointers_misalignment_and_a_short_workspace_are_refused():
    from pyqg_generative_amd._lib import lib
    fake, odd = C.c_void_p(4096), C.c_void_p(4100)
    shape = tuple(GOOD[f] for f in ('B', 'N', 'cin', 'cout', 'k'))
    assert lib.qgx_conv2d_workspace(*shape, None) == -1
    rc, need = _workspace_bytes()
    calls = {
        'qgx_conv2d_forward': (lib.qgx_conv2d_forward, ['x_dev', 'w_dev', 'bias_dev', 'y_dev'], {'bias_dev'}),
        'qgx_conv2d_backward_data': (lib.qgx_conv2d_backward_data, ['dy_dev', 'w_dev', 'dx_dev'], set()),
        'qgx_conv2d_backward_weight': (lib.qgx_conv2d_backward_weight, ['x_dev', 'dy_dev', 'dw_dev', 'db_dev'], {'db_dev'}),
    }
    for name, (fn, ptrs, optional) in calls.items():
        for i, p in enumerate(ptrs):
            for bad in (None, odd):
                if bad is None and p in optional:
                    continue
                args = [fake] * len(ptrs)
                args[i] = bad
                assert fn(*args, *shape, fake, need, None) == -1, (name, p)
                msg = lib.qgx_last_error()
                assert name.encode() in msg and p.encode() in msg, msg
        good = [fake] * len(ptrs)
        assert fn(*good, *shape, None, need, None) == -1 and b'work_dev' in lib.qgx_last_error()
        assert fn(*good, *shape, odd, need, None) == -1 and b'work_dev' in lib.qgx_last_error()
        assert fn(*good, *shape, fake, need - 1, None) == -1 and b'work_bytes' in lib.qgx_last_error()
        assert fn(*good, *shape, fake, 0, None) == -1


# ---- TrainableAndrewCNN ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('batch_norm', [True, False])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('hidden', [[5, 3], [128, 64, 32, 32, 32, 32, 32], [9]])
def test_state_dict_is_the_reference_nets(batch_norm, bias, hidden):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN
    net = TrainableAndrewCNN(2, 2, hidden, batch_norm=batch_norm, bias=bias, seed=3)
    sd = net.state_dict()
    # tests/arch_restatement.py's net: the dict of weights.synthetic_arch, whose state dict is state_dict_from_net's
    want = weights.state_dict_from_net(weights.synthetic_arch(2, hidden, batch_norm, bias))
    have = {k: tuple(v.shape) for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    assert have == {k: tuple(v.shape) for k, v in want.items()}
    assert have == weights.arch_shapes(2, hidden, batch_norm, bias)
    # ... and the reference module's own keys, counters included, in its order
    assert list(sd) == list(cr.torch_net(2, 2, hidden, batch_norm, bias, torch.float32).state_dict())
    tracked = [k for k in sd if k.endswith('num_batches_tracked')]
    assert len(tracked) == (len(hidden) if batch_norm else 0) and all(sd[k].dtype == torch.int64 for k in tracked)
    # the loaders take it unchanged
    back = weights.net_from_state_dict_arch(sd, 2, hidden, batch_norm, bias, False)
    np.testing.assert_array_equal(back['conv_w'][0], sd['conv.0.weight'].numpy())
    # torch's defaults under the seed, drawn on the CPU: reproducible, and the global stream is left alone
    state = torch.random.get_rng_state()
    again = TrainableAndrewCNN(2, 2, hidden, batch_norm=batch_norm, bias=bias, seed=3).state_dict()
    assert torch.equal(state, torch.random.get_rng_state())
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    other = TrainableAndrewCNN(2, 2, hidden, batch_norm=batch_norm, bias=bias, seed=4).state_dict()
    assert not torch.equal(sd['conv.0.weight'], other['conv.0.weight'])
    w0 = sd['conv.0.weight']
    assert float(w0.abs().max()) <= 1 / np.sqrt(2 * 25) + 1e-7 and all(p.device.type == 'cpu' for p in sd.values())
    if batch_norm:
        assert torch.equal(sd['conv.2.weight'], torch.ones(hidden[0])) and torch.equal(sd['conv.2.running_var'], torch.ones(hidden[0]))


def test_what_has_no_backward_yet_is_refused():
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN, fit_ols
    with pytest.raises(NotImplementedError, match='div'):
        TrainableAndrewCNN(2, 2, [8], div=True)
    with pytest.raises(NotImplementedError, match='final_activation'):
        TrainableAndrewCNN(2, 2, [8], final_activation='nn.Tanh()')
    with pytest.raises(ValueError, match='hidden_channels'):
        TrainableAndrewCNN(2, 2, [300])
    for kw, match in ((dict(batch_size=0), 'batch_size'), (dict(num_epochs=0), 'num_epochs'), (dict(learning_rate=float('nan')), 'learning_rate')):
        with pytest.raises(ValueError, match=match):
            fit_ols(None, None, **kw)


def test_ols_model_still_needs_a_trained_folder(tmp_path):
    from pyqg_generative_amd.models import OLSModel
    with pytest.raises(FileNotFoundError, match='net.pt'):
        OLSModel(folder=str(tmp_path))


# ---- schedule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 2, 3, 4, 5, 6, 7, 8, 9, 50])
def test_learning_rates_are_the_references_multisteplr(E):
    from pyqg_generative_amd.tools import train_CNN, train_common
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    want = []
    for _ in range(E):
        want.append(opt.param_groups[0]['lr'])
        opt.step()
        sched.step()
    assert train_common.learning_rates(E, 1e-3) == want
    assert cr.lr_sequence(E, 1e-3) == pytest.approx(want, rel=1e-12)
    if E == 50:
        assert [want[0], want[24], want[25], want[37], want[43]] == pytest.approx([1e-3, 1e-3, 1e-4, 1e-5, 1e-6], rel=1e-12)
    # train() builds exactly this scheduler: its source names the reference's milestones
    import inspect
    src = inspect.getsource(train_CNN.train)
    assert 'MultiStepLR' in src and 'int(E / 2), int(E * 3 / 4), int(E * 7 / 8)' in src and 'gamma=0.1' in src and 'optim.Adam' in src


# ---- the folder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden,batch_norm,bias', [([5, 3], True, True), ([9], False, True), ([4, 4, 4], True, False)])
def test_model_folder_round_trip(tmp_path, hidden, batch_norm, bias):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_CNN import TrainableAndrewCNN, write_model_folder, channel_scaler
    from pyqg_generative_amd.tools.simulate import dataset_backend
    net = TrainableAndrewCNN(2, 2, hidden, batch_norm=batch_norm, bias=bias, seed=11)
    rs = np.random.RandomState(5)
    X = rs.randn(6, 2, 16, 16) * np.array([8e-6, 1e-6]).reshape(1, 2, 1, 1) + 1e-7
    Y = rs.randn(6, 2, 16, 16) * np.array([7e-12, 2e-13]).reshape(1, 2, 1, 1)
    xs, ys = channel_scaler(X), channel_scaler(Y)
    np.testing.assert_array_equal(xs.std.reshape(-1), np.array([X[:, c].std() for c in range(2)]).astype('float32'))
    np.testing.assert_array_equal(xs.mean.reshape(-1), np.array([X[:, c].mean() for c in range(2)]).astype('float32'))
    assert xs.std.shape == (1, 2, 1, 1)
    args = dict(div=False, batch_norm=batch_norm, bias=bias, final_activation='None', hidden_channels=hidden)
    log = {'loss': [0.9, 0.5, 0.25], 'loss_test': [1.0, 0.625, 0.375]}
    folder = str(tmp_path / 'model')
    write_model_folder(folder, net.state_dict(), xs, ys, args, log)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'stats.nc', 'x_scale.json', 'y_scale.json']
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='OLSModel', **args)
    back = torch.load(os.path.join(folder, 'net.pt'), map_location='cpu', weights_only=True)
    assert list(back) == list(net.state_dict()) and all(torch.equal(back[k], v) for k, v in net.state_dict().items())
    nets, x_std, y_std = weights.load_folder(folder, 'ols', hidden_channels=hidden, batch_norm=batch_norm, bias=bias)
    np.testing.assert_array_equal(x_std, xs.std.reshape(-1))
    np.testing.assert_array_equal(y_std, ys.std.reshape(-1))
    want = weights.net_from_state_dict_arch(net.state_dict(), 2, hidden, batch_norm, bias, False)
    for key in ('conv_w', 'conv_b', 'bn_g', 'bn_b', 'bn_m', 'bn_v'):
        assert len(nets[0][key]) == len(want[key])
        for a, b in zip(nets[0][key], want[key]):
            np.testing.assert_array_equal(a, b)
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    np.testing.assert_array_equal(np.asarray(stats['epoch'].values), [1, 2, 3])
    for k, v in log.items():
        assert tuple(stats[k].dims) == ('epoch',)
        np.testing.assert_array_equal(np.asarray(stats[k].values), v)
    # a second write replaces the files
    write_model_folder(folder, net.state_dict(), xs, ys, args, {k: v[:2] for k, v in log.items()})
    assert dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))['loss'].shape == (2,)
