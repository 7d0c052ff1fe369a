"""CPU: the batch gather and the loss head of include/qgx_head_train.h — the restatement against torch autograd, the
declarations against the bindings, every refusal before any device call — and the host side of MeanVarModel's training in
tools/train_CNN.py: FusedHeadCNN's state dict, the folder writer, fit_meanvar's refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import head_restatement as hr
import train_plan_restatement as tp

EDGE = np.array([20.0, np.nextafter(np.float32(20), np.float32(21)), 30.0, -30.0, -100.0, 1e4, -1e4, 0.0, 19.999998], np.float32)


def _case(seed, B=3, N=8, C=2, n=5):
    y, _, t = hr.case_data(B, N, C, n, seed, integer=False)
    flat = y[..., :C].reshape(-1)
    flat[:len(EDGE)] = EDGE                      # a view of y: the edge values are in the first pixels
    y[..., :C] = flat.reshape(y[..., :C].shape)
    return y, t


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['mse', 'softplus_mse'])
@pytest.mark.parametrize('idx', [None, [4, 0, 4]], ids=['rows', 'idx'])
def test_restatement_is_torch_autograd(mode, idx):
    import torch.nn.functional as F
    B, N, Cn = 3, 8, 2
    y, t = _case(7)
    assert y[0, 0, 0, 0] == 20 and y[0, 0, 0, 1] > 20 and float(np.abs(y).max()) == 1e4
    yt = torch.tensor(cr.from_layout(y, Cn), dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.float64)[hr.rows(idx, B)]
    h = yt if mode == 'mse' else F.softplus(yt)
    loss = F.mse_loss(h, tt)
    gout = 0.375
    (loss * gout).backward()
    got_loss = hr.head_loss(y, t, idx, mode)
    assert np.isfinite(got_loss) and got_loss == pytest.approx(float(loss.detach()), rel=1e-13)
    # the gradient: torch's, but for the float32 rounding of the scale, which the restatement states on its own
    s = hr.scale(gout, B, Cn, N)
    assert s == np.float32(gout * 2.0 / (B * Cn * N * N)) and s.dtype == np.float32
    got = hr.head_grad(y, t, idx, mode, gout)
    assert got.shape == (B, N, N, 8) and not got[..., Cn:].any() and np.isfinite(got).all()
    want = yt.grad.numpy() * (float(s) / (gout * 2.0 / (B * Cn * N * N)))
    np.testing.assert_allclose(cr.from_layout(got, Cn), want, rtol=1e-13, atol=1e-300)
    # the planar outputs
    np.testing.assert_allclose(hr.head_apply(y, None, None, mode, Cn), h.detach().numpy(), rtol=1e-15)
    np.testing.assert_allclose(hr.head_apply(y, t, idx, mode, Cn), ((tt - h) ** 2).detach().numpy(), rtol=1e-13)
    assert np.isfinite(hr.head_apply(y, t, idx, mode, Cn)).all()
    if mode == 'softplus_mse':
        hv = hr.head(EDGE, mode)
        assert hv[0] == pytest.approx(20 + np.log1p(np.exp(-20.0)), rel=1e-15) and hv[1] == EDGE[1] and hv[5] == 1e4
        assert hv[4] == pytest.approx(np.exp(-100.0), rel=1e-12) and hv[6] == 0
        sv = hr.slope(EDGE, mode)
        assert sv[1] == 1 and sv[5] == 1 and sv[6] == 0 and 0 < sv[0] < 1


def test_gather_restatement_is_the_index_and_the_layout():
    _, src, _ = hr.case_data(2, 8, 3, 5, 9, integer=True)
    idx = [4, 1, 4, 0]
    out = hr.batch_gather(src, idx)
    assert out.shape == (4, 8, 8, 8) and out.dtype == np.float32 and not out[..., 3:].any()
    np.testing.assert_array_equal(cr.from_layout(out, 3), src[idx])
    np.testing.assert_array_equal(hr.batch_gather(src), cr.to_layout(src))


def test_integer_cases_are_exact():
    """every difference of the GPU test's integer cases is below 2^24 (float32) and every sum of squares below 2^53"""
    assert 16 < 2 ** 24 and 16 * 16 * 8 * 128 * 128 * 5 < 2 ** 53
    assert all(16 * 16 * Cn * N * N * B < 2 ** 53 for B, N, Cn in _gpu_shapes())
    # a float32 scale times an integer difference of 5 bits is exact in float64
    assert 24 + 5 <= 53


# ---- the loss's plan ---------------------------------------------------------------------------------------------------------
def _gpu_shapes():
    """every shape of tests/test_gpu_head_train.py, old and new (the module asks for no device when it is imported)"""
    import test_gpu_head_train as g
    return list(g.SHAPES)


def test_restated_plan_gives_the_librarys_workspace_size():
    """The workspace is one float64 per partial, rounded up to 256 bytes, so its size resolves the number of partials nb ONLY
    TO 32: it tells 257 partials from 256, and 513 from 512, but not 320 from 300.  Within that resolution the restated plan
    (tests/train_plan_restatement.py) is pinned to the library, for every GPU shape and on a sweep; the sweep's B are chosen
    with B N^2 / 256 on both sides of multiples of 32 and of the cap of 1024 partials."""
    shapes = _gpu_shapes()
    assert len(shapes) >= 11 and set(tp.HEAD_REGIMES) <= set(shapes)
    grids = [(B, N) for B, N, _ in shapes]
    grids += [(B, N) for N in tp.GRIDS for B in (1, 2, 3, 9, 23, 64, 130, 256, 257, 1023, 1024, 1025, 2 ** 29 // (N * N))]
    grids += [(B, N) for N in tp.GRIDS for q in (32, 256, 1024) for B in (q * 256 // (N * N), q * 256 // (N * N) + 1) if B >= 1]
    for B, N in grids:
        rc, n = _workspace_bytes(B, N)
        assert rc == 0 and n == tp.head_workspace_bytes(B, N), (B, N)


def test_declared_regimes_hold_in_the_restated_plan():
    for (B, N, Cn), regime in tp.HEAD_REGIMES.items():
        plan = tp.head_plan(B, N)
        assert {key: plan[key] for key in regime} == regime, (B, N, Cn)
    # the plan's own invariants: every pixel in exactly one block, blocks whole multiples of the 256 threads
    for N in tp.GRIDS:
        for B in (1, 2, 3, 9, 23, 64, 130, 257, 1025, 5000):
            p = tp.head_plan(B, N)
            assert (p['nb'] - 1) * p['ppb'] < B * N * N <= p['nb'] * p['ppb'] and p['nb'] <= 1024 and p['ppb'] % 256 == 0
    # fit_meanvar's batch of 64 at 64 x 64 sits on the boundary: one more image and k_head_loss takes a second pass
    assert tp.head_plan(64, 64)['loss_passes'] == 1 and tp.head_plan(65, 64)['loss_passes'] == 2


def test_var_net_is_the_reference_net_plus_softplus():
    net = hr.var_net(2, 2, [5, 3], torch.float64)
    plain = cr.torch_net(2, 2, [5, 3], True, True, torch.float64, net.state_dict())
    assert list(net.state_dict()) == list(plain.state_dict())
    x = torch.randn(2, 2, 8, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    net.eval(), plain.eval()
    with torch.no_grad():
        assert torch.equal(net(x), torch.nn.functional.softplus(plain(x)))
        assert torch.equal(net.compute_loss(x, x)['loss'], torch.nn.functional.mse_loss(net(x), x))


# ---- declarations and bindings -----------------------------------------------------------------------------------------------
NAMES = ['qgx_batch_gather', 'qgx_head_apply', 'qgx_head_grad', 'qgx_head_loss', 'qgx_head_workspace']


def test_header_declares_what_head_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_head_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_head_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.HEAD_TRAIN_SYMBOLS) == NAMES
    for name, _, args in _lib.HEAD_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    assert re.search(r'QGX_HEAD_MSE = 0, QGX_HEAD_SOFTPLUS_MSE = 1', code) and (_lib.HEAD_MSE, _lib.HEAD_SOFTPLUS_MSE) == (0, 1)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    others = _lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS + _lib.CONV_TRAIN_SYMBOLS
    assert not {n for n, _, _ in _lib.HEAD_TRAIN_SYMBOLS} & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'train_head.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_head_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    # the header says whose duty the indices' range is
    assert re.search(r"0 <= idx\[b\] < n is the CALLER'S DUTY", text)
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'fit_meanvar' in open(os.path.join(ROOT, doc)).read()


# ---- refusals, each without a device -----------------------------------------------------------------------------------------
GOOD = dict(B=3, N=16, C=2, n=5)
BAD_FIELDS = [('N', v) for v in (0, 8, 17, 24, 192, 256, -16)] + [('B', v) for v in (0, -1, 2 ** 29 // 256 + 1, 2 ** 62)] + \
             [('C', v) for v in (0, 9, -2)] + [('n', v) for v in (0, -4)]
FAKE, ODD = C.c_void_p(4096), C.c_void_p(4100)
BIG = 1 << 40


def _calls(lib, s, mode=0):
    """name -> (function, pointer names, optional ones, call(pointers)) for the four calls that take device pointers"""
    B, N, Cn, n = s['B'], s['N'], s['C'], s['n']
    return {
        'qgx_batch_gather': (['src_dev', 'idx_dev', 'out_dev'], {'idx_dev'},
                             lambda p, work=(FAKE, BIG): lib.qgx_batch_gather(*p, n, B, N, Cn, None)),
        'qgx_head_loss': (['y_dev', 't_dev', 'idx_dev', 'loss_dev'], {'idx_dev'},
                          lambda p, work=(FAKE, BIG): lib.qgx_head_loss(*p[:3], mode, p[3], B, N, Cn, n, *work, None)),
        'qgx_head_grad': (['y_dev', 't_dev', 'idx_dev', 'gout_dev', 'dy_dev'], {'idx_dev'},
                          lambda p, work=(FAKE, BIG): lib.qgx_head_grad(*p[:3], mode, p[3], p[4], B, N, Cn, n, None)),
        'qgx_head_apply': (['y_dev', 't_dev', 'idx_dev', 'out_dev'], {'t_dev', 'idx_dev'},
                           lambda p, work=(FAKE, BIG): lib.qgx_head_apply(*p[:3], mode, p[3], B, N, Cn, n, None)),
    }


def _workspace_bytes(B, N):
    from pyqg_generative_amd._lib import lib
    n = C.c_size_t(0)
    return lib.qgx_head_workspace(B, N, C.byref(n)), n.value


def test_workspace_is_a_function_of_the_grid_and_batch_alone():
    rc, n = _workspace_bytes(3, 16)
    assert rc == 0 and n > 0 and n % 16 == 0 and _workspace_bytes(3, 16) == (0, n)
    # float64 partials: a few KiB at the most, whatever the batch
    for B, N in ((1, 16), (64, 64), (2 ** 29 // 128 ** 2, 128), (2 ** 29 // 256, 16)):
        rc, n = _workspace_bytes(B, N)
        assert rc == 0 and 8 <= n <= 16 * 1024, (B, N, n)


@pytest.mark.parametrize('field,value', BAD_FIELDS)
def test_every_out_of_range_field_is_refused(field, value):
    from pyqg_generative_amd._lib import lib
    s = dict(GOOD, **{field: value})
    if field in ('B', 'N'):
        n = C.c_size_t(0)
        assert lib.qgx_head_workspace(s['B'], s['N'], C.byref(n)) == -1
        assert field.encode() in lib.qgx_last_error()
    for name, (ptrs, _, call) in _calls(lib, s).items():
        assert call([FAKE] * len(ptrs)) == -1, name
        msg = lib.qgx_last_error()
        assert name.encode() in msg and f'{field} = '.encode() in msg, msg


def test_rows_without_idx_and_an_unknown_mode_are_refused():
    from pyqg_generative_amd._lib import lib
    # n < B is fine with an index vector and refused without one
    s = dict(GOOD, n=2)
    for name, (ptrs, optional, call) in _calls(lib, s).items():
        p = [None if q == 'idx_dev' else FAKE for q in ptrs]
        assert call(p) == -1 and b'n = 2' in lib.qgx_last_error(), name
    # the forward output takes no targets: n is not looked at
    assert b'out_dev' in (lib.qgx_head_apply(FAKE, None, None, 0, None, 3, 16, 2, 0, None), lib.qgx_last_error())[1]
    for mode in (-1, 2, 7):
        for name, (ptrs, _, call) in _calls(lib, GOOD, mode).items():
            if name == 'qgx_batch_gather':
                continue
            assert call([FAKE] * len(ptrs)) == -1 and b'mode' in lib.qgx_last_error(), name


def test_null_pointers_misalignment_and_a_short_workspace_are_refused():
    from pyqg_generative_amd._lib import lib
    assert lib.qgx_head_workspace(3, 16, None) == -1 and b'bytes' in lib.qgx_last_error()
    rc, need = _workspace_bytes(GOOD['B'], GOOD['N'])
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
    ptrs, _, call = _calls(lib, GOOD)['qgx_head_loss']
    good = [FAKE] * len(ptrs)
    assert call(good, (None, need)) == -1 and b'work_dev' in lib.qgx_last_error()
    assert call(good, (ODD, need)) == -1 and b'work_dev' in lib.qgx_last_error()
    assert call(good, (FAKE, need - 1)) == -1 and b'work_bytes' in lib.qgx_last_error()
    assert call(good, (FAKE, 0)) == -1


# ---- FusedHeadCNN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', ['mse', 'softplus_mse'])
@pytest.mark.parametrize('hidden', [[5, 3], [128, 64, 32, 32, 32, 32, 32], [8]])
def test_state_dict_is_the_reference_nets(head, hidden):
    from pyqg_generative_amd.tools.train_CNN import FusedHeadCNN, TrainableAndrewCNN
    net = FusedHeadCNN(2, 2, hidden, head=head, seed=3)
    sd = net.state_dict()
    ref = hr.var_net(2, 2, hidden, torch.float32) if head == 'softplus_mse' else cr.torch_net(2, 2, hidden, True, True, torch.float32)
    assert list(sd) == list(ref.state_dict())
    assert all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in ref.state_dict().items())
    # the head adds no parameter and draws nothing: the seeded state is the parent's
    parent = TrainableAndrewCNN(2, 2, hidden, seed=3).state_dict()
    assert all(torch.equal(sd[k], parent[k]) for k in sd) and hasattr(net, 'indexed_loss') and net.head == head


def test_fused_head_refusals():
    from pyqg_generative_amd.tools.train_CNN import FusedHeadCNN
    with pytest.raises(ValueError, match='head'):
        FusedHeadCNN(2, 2, [8], head='softplus')
    with pytest.raises(ValueError, match='channels'):
        FusedHeadCNN(2, 9, [8])
    with pytest.raises(ValueError, match='hidden_channels'):
        FusedHeadCNN(2, 2, [300])


# ---- the folder --------------------------------------------------------------------------------------------------------------
def test_meanvar_folder_round_trip(tmp_path):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_CNN import FusedHeadCNN, write_meanvar_folder, channel_scaler
    from pyqg_generative_amd.tools.simulate import dataset_backend
    hidden = [5, 3]
    net_mean, net_var = FusedHeadCNN(2, 2, hidden, seed=11), FusedHeadCNN(2, 2, hidden, head='softplus_mse', seed=12)
    rs = np.random.RandomState(5)
    X = rs.randn(6, 2, 16, 16) * np.array([8e-6, 1e-6]).reshape(1, 2, 1, 1) + 1e-7
    Y = rs.randn(6, 2, 16, 16) * np.array([7e-12, 2e-13]).reshape(1, 2, 1, 1)
    xs, ys = channel_scaler(X), channel_scaler(Y)
    log_mean = {'loss': [0.9, 0.5, 0.25], 'loss_test': [1.0, 0.625, 0.375]}
    log_var = {'loss': [0.75, 0.5], 'loss_test': [0.875, 0.625]}
    folder = str(tmp_path / 'model')
    write_meanvar_folder(folder, net_mean.state_dict(), net_var.state_dict(), xs, ys, hidden, log_mean, log_var)
    files = ['model_args.json', 'net_mean.pt', 'net_var.pt', 'stats_mean.nc', 'stats_var.nc', 'x_scale.json', 'y_scale.json']
    assert sorted(os.listdir(folder)) == files
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='MeanVarModel', hidden_channels=hidden)
    for name, net in (('net_mean.pt', net_mean), ('net_var.pt', net_var)):
        back = torch.load(os.path.join(folder, name), map_location='cpu', weights_only=True)
        assert list(back) == list(net.state_dict()) and all(torch.equal(back[k], v) for k, v in net.state_dict().items())
    # what MeanVarModel(folder=..., hidden_channels=...) reads the folder with
    nets, x_std, y_std = weights.load_folder(folder, 'gz', hidden_channels=hidden)
    np.testing.assert_array_equal(x_std, xs.std.reshape(-1))
    np.testing.assert_array_equal(y_std, ys.std.reshape(-1))
    assert len(nets) == 2
    for got, net in zip(nets, (net_mean, net_var)):
        want = weights.net_from_state_dict_arch(net.state_dict(), 2, hidden, True, True, False)
        for key in ('conv_w', 'conv_b', 'bn_g', 'bn_b', 'bn_m', 'bn_v'):
            assert len(got[key]) == len(want[key])
            for a, b in zip(got[key], want[key]):
                np.testing.assert_array_equal(a, b)
    for name, log in (('stats_mean.nc', log_mean), ('stats_var.nc', log_var)):
        stats = dataset_backend().open_dataset(os.path.join(folder, name))
        np.testing.assert_array_equal(np.asarray(stats['epoch'].values), np.arange(1, len(log['loss']) + 1))
        for k, v in log.items():
            np.testing.assert_array_equal(np.asarray(stats[k].values), v)
    # a net_mean that was read from the folder has no log: its statistics stay as they are, the rest is replaced
    write_meanvar_folder(folder, net_mean.state_dict(), net_var.state_dict(), xs, ys, hidden, {}, {k: v[:1] for k, v in log_var.items()})
    assert sorted(os.listdir(folder)) == files
    assert dataset_backend().open_dataset(os.path.join(folder, 'stats_mean.nc'))['loss'].shape == (3,)
    assert dataset_backend().open_dataset(os.path.join(folder, 'stats_var.nc'))['loss'].shape == (1,)


def test_fit_meanvar_refusals_and_command_line():
    from pyqg_generative_amd.tools import train_CNN
    for kw, match in ((dict(batch_size=0), 'batch_size'), (dict(num_epochs=0), 'num_epochs'), (dict(learning_rate=float('nan')), 'learning_rate'),
                      (dict(learning_rate=-1.0), 'learning_rate'), (dict(hidden_channels=[300]), 'hidden_channels')):
        with pytest.raises(ValueError, match=match):
            train_CNN.fit_meanvar(None, None, **kw)
    assert 'seed + 1' in train_CNN.fit_meanvar.__doc__
    with pytest.raises(SystemExit):
        train_CNN.main(['--train', 'a', '--validate', 'b', '--model', 'CGANRegression'])
    # fit_ols keeps its torch-expression loss; train() takes the fused path only from a net that offers it
    assert not hasattr(train_CNN.TrainableAndrewCNN, 'indexed_loss')
