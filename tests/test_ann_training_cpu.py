"""CPU: the training entry points of include/qgx_train.h (declarations, bindings, argument refusals before any device
call), the learning-rate schedule of the restatement and of fit_ann against torch's MultiStepLR, fit_ann's refusals, and the
model-folder writer against the loaders."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT


def test_header_declares_what_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.TRAIN_SYMBOLS)
    assert {'qgx_ann_rows', 'qgx_ann_trainer_create', 'qgx_ann_trainer_destroy', 'qgx_ann_trainer_grad', 'qgx_ann_trainer_adam',
            'qgx_ann_trainer_step', 'qgx_ann_trainer_loss', 'qgx_ann_trainer_read', 'qgx_ann_trainer_write'} <= set(declared)
    # one argument type per declared argument
    for name, _, args in _lib.TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert not {n for n, _, _ in _lib.TRAIN_SYMBOLS} & {n for n, _, _ in _lib.SYMBOLS}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'ann_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'fit_ann' in open(os.path.join(ROOT, doc)).read()


def _weights_struct(s=3, hidden=(24, 24)):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.engine import Generator
    keep = []
    net = weights.synthetic_ann(3 if s % 2 == 0 else s, list(hidden), False, 0)
    a = Generator._ann_struct(net, keep)
    a.stencil_size = s
    return a, keep


def test_refusals_before_any_device_call():
    from pyqg_generative_amd._lib import lib
    fake = C.c_void_p(256)       # never dereferenced: every call below must be refused first
    nan, inf = float('nan'), float('inf')

    def rows(img=fake, n_img=4, N=24, s=3, step=3, out=fake):
        return lib.qgx_ann_rows(img, n_img, N, s, step, out, None)
    assert rows(img=None) == -1 and rows(out=None) == -1
    assert rows(n_img=0) == -1 and rows(N=0) == -1
    assert rows(s=2) == -1 and rows(s=4) == -1 and rows(s=0) == -1 and rows(s=9) == -1 and rows(s=-1) == -1
    assert rows(step=0) == -1 and rows(step=-3) == -1
    assert b'qgx_ann_rows' in lib.qgx_last_error()

    h = C.c_void_p()
    good, keep = _weights_struct()
    assert lib.qgx_ann_trainer_create(None, 0, C.byref(h)) == -1
    assert lib.qgx_ann_trainer_create(C.byref(good), 0, None) == -1
    even, keep2 = _weights_struct(s=4)
    assert lib.qgx_ann_trainer_create(C.byref(even), 0, C.byref(h)) == -1
    assert b'stencil_size' in lib.qgx_last_error()
    wide, keep3 = _weights_struct()
    wide.hidden[1] = 129
    assert lib.qgx_ann_trainer_create(C.byref(wide), 0, C.byref(h)) == -1
    deep, keep4 = _weights_struct()
    deep.n_hidden = 5
    assert lib.qgx_ann_trainer_create(C.byref(deep), 0, C.byref(h)) == -1
    assert lib.qgx_ann_trainer_create(C.byref(good), -1, C.byref(h)) == -1
    assert not h.value
    assert lib.qgx_ann_trainer_size(None) == -1

    def batch(fn, t=fake, x=fake, y=fake, idx=fake, n=8, xs=1.0, ys=1.0, lr=None, acc=fake):
        extra = [] if lr is None else [lr]
        return fn(t, x, y, idx, n, xs, ys, *extra, acc, None)
    for fn, lr in ((lib.qgx_ann_trainer_grad, None), (lib.qgx_ann_trainer_step, 1e-3), (lib.qgx_ann_trainer_loss, None)):
        assert batch(fn, lr=lr, t=None) == -1 and batch(fn, lr=lr, x=None) == -1 and batch(fn, lr=lr, y=None) == -1
        assert batch(fn, lr=lr, n=0) == -1 and batch(fn, lr=lr, n=-5) == -1
        assert batch(fn, lr=lr, xs=0.0) == -1 and batch(fn, lr=lr, ys=nan) == -1 and batch(fn, lr=lr, xs=inf) == -1
    assert batch(lib.qgx_ann_trainer_grad, idx=None) == -1 and batch(lib.qgx_ann_trainer_step, lr=1e-3, idx=None) == -1
    assert batch(lib.qgx_ann_trainer_loss, acc=None) == -1
    for bad in (nan, inf, -1e-3):
        assert batch(lib.qgx_ann_trainer_step, lr=bad) == -1
        assert lib.qgx_ann_trainer_adam(fake, bad, None) == -1
    assert b'lr' in lib.qgx_last_error()
    assert lib.qgx_ann_trainer_adam(None, 1e-3, None) == -1

    buf = np.zeros(4, np.float32)
    for what in (-1, 4, 100):
        assert lib.qgx_ann_trainer_read(fake, what, buf.ctypes.data) == -1
        assert lib.qgx_ann_trainer_write(fake, what, buf.ctypes.data, 0) == -1
    assert b'what' in lib.qgx_last_error()
    assert lib.qgx_ann_trainer_read(None, 0, buf.ctypes.data) == -1 and lib.qgx_ann_trainer_read(fake, 0, None) == -1
    assert lib.qgx_ann_trainer_write(None, 0, buf.ctypes.data, 0) == -1 and lib.qgx_ann_trainer_write(fake, 0, None, 0) == -1
    assert lib.qgx_ann_trainer_destroy(None) == 0


@pytest.mark.parametrize('E', [1, 2, 3, 4, 5, 6, 7, 8, 9, 50])
def test_learning_rates_are_multisteplr(E):
    import ann_training_restatement as ar
    from pyqg_generative_amd.tools.train_common import learning_rates
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    want = []
    for _ in range(E):
        want.append(opt.param_groups[0]['lr'])
        opt.step()
        sched.step()
    assert ar.lr_sequence(E, 1e-3) == want
    assert learning_rates(E, 1e-3) == want
    if E == 50:
        assert [want[0], want[24], want[25], want[37], want[43]] == pytest.approx([1e-3, 1e-3, 1e-4, 1e-5, 1e-6], rel=1e-12)


def test_fit_ann_refuses_before_device_work():
    import ann_training_restatement as ar
    from pyqg_generative_amd.tools.train_ANN import fit_ann
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    q, f = ar.teacher_student_images(4, 12, 0)
    ds = ar.as_dataset(q, f, 1)
    dims = ['run', 'time', 'lev', 'y', 'x']
    with pytest.raises(ValueError, match='batch_size'):
        fit_ann(ds, ds, batch_size=0)
    with pytest.raises(ValueError, match='num_epochs'):
        fit_ann(ds, ds, num_epochs=0)
    with pytest.raises(ValueError, match='q_forcing_advection'):
        fit_ann(xr.Dataset({'q': (dims, q.reshape(1, 2, 2, 12, 12))}), ds)
    with pytest.raises(ValueError, match="'q'"):
        fit_ann(ds, [ds, xr.Dataset({'q_forcing_advection': (dims, q.reshape(1, 2, 2, 12, 12))})])
    flat = xr.Dataset({k: (dims, q.reshape(1, 2, 2, 6, 24)) for k in ('q', 'q_forcing_advection')})
    with pytest.raises(ValueError, match='not square'):
        fit_ann(flat, ds)
    with pytest.raises(ValueError, match='learning_rate'):
        fit_ann(ds, ds, learning_rate=float('nan'))


def test_ann_model_still_refuses_training_and_points_to_fit_ann():
    from pyqg_generative_amd.models import ANNModel
    with pytest.raises(NotImplementedError, match='fit_ann') as e:
        ANNModel(read=False)
    assert 'read=False' in str(e.value) and 'training' in str(e.value)
    with pytest.raises(NotImplementedError, match='fit_ann') as e:
        ANNModel.fit(None)
    assert 'training' in str(e.value)


@pytest.mark.parametrize('s,hidden,si', [(3, [24, 24], False), (5, [7, 13, 5], True)])
def test_model_folder_round_trip(tmp_path, s, hidden, si):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_ANN import write_model_folder
    from pyqg_generative_amd.tools.simulate import dataset_backend
    net = weights.synthetic_ann(s, hidden, si, 7)
    sd = {}
    for l in range(len(hidden) + 1):
        sd[f'layers.{2 * l}.weight'], sd[f'layers.{2 * l}.bias'] = net['w'][l], net['b'][l]
    folder = str(tmp_path / 'model')
    log = {'loss': [0.9, 0.5, 0.25], 'loss_test': [1.0, 0.625, 0.375]}
    xs, ys = float(np.float32(1.2345678)), float(np.float32(9.87e-7))
    write_model_folder(folder, sd, xs, ys, s, hidden, si, log)
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'scale.json', 'stats.nc']
    back = torch.load(os.path.join(folder, 'net.pt'), map_location='cpu', weights_only=True)
    assert list(back) == list(sd) and all(v.dtype == torch.float32 and v.device.type == 'cpu' for v in back.values())
    nets, x_scale, y_scale = weights.load_ann_folder(folder)
    assert (x_scale, y_scale) == (xs, ys)
    assert nets[0]['stencil_size'] == s and nets[0]['hidden'] == hidden and nets[0]['scale_invariant'] == si
    for l in range(len(hidden) + 1):
        np.testing.assert_array_equal(nets[0]['w'][l], net['w'][l])
        np.testing.assert_array_equal(nets[0]['b'][l], net['b'][l])
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(model='ANNModel', stencil_size=s,
                                                                            hidden_channels=hidden, scale_invariant=si)
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    np.testing.assert_array_equal(np.asarray(stats['epoch'].values), [1, 2, 3])
    for k, v in log.items():
        assert tuple(stats[k].dims) == ('epoch',)
        np.testing.assert_array_equal(np.asarray(stats[k].values), v)
    # a second write replaces the files
    write_model_folder(folder, sd, xs, ys, s, hidden, si, {k: v[:2] for k, v in log.items()})
    assert dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))['loss'].shape == (2,)


def test_restated_rows_are_the_wrapped_stencils():
    import ann_training_restatement as ar
    rs = np.random.RandomState(0)
    img = rs.randn(3, 7, 7).astype(np.float32)
    rows = ar.stencil_rows(img, 3, 3)
    nc = 3
    assert rows.shape == (nc * nc * 3, 9)
    for (cj, ci, im, dy, dx) in [(0, 0, 0, 0, 0), (2, 1, 2, 2, 0), (1, 2, 1, 1, 1), (2, 2, 0, 2, 2)]:
        assert rows[(cj * nc + ci) * 3 + im, dy * 3 + dx] == img[im, (cj * 3 + dy - 1) % 7, (ci * 3 + dx - 1) % 7]
    np.testing.assert_array_equal(ar.stencil_rows(img, 1, 1).reshape(7, 7, 3), np.moveaxis(img, 0, -1))
