"""GPU: the differentiable circular convolution of include/qgx_conv_train.h (csrc/conv_train.hip) against the float64
restatement of tests/conv_train_restatement.py: exact on integer data, within the a-priori float32 bound on Gaussian data,
zero pad channels, the same bits on a second call and on another stream, and every output and the workspace between guard
bands (tests/redzone.py).

The ragged case.  The weight gradient cuts the U = B N / R units of R image rows (R = 4 where the two LDS patches of four
rows fit 80 KiB: every tested shape but the 5 x 5 one at 48 x 48, which has R = 2) into S shares of
ups = ceil(U / min(U, ceil(512 / pairs))) units, pairs = ceil(cout / 32) ceil(cin / 32).  (cin, cout, k) = (1, 256, 3) at
B = 34, N = 16 has pairs = 8, U = 136, ups = 3, S = 46: the last share holds ONE unit where the others hold three.  (Every
other tested shape has ups = 1.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
from redzone import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 5), (5, 2, 3), (8, 32, 3), (33, 7, 3), (40, 70, 5), (70, 40, 5), (1, 256, 3), (256, 1, 3)]
CASES = [s + (3, 16) for s in SHAPES] + \
        [s + bn for s in ((33, 7, 3), (40, 70, 5)) for bn in ((2, 48), (1, 16), (1, 48))] + \
        [(1, 256, 3, 34, 16)] + \
        [(8, 8, 5, 1, 32), (8, 8, 3, 2, 64), (8, 8, 3, 1, 96), (8, 8, 5, 1, 128)]       # ragged (module docstring); the other grids
IDS = ['cin%d-cout%d-k%d-B%d-N%d' % c for c in CASES]


def _dev():
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _data(case, integer):
    cin, cout, k, B, N = case
    arrays = cr.case_data(cin, cout, k, B, N, 1000 + 7 * cin + cout + k + B + N, integer)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _truth(case, integer, absolute=False):
    """float64 y, dx, dw, db of the case (absolute: of the operands' magnitudes — the bound's scale); computed once, read-only"""
    cin, cout, k, B, N = case
    x, w, b, dy = (np.abs(a) if absolute else a for a in _data(case, integer))
    dw, db = cr.backward_weight(x, dy, cin, cout, k)
    out = (cr.forward(x, w, b), cr.backward_data(dy, w), dw, db)
    for a in out:
        a.setflags(write=False)
    return out


def _run(case, integer, bias=True, guard=True):
    """the three calls through the C ABI on guarded buffers -> (y, dx, dw, db) as numpy, after the guard checks"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    cin, cout, k, B, N = case
    x, w, b, dy = (torch.as_tensor(a).to(_dev()) for a in _data(case, integer))
    n = C.c_size_t()
    check(lib.qgx_conv2d_workspace(B, N, cin, cout, k, C.byref(n)))
    ws = guarded((n.value,), torch.uint8, _dev())
    y = guarded((B, N, N, cr.c8(cout)), torch.float32, _dev())
    dx = guarded((B, N, N, cr.c8(cin)), torch.float32, _dev())
    dw = guarded((cout, cin, k, k), torch.float32, _dev())
    db = guarded((cout,), torch.float32, _dev())
    shape = (B, N, cin, cout, k)
    st = current_stream_ptr()
    check(lib.qgx_conv2d_forward(x.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None, y.t.data_ptr(), *shape,
                                 ws.t.data_ptr(), n.value, st))
    check(lib.qgx_conv2d_backward_data(dy.data_ptr(), w.data_ptr(), dx.t.data_ptr(), *shape, ws.t.data_ptr(), n.value, st))
    check(lib.qgx_conv2d_backward_weight(x.data_ptr(), dy.data_ptr(), dw.t.data_ptr(), db.t.data_ptr() if bias else None, *shape,
                                         ws.t.data_ptr(), n.value, st))
    torch.cuda.synchronize()
    if guard:
        ws.check(what='workspace')
        for g, name in ((y, 'y'), (dx, 'dx'), (dw, 'dw')) + (((db, 'db'),) if bias else ()):
            g.check(written=True, what=name)
        if not bias:
            db.check(what='db (not asked for)')
            assert db.unwritten() == cout
    return tuple(g.t.cpu().numpy() for g in (y, dx, dw, db))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_exact_on_integers(case):
    """x, w, bias, dy integers in -3 ... 3: every product and partial sum is an integer below 2^24, float32 arithmetic is exact in
    any order, and the results must EQUAL the float64 restatement — a dropped, doubled or misplaced term shows"""
    got = _run(case, True)
    for name, g, t in zip(('y', 'dx', 'dw', 'db'), got, _truth(case, True)):
        assert np.abs(t).max() < 2 ** 24
        bad = np.argwhere(g.astype(np.float64) != t)
        assert bad.size == 0, f'{name}: {len(bad)} of {t.size} elements differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {t[tuple(bad[0])]}'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_rounding_class_on_gaussian_data(case):
    """|result - truth64| <= (K + 2) 2^-24 truth64(|operands|) elementwise, K the number of summed terms (cin k^2, cout k^2,
    B N^2): the a-priori bound of a float32 sum in any order.  The largest ratio to the bound is printed."""
    cin, cout, k, B, N = case
    got = _run(case, False)
    K = dict(y=cin * k * k, dx=cout * k * k, dw=B * N * N, db=B * N * N)
    worst = {}
    for name, g, t, ta in zip(('y', 'dx', 'dw', 'db'), got, _truth(case, False), _truth(case, False, True)):
        bound = (K[name] + 2) * 2.0 ** -24 * ta
        err = np.abs(g.astype(np.float64) - t)
        live = bound > 0
        assert not err[~live].any(), name                       # pad channels: a zero bound, a zero result
        worst[name] = float((err[live] / bound[live]).max())
    print('\n%s: largest error / bound  ' % (case,) + '  '.join(f'{n} {v:.4f}' for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_pad_channels_are_zero(case):
    cin, cout, k, B, N = case
    for integer in (True, False):
        y, dx, _, _ = _run(case, integer, guard=False)
        assert y.shape[-1] == cr.c8(cout) and dx.shape[-1] == cr.c8(cin)
        assert not y[..., cout:].any() and not dx[..., cin:].any()
        assert y[..., :cout].any() and dx[..., :cin].any()


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_same_bits_again_and_on_another_stream(case):
    first = _run(case, False, guard=False)
    second = _run(case, False, guard=False)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        third = _run(case, False, guard=False)
    torch.cuda.current_stream().wait_stream(st)
    for name, a, b, c in zip(('y', 'dx', 'dw', 'db'), first, second, third):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f'{name}: a second call gave other bits'
        assert np.array_equal(a.view(np.int32), c.view(np.int32)), f'{name}: another stream gave other bits'


@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[-1]], ids=[IDS[0], IDS[3], IDS[-1]])
def test_without_bias_nothing_is_added_and_db_is_not_touched(case):
    cin, cout, k, B, N = case
    y, dx, dw, _ = _run(case, True, bias=False)
    x, w, b, dy = _data(case, True)
    assert np.array_equal(y.astype(np.float64), cr.forward(x, w))
    t = _truth(case, True)
    assert np.array_equal(dx.astype(np.float64), t[1]) and np.array_equal(dw.astype(np.float64), t[2])


def test_a_stale_workspace_changes_nothing():
    """the workspace's previous contents (NaN patterns, another shape's partial sums) do not enter a result"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    case = (40, 70, 5, 3, 16)
    cin, cout, k, B, N = case
    want = _run(case, False, guard=False)
    x, w, b, dy = (torch.as_tensor(a).to(_dev()) for a in _data(case, False))
    n = C.c_size_t()
    check(lib.qgx_conv2d_workspace(B, N, cin, cout, k, C.byref(n)))
    for fill in (0x00, 0x7F):
        ws = guarded((n.value,), torch.uint8, _dev(), fill=fill)
        dw = torch.empty((cout, cin, k, k), device=_dev())
        db = torch.empty((cout,), device=_dev())
        check(lib.qgx_conv2d_backward_weight(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), B, N, cin, cout, k,
                                             ws.t.data_ptr(), n.value, current_stream_ptr()))
        torch.cuda.synchronize()
        ws.check(what='workspace')
        assert np.array_equal(dw.cpu().numpy().view(np.int32), want[2].view(np.int32))
        assert np.array_equal(db.cpu().numpy().view(np.int32), want[3].view(np.int32))
