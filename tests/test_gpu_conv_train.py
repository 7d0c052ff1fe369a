"""GPU: the differentiable circular convolution of include/qgx_conv_train.h (csrc/conv_train.hip) against the float64
restatement of tests/conv_train_restatement.py: exact on integer data, within the a-priori float32 bound on Gaussian data,
zero pad channels, the same bits on a second call and on another stream, and every output and the workspace between guard
bands (tests/redzone.py).

More than one unit per share.  The weight gradient cuts the U = B N / R units of R image rows into S shares of `ups` consecutive
units, and the bias gradient the B N^2 pixels into blocks of ppb pixels; a workgroup that takes more than one unit (or a thread
more than one pixel per group) runs the accumulate-across-units code, the restaging barrier, the short last share.  Which case
does so is decided by the host-side plan, restated in tests/train_plan_restatement.py and pinned to the library on the CPU
(tests/test_conv_train_cpu.py).  The cases that are here for such a regime declare it as data (CONV_REGIMES there) and _run
asserts it against the restated plan before it launches; test_regime_table prints R, U, ups, S, the last share's units, the LDS
bytes and ppb of EVERY case from that plan — the table is computed, not written down here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import train_plan_restatement as tp
from redzone import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 5), (5, 2, 3), (8, 32, 3), (33, 7, 3), (40, 70, 5), (70, 40, 5), (1, 256, 3), (256, 1, 3)]
CASES = [s + (3, 16) for s in SHAPES] + \
        [s + bn for s in ((33, 7, 3), (40, 70, 5)) for bn in ((2, 48), (1, 16), (1, 48))] + \
        [(1, 256, 3, 34, 16)] + \
        [(8, 8, 5, 1, 32), (8, 8, 3, 2, 64), (8, 8, 3, 1, 96), (8, 8, 5, 1, 128)]       # a ragged last share; the other grids
CASES += [c for c in tp.CONV_REGIMES if c not in CASES]                                 # more than one unit per share
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


def _assert_regime(case):
    """a case that is here for a regime still is in it, by the restated plan"""
    cin, cout, k, B, N = case
    plan = tp.wgrad_plan(B, N, cin, cout, k)
    for key, want in tp.CONV_REGIMES.get(case, {}).items():
        assert plan[key] == want, f'{case} is no longer in its regime: {key} = {plan[key]}, declared {want}'


def test_regime_table():
    print('\n' + tp.regime_table(CASES))
    assert all(c in CASES for c in tp.CONV_REGIMES)
    plans = [tp.wgrad_plan(c[3], c[4], c[0], c[1], c[2]) for c in CASES]
    # what the cases cover between them: every unit size with several units per share, both LDS caps, every grid with either k
    assert {(p['R'], min(p['ups'], 3)) for p in plans} >= {(R, u) for R in (1, 2, 4) for u in (1, 2, 3)} - {(2, 3)}
    assert {p['under_80k'] for p in plans} == {True, False} and any(p['crosses_image'] for p in plans)
    assert any(p['ups'] > 1 and p['cot_n'] > 1 and p['cit_n'] > 1 for p in plans)
    assert any(p['dbias_passes'] > 2 and not p['dbias_even'] for p in plans)
    assert {(c[4], c[2]) for c in CASES} >= {(128, 3), (96, 5), (64, 5)}


def _run(case, integer, bias=True, guard=True):
    """the three calls through the C ABI on guarded buffers -> (y, dx, dw, db) as numpy, after the guard checks"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    _assert_regime(case)
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


NO_BIAS = [CASES[0], CASES[3], (8, 8, 5, 1, 128), (40, 70, 5, 23, 16)]      # the last: several units per share


@pytest.mark.parametrize('case', NO_BIAS, ids=[IDS[CASES.index(c)] for c in NO_BIAS])
def test_without_bias_nothing_is_added_and_db_is_not_touched(case):
    cin, cout, k, B, N = case
    y, dx, dw, _ = _run(case, True, bias=False)
    x, w, b, dy = _data(case, True)
    assert np.array_equal(y.astype(np.float64), cr.forward(x, w))
    t = _truth(case, True)
    assert np.array_equal(dx.astype(np.float64), t[1]) and np.array_equal(dw.astype(np.float64), t[2])


def test_a_stale_workspace_changes_nothing():
    """the workspace's previous contents (NaN patterns, another shape's partial sums) do not enter a result; the case with
    ups = 2 covers the slices a workgroup writes after its later units"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    for case in ((40, 70, 5, 3, 16), (40, 70, 5, 23, 16)):
        assert tp.wgrad_plan(case[3], case[4], *case[:3])['ups'] == (1 if case[3] == 3 else 2)
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
            assert np.array_equal(dw.cpu().numpy().view(np.int32), want[2].view(np.int32)), (case, fill)
            assert np.array_equal(db.cpu().numpy().view(np.int32), want[3].view(np.int32)), (case, fill)
