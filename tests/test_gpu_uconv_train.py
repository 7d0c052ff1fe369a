"""GPU: the U-Net's training convolution of include/qgx_uconv_train.h (csrc/uconv_train.hip) against the float64 restatement of
tests/uconv_train_restatement.py: exact on integer data, within the a-priori float32 bound on Gaussian data, zero pad channels,
the same bits on a second call and on another stream, no bias, a stale workspace, and every output and the workspace between
guard bands (tests/redzone.py).

The cases that are here for a regime of the weight gradient (a share of several units, a ragged last share, one share stored
directly, units that cross an image boundary) declare it as data (UCONV_REGIMES there); _run asserts it against the restated
plan before it launches, and tests/test_uconv_train_cpu.py pins that plan to the library."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import uconv_train_restatement as ur
from redzone import guarded

pytestmark = pytest.mark.gpu

# (cin, cout, k, B, N)
CASES = [(1, 1, 3, 1, 2), (4, 7, 3, 3, 2), (7, 4, 1, 1, 2),        # 2 x 2: the taps 0 and 2 wrap onto the same row
         (33, 7, 3, 2, 3), (4, 33, 1, 3, 3),                       # an odd grid
         (7, 70, 3, 1, 4), (70, 33, 3, 3, 4),                      # 16 pixels: images that do not fill a unit of 32
         (70, 4, 1, 2, 6), (1, 70, 3, 1, 6),
         (512, 8, 3, 1, 4), (8, 1024, 1, 3, 4),                    # the widest input, the widest output (up512's ConvTranspose2d)
         (4, 32, 3, 2, 16), (32, 32, 3, 1, 32)]                    # conv32 and a top-level layer: many row tiles
CASES += [c for c in ur.UCONV_REGIMES if c not in CASES]
IDS = ['cin%d-cout%d-k%d-B%d-N%d' % c for c in CASES]


def _dev():
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _data(case, integer):
    cin, cout, k, B, N = case
    arrays = ur.case_data(cin, cout, k, B, N, 3000 + 7 * cin + cout + 5 * k + B + N, integer)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _truth(case, integer, absolute=False, bias=True):
    """float64 y, dx, dw, db of the case (absolute: of the operands' magnitudes — the bound's scale); computed once, read-only"""
    cin, cout, k, B, N = case
    x, w, b, dy = (np.abs(a) if absolute else a for a in _data(case, integer))
    out = (ur.forward(x, w, b if bias else None), ur.backward_data(dy, w)) + ur.backward_weight(x, dy, cin, cout, k)
    for a in out:
        a.setflags(write=False)
    return out


def _assert_regime(case):
    cin, cout, k, B, N = case
    plan = ur.uwgrad_plan(B, N, cin, cout, k)
    for key, want in ur.UCONV_REGIMES.get(case, {}).items():
        assert plan[key] == want, f'{case} is no longer in its regime: {key} = {plan[key]}, declared {want}'


def _run(case, integer, guard=True, ws_fill=0xFF, bias=True):
    """the three calls through the C ABI on guarded buffers -> (y, dx, dw, db) as numpy, after the guard checks; without
    `bias` the forward gets no bias and the weight gradient no db, whose buffer must keep its prefill"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    _assert_regime(case)
    cin, cout, k, B, N = case
    x, w, b, dy = (torch.as_tensor(a).to(_dev()) for a in _data(case, integer))
    n = C.c_size_t()
    check(lib.qgx_uconv2d_workspace(B, N, cin, cout, k, C.byref(n)))
    assert n.value == ur.workspace_bytes(B, N, cin, cout, k)
    ws = guarded((n.value,), torch.uint8, _dev(), fill=ws_fill)
    y = guarded((B, N, N, cr.c8(cout)), torch.float32, _dev())
    dx = guarded((B, N, N, cr.c8(cin)), torch.float32, _dev())
    dw = guarded((cout, cin, k, k), torch.float32, _dev())
    db = guarded((cout,), torch.float32, _dev())
    shape = (B, N, cin, cout, k)
    st = current_stream_ptr()
    work = (ws.t.data_ptr(), n.value, st)
    check(lib.qgx_uconv2d_forward(x.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None, y.t.data_ptr(), *shape, *work))
    check(lib.qgx_uconv2d_backward_data(dy.data_ptr(), w.data_ptr(), dx.t.data_ptr(), *shape, *work))
    check(lib.qgx_uconv2d_backward_weight(x.data_ptr(), dy.data_ptr(), dw.t.data_ptr(), db.t.data_ptr() if bias else None, *shape, *work))
    torch.cuda.synchronize()
    if guard:
        ws.check(what='workspace')
        for g, name in ((y, 'y'), (dx, 'dx'), (dw, 'dw')):
            g.check(written=True, what=name)
        db.check(written=bias, what='db')
        if not bias:
            assert db.unwritten() == cout, 'db was written without being asked for'
    return tuple(g.t.cpu().numpy() for g in (y, dx, dw, db))


NAMES = ('y', 'dx', 'dw', 'db')


def test_regime_table():
    """the restated plan of every case, printed"""
    print('\n%-28s %8s %6s %5s %5s %6s %6s %7s' % ('case', 'pixels', 'units', 'ups', 'S', 'tiles', 'last', 'direct'))
    for case, name in zip(CASES, IDS):
        cin, cout, k, B, N = case
        _assert_regime(case)
        p = ur.uwgrad_plan(B, N, cin, cout, k)
        print('%-28s %8d %6d %5d %5d %6d %6d %7s' % (name, p['P'], p['U'], p['ups'], p['S'], p['tiles'], p['last_units'], p['direct']))
    plans = [ur.uwgrad_plan(B, N, cin, cout, k) for cin, cout, k, B, N in CASES]
    assert any(p['direct'] and p['U'] > 1 for p in plans) and any(p['ups'] > 1 and p['last_units'] < p['ups'] for p in plans)
    assert any(N * N % ur.UNIT and B > 1 for _, _, _, B, N in CASES)           # a unit that crosses an image boundary
    assert any(B == 1 for _, _, _, B, _ in CASES) and any(B % 2 and B > 1 for _, _, _, B, _ in CASES)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_exact_on_integers(case):
    """x, w, bias, dy integers in -3 ... 3: every product and partial sum is an integer below 2^24 (asserted from the
    restatement of |operands|, whose entries bound every partial sum), float32 arithmetic is exact in any order, and the
    results must EQUAL the float64 restatement — a dropped, doubled or misplaced term shows"""
    got = _run(case, True)
    for name, g, t, ta in zip(NAMES, got, _truth(case, True), _truth(case, True, True)):
        assert ta.max() < 2 ** 24
        bad = np.argwhere(g.astype(np.float64) != t)
        assert bad.size == 0, f'{name}: {len(bad)} of {t.size} elements differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {t[tuple(bad[0])]}'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_rounding_class_on_gaussian_data(case):
    """|result - truth64| <= (K + 2) 2^-24 truth64(|operands|) elementwise, K the number of summed terms (k^2 cin and the
    bias, k^2 cout, B N^2): the a-priori bound of a float32 sum in any order.  The largest ratio to the bound is printed."""
    cin, cout, k, B, N = case
    got = _run(case, False)
    K = dict(y=k * k * cin + 1, dx=k * k * cout, dw=B * N * N, db=B * N * N)
    worst = {}
    for name, g, t, ta in zip(NAMES, got, _truth(case, False), _truth(case, False, True)):
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
        assert y.shape == (B, N, N, cr.c8(cout)) and dx.shape == (B, N, N, cr.c8(cin))
        assert not y[..., cout:].any() and not dx[..., cin:].any()
        if not integer:                     # a single integer of -3 ... 3 may be zero; a Gaussian is not
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
    for name, a, b, c in zip(NAMES, first, second, third):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f'{name}: a second call gave other bits'
        assert np.array_equal(a.view(np.int32), c.view(np.int32)), f'{name}: another stream gave other bits'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_without_a_bias_nothing_is_added_and_db_is_untouched(case):
    """bias_dev = NULL: y is the convolution alone (exact on integers); db_dev = NULL: dw has the bits of the run with db, and
    the db buffer that was not passed keeps its prefill (_run)"""
    y, dx, dw, _ = _run(case, True, bias=False)
    assert np.array_equal(y.astype(np.float64), _truth(case, True, bias=False)[0])
    with_bias = _run(case, True, guard=False)
    assert np.array_equal(dw.view(np.int32), with_bias[2].view(np.int32)) and np.array_equal(dx.view(np.int32), with_bias[1].view(np.int32))


STALE = [(70, 33, 3, 3, 4), (8, 72, 3, 500, 6), (512, 456, 3, 3, 4)]


@pytest.mark.parametrize('case', STALE, ids=[IDS[CASES.index(c)] for c in STALE])
def test_a_stale_workspace_changes_nothing(case):
    """the workspace's previous contents (NaN patterns, zeros) do not enter a result; the case with ups = 5 covers the slices a
    workgroup writes after its later units, the direct one a workspace that holds the weights alone"""
    want = _run(case, False, guard=False)
    for fill in (0x00, 0x7F):
        got = _run(case, False, ws_fill=fill)
        for name, a, b in zip(NAMES, want, got):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, case, fill)
