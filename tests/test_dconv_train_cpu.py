"""CPU: the discriminator's stride-2 convolution of include/qgx_dconv_train.h — the restatement against torch autograd of
F.conv2d(stride=2, padding=1), the parity-class identity the device's data gradient rests on, the declarations against the
bindings, every refusal before any device call, and the workspace size against the restated share plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import dconv_train_restatement as dr

SHAPES = [(1, 1, 2, 2), (2, 5, 2, 8), (6, 8, 3, 16), (33, 7, 2, 6), (8, 16, 1, 12)]       # cin, cout, B, N


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout,B,N', SHAPES)
def test_restatement_is_torch_autograd(cin, cout, B, N):
    import torch.nn.functional as F
    x, w, dy = dr.case_data(cin, cout, B, N, 100 + cin, integer=False)
    xt = torch.tensor(cr.from_layout(x, cin), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xt, wt, None, stride=2, padding=1)
    y.backward(torch.tensor(cr.from_layout(dy, cout), dtype=torch.float64))
    got_y, got_dx, got_dw = dr.forward(x, w), dr.backward_data(dy, w, N), dr.backward_weight(x, dy, cin, cout)
    tol = dict(rtol=0, atol=1e-12 * cin * cout * 16)
    np.testing.assert_allclose(cr.from_layout(got_y, cout), y.detach().numpy(), **tol)
    np.testing.assert_allclose(cr.from_layout(got_dx, cin), xt.grad.numpy(), **tol)
    np.testing.assert_allclose(got_dw, wt.grad.numpy(), rtol=0, atol=1e-12 * B * N * N)
    assert got_y.shape == (B, N // 2, N // 2, cr.c8(cout)) and got_dx.shape == (B, N, N, cr.c8(cin))
    assert not got_y[..., cout:].any() and not got_dx[..., cin:].any()


@pytest.mark.parametrize('cin,cout,B,N', SHAPES)
def test_data_gradient_is_four_parity_classes_of_a_2x2_tap_convolution(cin, cout, B, N):
    x, w, dy = dr.case_data(cin, cout, B, N, 200 + cin, integer=True)
    # integers: both sides are exact
    np.testing.assert_array_equal(dr.backward_data_by_parity(dy, w, N), dr.backward_data(dy, w, N))
    # the taps of a class: r = 2 i - 1 + ky with i = i' + di
    for p in (0, 1):
        assert all(2 * di - 1 + ky == p for ky, di in dr.parity_taps(p))
    assert sorted(ky for p in (0, 1) for ky, _ in dr.parity_taps(p)) == [0, 1, 2, 3]


def test_the_three_operations_are_closed_under_differentiation():
    """the identities tools/train_ops.py builds its Functions' backwards from: with <a, b> the sum of products,
    <g, bd(dy, w)> = <fw(g, w), dy> = <bw(g, dy), w>  and  <g, bw(x, dy)> = <bd(dy, g), x> = <fw(x, g), dy>"""
    cin, cout, B, N = 3, 5, 2, 6
    x, w, dy = dr.case_data(cin, cout, B, N, 7, integer=True)
    rs = np.random.RandomState(8)
    gx = cr.to_layout(rs.randint(-3, 4, size=(B, cin, N, N)).astype(np.float64))
    gw = rs.randint(-3, 4, size=w.shape).astype(np.float64)
    dot = lambda a, b: float(np.sum(np.asarray(a, np.float64) * np.asarray(b, np.float64)))
    assert dot(gx, dr.backward_data(dy, w, N)) == dot(dr.forward(gx, w), dy) == dot(dr.backward_weight(gx, dy, cin, cout), w)
    assert dot(gw, dr.backward_weight(x, dy, cin, cout)) == dot(dr.backward_data(dy, gw, N), x) == dot(dr.forward(x, gw), dy)


def _gpu_cases():
    """every case of tests/test_gpu_dconv_train.py (the module asks for no device when it is imported)"""
    import test_gpu_dconv_train as g
    return list(g.CASES)


def test_integer_cases_are_exact_in_float32():
    """operands in -3 ... 3: every partial sum of the GPU test's integer cases stays below 9 K < 2^24 in magnitude"""
    for cin, cout, B, N in _gpu_cases():
        assert 9 * 16 * cin < 2 ** 24 and 9 * 4 * cout < 2 ** 24 and 9 * B * (N // 2) ** 2 < 2 ** 24


# ---- the weight gradient's plan --------------------------------------------------------------------------------------
def _library_bytes(cin, cout, B, N):
    from pyqg_generative_amd._lib import lib
    n = C.c_size_t(0)
    assert lib.qgx_dconv2d_workspace(B, N, cin, cout, C.byref(n)) == 0
    return n.value


def test_restated_plan_gives_the_librarys_workspace_size():
    cases = _gpu_cases()
    assert set(dr.DCONV_REGIMES) <= set(cases)
    for cin, cout, B, N in cases:
        assert _library_bytes(cin, cout, B, N) == dr.workspace_bytes(B, N, cin, cout), (cin, cout, B, N)
    n = 0
    for N in (2, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128):
        for B in (1, 2, 3, 9, 64, 256, 500):
            for cin in (1, 6, 33, 64, 256, 512):
                for cout in (1, 7, 64, 130, 512):
                    assert _library_bytes(cin, cout, B, N) == dr.workspace_bytes(B, N, cin, cout), (cin, cout, B, N)
                    n += 1
    assert n == 12 * 7 * 6 * 5


def test_declared_regimes_hold_in_the_restated_plan():
    ragged = 0
    for (cin, cout, B, N), regime in dr.DCONV_REGIMES.items():
        plan = dr.dwgrad_plan(B, N, cin, cout)
        assert {key: plan[key] for key in regime} == regime, (cin, cout, B, N)
        ragged += plan['ups'] > 1 and plan['last_units'] < plan['ups']
    assert ragged >= 2
    # the plan's invariants: every unit in exactly one share, every pixel in exactly one unit
    for N in (2, 6, 16, 64, 128):
        for B in (1, 3, 64, 256, 500):
            for c in (1, 6, 70, 512):
                p = dr.dwgrad_plan(B, N, c, c)
                assert (p['S'] - 1) * p['ups'] < p['U'] <= p['S'] * p['ups'] and 1 <= p['last_units'] <= p['ups']
                assert (p['U'] - 1) * dr.UNIT < p['P'] <= p['U'] * dr.UNIT
    # the shipped discriminator at 64 x 64 and the 4B batch of 256: both regimes of the issue
    first, last = dr.dwgrad_plan(256, 64, 6, 64), dr.dwgrad_plan(256, 8, 256, 512)
    assert (first['tiles'], first['U'], first['ups']) == (2, 8192, 32) and (last['tiles'], last['U'], last['S']) == (512, 128, 1)


# ---- declarations and bindings ---------------------------------------------------------------------------------------
NAMES = ['qgx_dconv2d_backward_data', 'qgx_dconv2d_backward_weight', 'qgx_dconv2d_forward', 'qgx_dconv2d_workspace']


def test_header_declares_what_dconv_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_dconv_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_dconv_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.DCONV_TRAIN_SYMBOLS) == NAMES
    for name, _, args in _lib.DCONV_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    others = (_lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS + _lib.CONV_TRAIN_SYMBOLS + _lib.HEAD_TRAIN_SYMBOLS
              + _lib.FLUX_TRAIN_SYMBOLS + _lib.LATENT_TRAIN_SYMBOLS)
    assert not set(NAMES) & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'dconv_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_dconv_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()


# ---- refusals --------------------------------------------------------------------------------------------------------
GOOD = dict(B=3, N=16, cin=5, cout=7)
BAD_FIELDS = [('N', v) for v in (0, 1, 3, 17, 130, 256, -16)] + [('B', v) for v in (0, -1, 2 ** 29 // 256 + 1, 2 ** 62)] + \
             [('cin', v) for v in (0, 513, -3)] + [('cout', v) for v in (0, 513, -3)]


def _workspace_bytes(**kw):
    from pyqg_generative_amd._lib import lib
    s = dict(GOOD, **kw)
    n = C.c_size_t(0)
    rc = lib.qgx_dconv2d_workspace(s['B'], s['N'], s['cin'], s['cout'], C.byref(n))
    return rc, n.value


def test_workspace_is_a_function_of_the_shape_alone():
    rc, n = _workspace_bytes()
    assert rc == 0 and n > 0 and n % 16 == 0
    assert _workspace_bytes() == (0, n)
    # the shipped discriminator's layers at the 4B batch of 256: some tens of MB at the most
    for N, cin, cout in ((64, 6, 64), (32, 64, 128), (16, 128, 256), (8, 256, 512)):
        rc, big = _workspace_bytes(B=256, N=N, cin=cin, cout=cout)
        assert rc == 0 and big < 2 ** 26
    # the largest admitted grid and widths, the smallest grid with the largest batch
    assert _workspace_bytes(B=1, N=128, cin=512, cout=512)[0] == 0
    assert _workspace_bytes(B=2 ** 27, N=2, cin=1, cout=1)[0] == 0


@pytest.mark.parametrize('field,value', BAD_FIELDS)
def test_every_out_of_range_field_is_refused(field, value):
    from pyqg_generative_amd._lib import lib
    fake = C.c_void_p(4096)       # never dereferenced: every call below must be refused first
    s = dict(GOOD, **{field: value})
    shape = (s['B'], s['N'], s['cin'], s['cout'])
    n = C.c_size_t(0)
    assert lib.qgx_dconv2d_workspace(*shape, C.byref(n)) == -1
    assert field.encode() in lib.qgx_last_error()
    big = 1 << 40
    for fn in (lib.qgx_dconv2d_forward, lib.qgx_dconv2d_backward_data, lib.qgx_dconv2d_backward_weight):
        assert fn(fake, fake, fake, *shape, fake, big, None) == -1
        assert field.encode() in lib.qgx_last_error()


def test_null_pointers_misalignment_and_a_short_workspace_are_refused():
    from pyqg_generative_amd._lib import lib
    fake, odd = C.c_void_p(4096), C.c_void_p(4100)
    shape = tuple(GOOD[f] for f in ('B', 'N', 'cin', 'cout'))
    assert lib.qgx_dconv2d_workspace(*shape, None) == -1
    rc, need = _workspace_bytes()
    calls = {
        'qgx_dconv2d_forward': (lib.qgx_dconv2d_forward, ['x_dev', 'w_dev', 'y_dev']),
        'qgx_dconv2d_backward_data': (lib.qgx_dconv2d_backward_data, ['dy_dev', 'w_dev', 'dx_dev']),
        'qgx_dconv2d_backward_weight': (lib.qgx_dconv2d_backward_weight, ['x_dev', 'dy_dev', 'dw_dev']),
    }
    for name, (fn, ptrs) in calls.items():
        for i, p in enumerate(ptrs):
            for bad in (None, odd):
                args = [fake] * 3
                args[i] = bad
                assert fn(*args, *shape, fake, need, None) == -1, (name, p)
                msg = lib.qgx_last_error()
                assert name.encode() in msg and p.encode() in msg, msg
        good = [fake] * 3
        assert fn(*good, *shape, None, need, None) == -1 and b'work_dev' in lib.qgx_last_error()
        assert fn(*good, *shape, odd, need, None) == -1 and b'work_dev' in lib.qgx_last_error()
        assert fn(*good, *shape, fake, need - 1, None) == -1 and b'work_bytes' in lib.qgx_last_error()
        assert fn(*good, *shape, fake, 0, None) == -1
