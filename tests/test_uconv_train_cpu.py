"""CPU: the U-Net's training convolution of include/qgx_uconv_train.h — the restatement against torch autograd of F.conv2d on
circular padding, the declarations against the bindings, every refusal before any device call, and the workspace size against
the restated share plan, over every layer of the U-Net at every admitted grid."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import ROOT

import conv_train_restatement as cr
import uconv_train_restatement as ur

SHAPES = [(1, 1, 3, 1, 2), (2, 5, 3, 2, 3), (6, 8, 1, 3, 4), (33, 7, 3, 2, 6), (8, 16, 1, 1, 2), (4, 9, 3, 2, 5)]     # cin, cout, k, B, N


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout,k,B,N', SHAPES)
def test_restatement_is_torch_autograd(cin, cout, k, B, N):
    import torch.nn.functional as F
    x, w, b, dy = ur.case_data(cin, cout, k, B, N, 100 + cin, integer=False)
    xt = torch.tensor(cr.from_layout(x, cin), dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    p = k // 2
    y = F.conv2d(F.pad(xt, (p, p, p, p), mode='circular') if p else xt, wt, bt)
    y.backward(torch.tensor(cr.from_layout(dy, cout), dtype=torch.float64))
    got_y, got_dx = ur.forward(x, w, b), ur.backward_data(dy, w)
    got_dw, got_db = ur.backward_weight(x, dy, cin, cout, k)
    tol = dict(rtol=0, atol=1e-12 * cin * cout * k * k)
    np.testing.assert_allclose(cr.from_layout(got_y, cout), y.detach().numpy(), **tol)
    np.testing.assert_allclose(cr.from_layout(got_dx, cin), xt.grad.numpy(), **tol)
    np.testing.assert_allclose(got_dw, wt.grad.numpy(), rtol=0, atol=1e-12 * B * N * N)
    np.testing.assert_allclose(got_db, bt.grad.numpy(), rtol=0, atol=1e-12 * B * N * N)
    assert got_y.shape == (B, N, N, cr.c8(cout)) and got_dx.shape == (B, N, N, cr.c8(cin))
    assert not got_y[..., cout:].any() and not got_dx[..., cin:].any()
    # without a bias nothing is added
    np.testing.assert_array_equal(ur.forward(x, w), ur.forward(x, w, np.zeros(cout)))


def test_at_two_by_two_the_outer_taps_reach_the_same_row():
    x, w, b, dy = ur.case_data(2, 3, 3, 1, 2, 5, integer=True)
    folded = np.zeros_like(w)
    folded[:, :, 1, :] = w[:, :, 1, :]
    folded[:, :, 0, :] = w[:, :, 0, :] + w[:, :, 2, :]          # ky = 0 and ky = 2 read the same row of a 2 x 2 grid
    np.testing.assert_array_equal(ur.forward(x, w), ur.forward(x, folded))


def _gpu_cases():
    """every case of tests/test_gpu_uconv_train.py (the module asks for no device when it is imported)"""
    import test_gpu_uconv_train as g
    return list(g.CASES)


def test_integer_cases_are_exact_in_float32():
    """operands in -3 ... 3: every partial sum of the GPU test's integer cases stays below 9 K + 3 < 2^24 in magnitude"""
    for cin, cout, k, B, N in _gpu_cases():
        assert 9 * k * k * cin + 3 < 2 ** 24 and 9 * k * k * cout < 2 ** 24 and 9 * B * N * N < 2 ** 24


# ---- the weight gradient's plan --------------------------------------------------------------------------------------
def _library_bytes(cin, cout, k, B, N):
    from pyqg_generative_amd._lib import lib
    n = C.c_size_t(0)
    assert lib.qgx_uconv2d_workspace(B, N, cin, cout, k, C.byref(n)) == 0, lib.qgx_last_error()
    return n.value


def test_restated_plan_gives_the_librarys_workspace_size():
    cases = _gpu_cases()
    assert set(ur.UCONV_REGIMES) <= set(cases)
    for cin, cout, k, B, N in cases:
        assert _library_bytes(cin, cout, k, B, N) == ur.workspace_bytes(B, N, cin, cout, k), (cin, cout, k, B, N)
    n = 0
    for N in (2, 3, 5, 8, 17, 64, 128):
        for B in (1, 3, 64, 500):
            for cin in (1, 7, 64, 512):
                for cout in (1, 70, 512, 1024):
                    for k in (1, 3):
                        assert _library_bytes(cin, cout, k, B, N) == ur.workspace_bytes(B, N, cin, cout, k), (cin, cout, k, B, N)
                        n += 1
    assert n == 7 * 4 * 4 * 4 * 2


def test_every_unet_layer_is_admitted_and_sized_by_the_restated_plan():
    seen = 0
    for N in (32, 48, 64, 96, 128):
        layers = ur.unet_layers(N)
        assert len(layers) == 1 + 11 * 3 + 4 + 1
        assert {n for _, _, _, n in layers} == {N, N // 2, N // 4, N // 8, N // 16}
        for cin, cout, k, n in layers:
            for B in (1, 2, 64, 256):
                got = _library_bytes(cin, cout, k, B, n)
                assert got == ur.workspace_bytes(B, n, cin, cout, k), (cin, cout, k, B, n)
                assert got < 2 ** 27
                seen += 1
    assert seen == 5 * 39 * 4
    # the two ends of the issue: the top level at 64 x 64 / 64 members is cut into many shares, the bottom stores directly
    top, bottom = ur.uwgrad_plan(64, 64, 32, 32, 3), ur.uwgrad_plan(64, 4, 512, 512, 3)
    assert (top['tiles'], top['U'], top['ups'], top['S']) == (5, 8192, 80, 103) and not top['direct']
    assert (bottom['tiles'], bottom['U'], bottom['S']) == (576, 32, 1) and bottom['direct']


def test_declared_regimes_hold_in_the_restated_plan():
    ragged = direct = several = 0
    for (cin, cout, k, B, N), regime in ur.UCONV_REGIMES.items():
        plan = ur.uwgrad_plan(B, N, cin, cout, k)
        assert {key: plan[key] for key in regime} == regime, (cin, cout, k, B, N)
        ragged += plan['ups'] > 1 and plan['last_units'] < plan['ups']
        direct += plan['direct'] and plan['U'] > 1
        several += plan['ups'] > 1 and plan['S'] > 1
    assert ragged >= 2 and direct >= 1 and several >= 2
    # the plan's invariants: every unit in exactly one share, every pixel in exactly one unit
    for N in (2, 3, 6, 16, 64, 128):
        for B in (1, 3, 64, 256, 500):
            for c in (1, 6, 70, 512):
                for k in (1, 3):
                    p = ur.uwgrad_plan(B, N, c, c, k)
                    assert (p['S'] - 1) * p['ups'] < p['U'] <= p['S'] * p['ups'] and 1 <= p['last_units'] <= p['ups']
                    assert (p['U'] - 1) * ur.UNIT < p['P'] <= p['U'] * ur.UNIT and 1 <= p['last_pixels'] <= ur.UNIT
                    assert p['direct'] == (p['S'] == 1)


# ---- declarations and bindings ---------------------------------------------------------------------------------------
NAMES = ['qgx_uconv2d_backward_data', 'qgx_uconv2d_backward_weight', 'qgx_uconv2d_forward', 'qgx_uconv2d_workspace']


def test_header_declares_what_uconv_train_symbols_binds():
    from pyqg_generative_amd import _lib
    assert '#include "qgx_uconv_train.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_uconv_train.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.UCONV_TRAIN_SYMBOLS) == NAMES
    for name, _, args in _lib.UCONV_TRAIN_SYMBOLS:
        proto = re.search(rf'\b{name}\((.*?)\);', code, flags=re.S).group(1)
        assert len(args) == len(proto.split(',')), name
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    others = (_lib.SYMBOLS + _lib.ARCH_SYMBOLS + _lib.STATS_SYMBOLS + _lib.TRAIN_SYMBOLS + _lib.CONV_TRAIN_SYMBOLS + _lib.HEAD_TRAIN_SYMBOLS
              + _lib.FLUX_TRAIN_SYMBOLS + _lib.LATENT_TRAIN_SYMBOLS + _lib.DCONV_TRAIN_SYMBOLS)
    assert not set(NAMES) & {n for n, _, _ in others}
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'uconv_train.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_uconv_train.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()


# ---- refusals --------------------------------------------------------------------------------------------------------
GOOD = dict(B=3, N=6, cin=5, cout=7, k=3)
BAD_FIELDS = [('N', v) for v in (0, 1, 129, -2)] + [('k', v) for v in (0, 2, 5)] + [('cin', v) for v in (0, 513)] + \
             [('cout', v) for v in (0, 1025)] + [('B', v) for v in (0, 2 ** 29 // 36 + 1, 2 ** 62)]
ORDER = ('B', 'N', 'cin', 'cout', 'k')


def _workspace_bytes(**kw):
    from pyqg_generative_amd._lib import lib
    s = dict(GOOD, **kw)
    n = C.c_size_t(0)
    rc = lib.qgx_uconv2d_workspace(*(s[f] for f in ORDER), C.byref(n))
    return rc, n.value


def _calls(lib):
    """name -> (function, its pointer arguments in order, which of them may be NULL)"""
    return {
        'qgx_uconv2d_forward': (lib.qgx_uconv2d_forward, ['x_dev', 'w_dev', 'bias_dev', 'y_dev'], {'bias_dev'}),
        'qgx_uconv2d_backward_data': (lib.qgx_uconv2d_backward_data, ['dy_dev', 'w_dev', 'dx_dev'], set()),
        'qgx_uconv2d_backward_weight': (lib.qgx_uconv2d_backward_weight, ['x_dev', 'dy_dev', 'dw_dev', 'db_dev'], {'db_dev'}),
    }


def test_workspace_is_a_function_of_the_shape_alone():
    rc, n = _workspace_bytes()
    assert rc == 0 and n > 0 and n % 16 == 0
    assert _workspace_bytes() == (0, n)
    # the widest layer, the largest grid, the smallest grid with the largest batch
    assert _workspace_bytes(B=1, N=128, cin=512, cout=1024)[0] == 0
    assert _workspace_bytes(B=2 ** 27, N=2, cin=1, cout=1, k=1)[0] == 0
    assert _workspace_bytes(B=2 ** 29 // 36)[0] == 0


@pytest.mark.parametrize('field,value', BAD_FIELDS)
def test_every_out_of_range_field_is_refused(field, value):
    from pyqg_generative_amd._lib import lib
    fake = C.c_void_p(4096)       # never dereferenced: every call below must be refused first
    s = dict(GOOD, **{field: value})
    shape = tuple(s[f] for f in ORDER)
    n = C.c_size_t(0)
    assert lib.qgx_uconv2d_workspace(*shape, C.byref(n)) == -1
    assert (field + ' = ').encode() in lib.qgx_last_error()
    big = 1 << 40
    for name, (fn, ptrs, _) in _calls(lib).items():
        assert fn(*[fake] * len(ptrs), *shape, fake, big, None) == -1
        msg = lib.qgx_last_error()
        assert name.encode() in msg and (field + ' = ').encode() in msg, msg


def test_null_pointers_misalignment_and_a_short_workspace_are_refused():
    from pyqg_generative_amd._lib import lib
    fake, odd = C.c_void_p(4096), C.c_void_p(4100)
    shape = tuple(GOOD[f] for f in ORDER)
    assert lib.qgx_uconv2d_workspace(*shape, None) == -1
    rc, need = _workspace_bytes()
    for name, (fn, ptrs, optional) in _calls(lib).items():
        for i, p in enumerate(ptrs):
            for bad in (None, odd):
                if bad is None and p in optional:
                    continue                 # an optional pointer may be NULL: nothing to refuse (the GPU test runs it)
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
