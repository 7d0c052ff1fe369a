"""GPU: the discriminator's stride-2 convolution of include/qgx_dconv_train.h (csrc/dconv_train.hip) against the float64
restatement of tests/dconv_train_restatement.py: exact on integer data, within the a-priori float32 bound on Gaussian data,
zero pad channels, the same bits on a second call and on another stream, a stale workspace, and every output and the workspace
between guard bands (tests/redzone.py).

The cases that are here for a regime of the weight gradient (a share of more than one unit, a ragged last share, a partial last
unit) declare it as data (DCONV_REGIMES there); _run asserts it against the restated plan before it launches, and
tests/test_dconv_train_cpu.py pins that plan to the library."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import dconv_train_restatement as dr
from redzone import guarded

pytestmark = pytest.mark.gpu

# (cin, cout, B, N)
CASES = [(1, 1, 1, 2), (32, 64, 2, 2),          # a 1 x 1 output: every tap but four reads padding
         (16, 32, 2, 4), (8, 16, 2, 8),
         (6, 8, 3, 16),                         # the first layer's pad channels
         (33, 7, 2, 6),                         # an odd output size, ragged channel counts
         (40, 70, 1, 12),
         (260, 512, 1, 4)]                      # beyond conv_train's 256 channels
CASES += [(8, 8, 2, N) for N in (24, 32, 48, 64, 96, 128)]
CASES += [c for c in dr.DCONV_REGIMES if c not in CASES]
IDS = ['cin%d-cout%d-B%d-N%d' % c for c in CASES]


def _dev():
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _data(case, integer):
    cin, cout, B, N = case
    arrays = dr.case_data(cin, cout, B, N, 2000 + 7 * cin + cout + B + N, integer)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _truth(case, integer, absolute=False):
    """float64 y, dx, dw of the case (absolute: of the operands' magnitudes — the bound's scale); computed once, read-only"""
    cin, cout, B, N = case
    x, w, dy = (np.abs(a) if absolute else a for a in _data(case, integer))
    out = (dr.forward(x, w), dr.backward_data(dy, w, N), dr.backward_weight(x, dy, cin, cout))
    for a in out:
        a.setflags(write=False)
    return out


def _assert_regime(case):
    cin, cout, B, N = case
    plan = dr.dwgrad_plan(B, N, cin, cout)
    for key, want in dr.DCONV_REGIMES.get(case, {}).items():
        assert plan[key] == want, f'{case} is no longer in its regime: {key} = {plan[key]}, declared {want}'


def _run(case, integer, guard=True, ws_fill=0xFF):
    """the three calls through the C ABI on guarded buffers -> (y, dx, dw) as numpy, after the guard checks"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    _assert_regime(case)
    cin, cout, B, N = case
    x, w, dy = (torch.as_tensor(a).to(_dev()) for a in _data(case, integer))
    n = C.c_size_t()
    check(lib.qgx_dconv2d_workspace(B, N, cin, cout, C.byref(n)))
    assert n.value == dr.workspace_bytes(B, N, cin, cout)
    ws = guarded((n.value,), torch.uint8, _dev(), fill=ws_fill)
    y = guarded((B, N // 2, N // 2, cr.c8(cout)), torch.float32, _dev())
    dx = guarded((B, N, N, cr.c8(cin)), torch.float32, _dev())
    dw = guarded((cout, cin, 4, 4), torch.float32, _dev())
    shape = (B, N, cin, cout)
    st = current_stream_ptr()
    check(lib.qgx_dconv2d_forward(x.data_ptr(), w.data_ptr(), y.t.data_ptr(), *shape, ws.t.data_ptr(), n.value, st))
    check(lib.qgx_dconv2d_backward_data(dy.data_ptr(), w.data_ptr(), dx.t.data_ptr(), *shape, ws.t.data_ptr(), n.value, st))
    check(lib.qgx_dconv2d_backward_weight(x.data_ptr(), dy.data_ptr(), dw.t.data_ptr(), *shape, ws.t.data_ptr(), n.value, st))
    torch.cuda.synchronize()
    if guard:
        ws.check(what='workspace')
        for g, name in ((y, 'y'), (dx, 'dx'), (dw, 'dw')):
            g.check(written=True, what=name)
    return tuple(g.t.cpu().numpy() for g in (y, dx, dw))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_exact_on_integers(case):
    """x, w, dy integers in -3 ... 3: every product and partial sum is an integer below 2^24 (asserted from the restatement of
    |operands|, whose entries bound every partial sum), float32 arithmetic is exact in any order, and the results must EQUAL the
    float64 restatement — a dropped, doubled or misplaced term shows"""
    got = _run(case, True)
    for name, g, t, ta in zip(('y', 'dx', 'dw'), got, _truth(case, True), _truth(case, True, True)):
        assert ta.max() < 2 ** 24
        bad = np.argwhere(g.astype(np.float64) != t)
        assert bad.size == 0, f'{name}: {len(bad)} of {t.size} elements differ, first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {t[tuple(bad[0])]}'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_rounding_class_on_gaussian_data(case):
    """|result - truth64| <= (K + 2) 2^-24 truth64(|operands|) elementwise, K the number of summed terms (16 cin, 4 cout,
    B (N/2)^2): the a-priori bound of a float32 sum in any order.  The largest ratio to the bound is printed."""
    cin, cout, B, N = case
    got = _run(case, False)
    K = dict(y=16 * cin, dx=4 * cout, dw=B * (N // 2) ** 2)
    worst = {}
    for name, g, t, ta in zip(('y', 'dx', 'dw'), got, _truth(case, False), _truth(case, False, True)):
        bound = (K[name] + 2) * 2.0 ** -24 * ta
        err = np.abs(g.astype(np.float64) - t)
        live = bound > 0
        assert not err[~live].any(), name                       # pad channels: a zero bound, a zero result
        worst[name] = float((err[live] / bound[live]).max())
    print('\n%s: largest error / bound  ' % (case,) + '  '.join(f'{n} {v:.4f}' for n, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_pad_channels_are_zero(case):
    cin, cout, B, N = case
    for integer in (True, False):
        y, dx, _ = _run(case, integer, guard=False)
        assert y.shape == (B, N // 2, N // 2, cr.c8(cout)) and dx.shape == (B, N, N, cr.c8(cin))
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
    for name, a, b, c in zip(('y', 'dx', 'dw'), first, second, third):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), f'{name}: a second call gave other bits'
        assert np.array_equal(a.view(np.int32), c.view(np.int32)), f'{name}: another stream gave other bits'


STALE = [(40, 70, 1, 12), (8, 72, 500, 6), (260, 512, 1, 4)]


@pytest.mark.parametrize('case', STALE, ids=[IDS[CASES.index(c)] for c in STALE])
def test_a_stale_workspace_changes_nothing(case):
    """the workspace's previous contents (NaN patterns, zeros) do not enter a result; the case with ups = 2 covers the slices a
    workgroup writes after its later units"""
    want = _run(case, False, guard=False)
    for fill in (0x00, 0x7F):
        got = _run(case, False, ws_fill=fill)
        for name, a, b in zip(('y', 'dx', 'dw'), want, got):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, case, fill)


def test_strided_conv2d_is_twice_differentiable():
    """the three Functions of tools/train_ops.py against torch CPU double backward of F.conv2d(stride=2, padding=1) in float64:
    with a(y) = leaky_relu(y, 0.2) + y^2 / 2 and s = sum(a(conv(x, w)) c), the gradient of |ds/dx|^2 with respect to w and x —
    a once-differentiable Function gives no graph here.  Margin: 8 x the deviation of the float32 CPU evaluation of the same
    statement from the float64 one, per tensor, relative to its largest magnitude, with a floor of 2^-22."""
    import torch.nn.functional as F
    from pyqg_generative_amd.tools import train_ops
    cin, cout, B, N = 6, 8, 3, 16
    x, w, dy = _data((cin, cout, B, N), False)

    def statement(conv, xe, wt, c):
        y = conv(xe, wt)
        s = ((F.leaky_relu(y, 0.2) + 0.5 * y * y) * c).sum()
        gx, = torch.autograd.grad(s, xe, create_graph=True)
        gw2, gx2 = torch.autograd.grad((gx ** 2).sum(), (wt, xe))
        return y.detach(), gx.detach(), gw2, gx2

    def on_cpu(dtype):
        xe = torch.tensor(cr.from_layout(x, cin), dtype=dtype, requires_grad=True)
        wt = torch.tensor(w, dtype=dtype, requires_grad=True)
        c = torch.tensor(cr.from_layout(dy, cout), dtype=dtype)
        y, gx, gw2, gx2 = statement(lambda a, b: F.conv2d(a, b, None, stride=2, padding=1), xe, wt, c)
        return [cr.to_layout(y.numpy()), cr.to_layout(gx.numpy()), gw2.numpy(), cr.to_layout(gx2.numpy())]

    xe = torch.as_tensor(x).to(_dev()).requires_grad_(True)
    wt = torch.as_tensor(w).to(_dev()).requires_grad_(True)
    before = dict(train_ops.DCONV_LAUNCHES)
    got = [t.cpu().numpy() for t in statement(train_ops.strided_conv2d, xe, wt, torch.as_tensor(dy).to(_dev()))]
    print({k: train_ops.DCONV_LAUNCHES[k] - before[k] for k in before})
    want, f32 = on_cpu(torch.float64), on_cpu(torch.float32)
    for name, g, t, f in zip(('y', 'dx', 'd2/dw', 'd2/dx'), got, want, f32):
        scale = np.abs(t).max()
        assert scale > 0, name
        err, ref = np.abs(g - t).max() / scale, np.abs(f - t).max() / scale
        print(f'{name}: device {err:.3e}, float32 CPU {ref:.3e} of the largest magnitude')
        assert err <= max(8 * ref, 2.0 ** -22), name
