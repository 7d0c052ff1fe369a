"""GPU: the batch gather and the loss head of include/qgx_head_train.h (csrc/train_head.hip) against tests/head_restatement.py:
EXACT on integer data in MSE mode, softplus mode against the float64 restatement with the float32 torch CPU evaluation as the
yardstick, zero pad channels in outputs prefilled with NaN, the same bits on a second call and on another stream, and every
output and the workspace between guard bands (tests/redzone.py).

Shapes (B, N): the smallest (1, 16): one workgroup, one partial; (3, 16) and (5, 16): odd partial counts; (2, 48): a grid that
is no power of two, 18 partials; (1, 128): the largest pixel offset within an image.  C = 2 throughout, C = 1 and C = 8 (the
second 16-byte half of a record) at (3, 16).  Every shape runs without idx (n = B + 2 rows, the first B used) and with a
permuted idx into n = B + 2 rows that repeats a row.

More than one share per thread.  The loss is cut into nb <= 1024 partials of ppb pixels (tests/train_plan_restatement.py restates
the plan; tests/test_head_train_cpu.py pins it to the library).  Up to 65 536 pixels every thread of k_head_finish adds one
partial at the most, and up to 262 144 every thread of k_head_loss one pixel.  (257, 16): 257 partials, thread 0 of
k_head_finish adds two; (5, 128): 320 partials at the largest offsets within an image; (1025, 16) with C = 2 and C = 8:
ppb = 512 — the second pass of k_head_loss — with 513 partials, the last of 256 pixels only.  These shapes declare their regime
as data (HEAD_REGIMES there) and _run asserts it against the restated plan before it launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import head_restatement as hr
import train_plan_restatement as tp
from redzone import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 2), (3, 16, 2), (5, 16, 2), (2, 48, 2), (1, 128, 2), (3, 16, 1), (3, 16, 8)]
SHAPES += list(tp.HEAD_REGIMES)          # (257, 16, 2), (5, 128, 2), (1025, 16, 2), (1025, 16, 8)
IDS = [f'B{b}-N{n}-C{c}' for b, n, c in SHAPES]
SOFTPLUS_MARGIN = 4.0


def _dev():
    return torch.device('cuda', 0)


def _idx(B, n, seed):
    """B rows of n in a shuffled order, the last one a repeat of the first (B >= 2); None for seed None"""
    if seed is None:
        return None
    idx = np.random.RandomState(seed).permutation(n)[:B].astype(np.int64)
    if B >= 2:
        idx[-1] = idx[0]
    return idx


_CASES = {}


def _case(shape, integer, with_idx):
    """inputs and the float64 restatement of every call, computed once per case and shared (never modified)"""
    key = (shape, integer, with_idx)
    if key not in _CASES:
        B, N, Cn = shape
        n = B + 2
        y, src, t = hr.case_data(B, N, Cn, n, 17 * B + N + Cn, integer)
        idx = _idx(B, n, 5 + B if with_idx else None)
        _CASES[key] = dict(B=B, N=N, C=Cn, n=n, y=y, src=src, t=t, idx=idx)
    return _CASES[key]


def _run(case, mode, gout=1.0, stream=None):
    """the five calls through the C ABI on guarded buffers -> {name: numpy} after the guard checks"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    B, N, Cn, n = case['B'], case['N'], case['C'], case['n']
    plan = tp.head_plan(B, N)
    for key, want in tp.HEAD_REGIMES.get((B, N, Cn), {}).items():
        assert plan[key] == want, f'{(B, N, Cn)} is no longer in its regime: {key} = {plan[key]}, declared {want}'
    m = hr.MODES[mode]
    dev = _dev()
    y, src, t = (torch.tensor(case[k]).to(dev) for k in ('y', 'src', 't'))
    idx = None if case['idx'] is None else torch.tensor(case['idx']).to(dev)
    ip = None if idx is None else idx.data_ptr()
    g = torch.tensor(gout, dtype=torch.float64, device=dev)
    nb = C.c_size_t()
    check(lib.qgx_head_workspace(B, N, C.byref(nb)))
    ws = guarded((nb.value,), torch.uint8, dev)
    out = dict(gather=guarded((B, N, N, 8), torch.float32, dev), loss=guarded((1,), torch.float64, dev),
               dy=guarded((B, N, N, 8), torch.float32, dev), forward=guarded((B, Cn, N, N), torch.float32, dev),
               residual=guarded((B, Cn, N, N), torch.float32, dev))
    st = current_stream_ptr()
    check(lib.qgx_batch_gather(src.data_ptr(), ip, out['gather'].t.data_ptr(), n, B, N, Cn, st))
    check(lib.qgx_head_loss(y.data_ptr(), t.data_ptr(), ip, m, out['loss'].t.data_ptr(), B, N, Cn, n, ws.t.data_ptr(), nb.value, st))
    check(lib.qgx_head_grad(y.data_ptr(), t.data_ptr(), ip, m, g.data_ptr(), out['dy'].t.data_ptr(), B, N, Cn, n, st))
    check(lib.qgx_head_apply(y.data_ptr(), None, None, m, out['forward'].t.data_ptr(), B, N, Cn, 0, st))
    check(lib.qgx_head_apply(y.data_ptr(), t.data_ptr(), ip, m, out['residual'].t.data_ptr(), B, N, Cn, n, st))
    torch.cuda.current_stream().synchronize()
    ws.check(what='workspace')
    res = {}
    for name, buf in out.items():
        buf.check(written=True, what=name)          # NaN prefill: every element was written, pad channels included
        res[name] = buf.t.cpu().numpy().copy()
    return res


def _want(case, mode, gout=1.0):
    y, t, idx, Cn = case['y'], case['t'], case['idx'], case['C']
    return dict(gather=hr.batch_gather(case['src'], idx, case['B']).astype(np.float64), loss=np.array([hr.head_loss(y, t, idx, mode)]),
                dy=hr.head_grad(y, t, idx, mode, gout), forward=hr.head_apply(y, None, None, mode, Cn),
                residual=hr.head_apply(y, t, idx, mode, Cn))


@pytest.mark.parametrize('with_idx', [False, True], ids=['rows', 'idx'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_mse_mode_is_exact_on_integers(shape, with_idx):
    case = _case(shape, True, with_idx)
    for gout in (1.0, 0.375):
        got, want = _run(case, 'mse', gout), _want(case, 'mse', gout)
        for name in ('gather', 'loss', 'forward', 'residual'):
            assert got[name].shape == want[name].shape
            assert np.array_equal(got[name].astype(np.float64), want[name]), name
        # the float32 scale times an integer difference is exact in float64: the device's float32 product rounds it once
        assert np.array_equal(got['dy'], want['dy'].astype(np.float32)), f'dy, gout = {gout}'
        for name in ('gather', 'dy'):
            assert not got[name][..., shape[2]:].any(), f'{name}: pad channels'
    assert want['loss'][0] > 0 and np.abs(want['dy']).max() > 0


def _rel(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / np.abs(truth).max())


def _torch_f32(case):
    """the float32 torch CPU evaluation of the softplus head's expressions"""
    import torch.nn.functional as F
    Cn, B = case['C'], case['B']
    yt = torch.tensor(cr.from_layout(case['y'], Cn), requires_grad=True)
    tt = torch.tensor(case['t'])[hr.rows(case['idx'], B)]
    h = F.softplus(yt)
    loss = F.mse_loss(h, tt)
    loss.backward()
    return dict(loss=np.array([float(loss.detach())]), dy=cr.to_layout(yt.grad.numpy()), forward=h.detach().numpy(),
                residual=((tt - h) ** 2).detach().numpy())


@pytest.mark.parametrize('with_idx', [False, True], ids=['rows', 'idx'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_softplus_mode_within_four_times_float32_torch(shape, with_idx):
    case = _case(shape, False, with_idx)
    assert np.abs(case['y']).max() == 30 and case['y'].min() == -30 and (case['y'] == 20).any()
    got, want, cpu = _run(case, 'softplus_mse'), _want(case, 'softplus_mse'), _torch_f32(case)
    assert np.array_equal(got['gather'].astype(np.float64), want['gather'])
    assert not got['dy'][..., shape[2]:].any() and np.isfinite(got['dy']).all()
    print()
    worst = {}
    for name in ('loss', 'dy', 'forward', 'residual'):
        worst[name] = (_rel(got[name], want[name]), _rel(cpu[name], want[name]))
        print(f'  {name:9s} device {worst[name][0]:.2e}   float32 torch CPU {worst[name][1]:.2e}')
    for name, (dev, ref) in worst.items():
        assert dev <= SOFTPLUS_MARGIN * ref, (name, dev, ref)


@pytest.mark.parametrize('shape', [SHAPES[2], SHAPES[3], SHAPES[6], (1025, 16, 2)], ids=[IDS[2], IDS[3], IDS[6], 'B1025-N16-C2'])
def test_same_bits_again_and_on_another_stream(shape):
    case = _case(shape, False, True)
    a, b = _run(case, 'softplus_mse', 0.375), _run(case, 'softplus_mse', 0.375)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = _run(case, 'softplus_mse', 0.375)
    torch.cuda.current_stream().wait_stream(st)
    for name in a:
        bits = lambda v: v.view(np.int64 if v.dtype == np.float64 else np.int32)
        assert np.array_equal(bits(a[name]), bits(b[name])), f'{name}: a second call gave other bits'
        assert np.array_equal(bits(a[name]), bits(c[name])), f'{name}: another stream gave other bits'


def test_wrappers_and_autograd():
    """tools/train_CNN.py's surface: gather_batch, head_apply, and head_loss through torch.autograd (the incoming gradient is
    read on the device), the cached workspace, the refusals of the facade"""
    from pyqg_generative_amd.tools import train_ops as T
    case = _case((3, 16, 2), True, True)
    dev = _dev()
    y, src, t = (torch.tensor(case[k]).to(dev) for k in ('y', 'src', 't'))
    idx = torch.tensor(case['idx']).to(dev)
    assert np.array_equal(T.gather_batch(src, idx).cpu().numpy(), hr.batch_gather(case['src'], case['idx']))
    assert np.array_equal(T.gather_batch(src).cpu().numpy(), cr.to_layout(case['src']))
    # a misaligned index vector (an odd offset into an epoch's order) is taken too
    shifted = torch.cat([idx[:1], idx])[1:]
    assert shifted.data_ptr() % 16 == 8
    assert np.array_equal(T.gather_batch(src, shifted).cpu().numpy(), hr.batch_gather(case['src'], case['idx']))
    for mode in ('mse', 'softplus_mse'):
        yd = y.clone().requires_grad_(True)
        before = dict(T.HEAD_LAUNCHES)
        loss = T.head_loss(yd, t, idx, mode)
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad
        (loss * 0.375).backward()
        assert T.HEAD_LAUNCHES['loss'] - before['loss'] == 1 and T.HEAD_LAUNCHES['grad'] - before['grad'] == 1
        if mode == 'mse':
            assert float(loss.detach()) == hr.head_loss(case['y'], case['t'], case['idx'], mode)
            assert np.array_equal(yd.grad.cpu().numpy(), hr.head_grad(case['y'], case['t'], case['idx'], mode, 0.375).astype(np.float32))
            assert np.array_equal(T.head_apply(y, 2, mode, T=t, idx=idx).cpu().numpy().astype(np.float64),
                                  hr.head_apply(case['y'], case['t'], case['idx'], mode, 2))
            assert np.array_equal(T.head_apply(y, 2, mode).cpu().numpy(), cr.from_layout(case['y'], 2))
        else:
            assert float(loss.detach()) == pytest.approx(hr.head_loss(case['y'], case['t'], case['idx'], mode), rel=1e-6)
            assert yd.grad.shape == y.shape and not yd.grad[..., 2:].any()
    n = len(T._WORK)
    T.head_loss(y, t, idx, 'mse')
    assert len(T._WORK) == n
    with pytest.raises(ValueError, match='head'):
        T.head_loss(y, t, idx, 'softplus')
    with pytest.raises(ValueError, match='do not fit'):
        T.head_loss(y, t, idx[:2], 'mse')
    with pytest.raises(ValueError, match='int64'):
        T.gather_batch(src, idx.to(torch.int32))
    with pytest.raises(ValueError, match='engine layout'):
        T.head_loss(src, t, idx, 'mse')
