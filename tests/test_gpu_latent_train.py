"""GPU: the latent step of include/qgx_latent_train.h (csrc/latent_train.hip) against tests/latent_restatement.py.

Shapes (B, N, rows of x), with eps given (latent_restatement.LATENT_REGIMES states each one's regime as data, and _run asserts it
against the restated plan before it launches): (3, 16) with a permuted idx into 5 rows — 768 pixels, 192 quads: one block of
which a quarter of the lanes has nothing to do; (1, 48): a grid that is no power of two, three blocks, the last of one wave;
(2, 96): 18 full blocks; (17, 128): 278 528 pixels, more than 1024 * 256, so a lane takes two quads.

Bounds.  Elementwise (dec_in, d_enc): 16 * 2^-24 * A, with A the float64 value of the expression with every term replaced by
its magnitude: the longest expression, d_logvar, has at most eight float32 roundings on such terms, counting an expf of 2 ulp,
and 16 doubles that count.  The three statistics are float64 sums of float32 terms: 2^-24 * sum |term|.  The x channels are
copied exactly and the pad channels are zero.  Outputs are prefilled with NaN between guard bands (tests/redzone.py), and so is
the workspace.  A second call and a call on another stream give the same bits.  The drawn eps are the oracle's Philox normals
within 2e-5, the bound of the sampler tests, differ between steps and members, and the backward that draws them again has
the bits of the backward that is given them."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import latent_restatement as lr
from redzone import guarded

pytestmark = pytest.mark.gpu

SHAPES = list(lr.LATENT_REGIMES)          # (3, 16, 5), (1, 48, 1), (2, 96, 2), (17, 128, 17)
IDS = [f'B{b}-N{n}' for b, n, _ in SHAPES]
SEED, STEP = 0x1234567890ABCDEF, (3 << 32) + 7


def _dev():
    return torch.device('cuda', 0)


_CASES = {}


def _case(shape):
    """inputs and the float64 restatement of both calls, computed once per shape and shared (never modified)"""
    if shape not in _CASES:
        B, N, n = shape
        enc, x, eps, w = lr.case_data(B, N, n, 17 * B + N)
        idx = np.random.RandomState(5 + B).permutation(n)[:B].astype(np.int64) if n > B else None
        if idx is not None:
            idx[-1] = idx[0]
        c = dict(B=B, N=N, n=n, enc=enc, x=x, eps=eps, w=w, idx=idx, gout=0.375)
        c['forward'] = lr.latent_forward(enc, x, idx, eps)
        c['d_enc'], c['A_d_enc'] = lr.latent_backward(enc, eps, w, c['gout'])
        _CASES[shape] = c
    return _CASES[shape]


def _run(case, enc=True, eps=True, backward_eps=None, step=STEP, enc_values=None):
    """the two calls through the C ABI on guarded buffers -> {name: numpy} after the guard checks; enc=False: the prior;
    eps=False: drawn; backward_eps: what the backward is given (default: what the forward was)"""
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    B, N, n = case['B'], case['N'], case['n']
    plan = lr.latent_plan(B, N)
    for key, want in lr.LATENT_REGIMES.get((B, N, n), {}).items():
        assert plan[key] == want, f'{(B, N)} is no longer in its regime: {key} = {plan[key]}, declared {want}'
    dev = _dev()
    up = lambda a: torch.tensor(a).to(dev)
    x, w = up(case['x']), up(case['w'])
    enc_t = up(case['enc'] if enc_values is None else enc_values) if enc else None
    eps_t = up(case['eps']) if eps else None
    idx = None if case['idx'] is None else up(case['idx'])
    g = torch.tensor(case['gout'], dtype=torch.float64, device=dev)
    nb = C.c_size_t()
    check(lib.qgx_latent_workspace(B, N, C.byref(nb)))
    ws = guarded((nb.value,), torch.uint8, dev)
    out = dict(dec_in=guarded((B, N, N, 8), torch.float32, dev), stats=guarded((3,), torch.float64, dev),
               d_enc=guarded((B, N, N, 8), torch.float32, dev))
    ptr = lambda t: None if t is None else t.data_ptr()
    st = current_stream_ptr()
    check(lib.qgx_latent_forward(ptr(enc_t), x.data_ptr(), ptr(idx), ptr(eps_t), SEED, step, out['dec_in'].t.data_ptr(),
                                 out['stats'].t.data_ptr() if enc else None, B, N, n, ws.t.data_ptr() if enc else None,
                                 nb.value if enc else 0, st))
    if enc:
        be = eps_t if backward_eps is None else (up(backward_eps) if backward_eps is not False else None)
        check(lib.qgx_latent_backward(enc_t.data_ptr(), ptr(be), SEED, step, w.data_ptr(), g.data_ptr(), out['d_enc'].t.data_ptr(),
                                      B, N, st))
    torch.cuda.current_stream().synchronize()
    ws.check(what='workspace')
    res = {}
    for name, buf in out.items():
        if enc:
            buf.check(written=True, what=name)          # NaN prefill: every element was written, pad channels included
        else:
            buf.check(written=name == 'dec_in', what=name)
            if name != 'dec_in':
                assert buf.unwritten() == buf.t.numel(), f'{name}: the prior wrote it'
        res[name] = buf.t.cpu().numpy().copy()
    return res


WORST = {}


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_both_calls_against_the_restatement(shape):
    case = _case(shape)
    B, N = case['B'], case['N']
    got, f = _run(case), case['forward']
    rows = lr.rows(case['idx'], B)
    # x is copied exactly, the pad channels are zero
    assert np.array_equal(cr.from_layout(got['dec_in'], 4)[:, :2], case['x'][rows])
    assert not got['dec_in'][..., 4:].any() and not got['d_enc'][..., 4:].any()
    ratios = {}
    for name, want, A in (('dec_in', f['dec_in'], f['A_dec_in']), ('d_enc', case['d_enc'], case['A_d_enc'])):
        assert got[name].shape == want.shape and np.isfinite(got[name]).all()
        err, live = np.abs(got[name].astype(np.float64) - want)[..., 2 if name == 'dec_in' else 0:4], A[..., 2 if name == 'dec_in' else 0:4]
        assert (live > 0).all()
        ratios[name] = float((err / (lr.ELEMENTWISE * live)).max())
    for k, name in enumerate(('loss_KL', 'var_latent', 'var_aggr')):
        ratios[name] = float(abs(got['stats'][k] - f['stats'][k]) / f['stat_bounds'][k])
    WORST[shape] = ratios
    print('\n  ' + '   '.join(f'{k} {v:.3f}' for k, v in ratios.items()) + '   (error / bound)')
    assert f['stats'][0] > 0 and f['stats'][2] > f['stats'][1] > 0
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_same_bits_again_and_on_another_stream(shape):
    case = _case(shape)
    runs = []
    for eps in (True, False):
        a, b = _run(case, eps=eps), _run(case, eps=eps)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            c = _run(case, eps=eps)
        torch.cuda.current_stream().wait_stream(st)
        bits = lambda v: v.view(np.int64 if v.dtype == np.float64 else np.int32)
        for name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), f'{name}: a second call gave other bits'
            assert np.array_equal(bits(a[name]), bits(c[name])), f'{name}: another stream gave other bits'
        runs.append(a)
    assert not np.array_equal(runs[0]['dec_in'], runs[1]['dec_in'])          # the drawn eps are not the given ones


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[IDS[0], IDS[1], IDS[3]])
def test_drawn_eps_are_the_oracles_normals(shape):
    case = _case(shape)
    B, N = case['B'], case['N']
    zero = np.zeros_like(case['enc'])
    got = _run(case, eps=False, enc_values=zero)
    z = cr.from_layout(got['dec_in'], 4)[:, 2:]                   # expf(0) = 1: channels 2, 3 ARE the normals
    want = lr.normals(SEED, STEP, B, N)
    assert np.abs(z.astype(np.float64) - want).max() <= 2e-5
    assert abs(float(z.mean())) < 5 / np.sqrt(z.size) and abs(float(z.std()) - 1) < 5 / np.sqrt(z.size)
    if B > 1:
        assert not np.array_equal(z[0], z[1])
    other = cr.from_layout(_run(case, eps=False, enc_values=zero, step=STEP + 1)['dec_in'], 4)[:, 2:]
    assert not np.array_equal(z, other) and np.abs(other.astype(np.float64) - lr.normals(SEED, STEP + 1, B, N)).max() <= 2e-5
    # the prior call gives the same bits and writes no statistics
    prior = _run(case, enc=False, eps=False)
    assert np.array_equal(prior['dec_in'].view(np.int32), got['dec_in'].view(np.int32))
    # KL of the prior against itself is zero, var_latent one and var_aggr one
    assert got['stats'][0] == 0 and got['stats'][1] == 1 and got['stats'][2] == 1
    # the backward that draws eps again has the bits of the backward given the eps read back from the forward
    drawn = _run(case, eps=False)
    sd = np.exp(0.5 * cr.from_layout(case['enc'], 4)[:, 2:].astype(np.float64))
    given = _run(case, eps=False, backward_eps=np.ascontiguousarray(z))
    assert np.array_equal(drawn['d_enc'].view(np.int32), given['d_enc'].view(np.int32))
    assert np.array_equal(drawn['dec_in'].view(np.int32), given['dec_in'].view(np.int32)) and np.abs(drawn['d_enc']).max() > 0
    zz = cr.from_layout(drawn['dec_in'], 4)[:, 2:].astype(np.float64)
    mu = cr.from_layout(case['enc'], 4)[:, :2].astype(np.float64)
    A = np.abs(z.astype(np.float64)) * sd + np.abs(mu)
    assert (np.abs(zz - (z.astype(np.float64) * sd + mu)) <= lr.ELEMENTWISE * A).all()


def test_latent_sample_under_autograd():
    """tools/train_ops.py's surface: latent_sample through torch.autograd against float64 torch of the loss as the reference
    writes it, within the kernels' bounds; the cached workspace, the launch counters, the prior, the facade's refusals"""
    from pyqg_generative_amd.tools import train_ops as T
    case = _case(SHAPES[0])
    B, N, gout = case['B'], case['N'], case['gout']
    dev = _dev()
    enc, x, eps, w = (torch.tensor(case[k]).to(dev) for k in ('enc', 'x', 'eps', 'w'))
    idx = torch.tensor(case['idx']).to(dev)
    # float64 torch on the CPU
    et = torch.tensor(cr.from_layout(case['enc'], 4), dtype=torch.float64, requires_grad=True)
    z, loss_KL, var_latent, var_aggr = lr.latent_torch(et, torch.tensor(case['eps'], dtype=torch.float64))
    wz = torch.tensor(cr.from_layout(case['w'], 4)[:, 2:], dtype=torch.float64)
    ((wz * z).sum() + gout * loss_KL).backward()
    for given in (eps, None):
        ed = enc.clone().requires_grad_(True)
        before = dict(T.LATENT_LAUNCHES)
        dec_in, kl, vl, va = T.latent_sample(ed, x, idx, SEED, STEP, given)
        assert dec_in.shape == (B, N, N, 8) and dec_in.requires_grad and kl.requires_grad and not vl.requires_grad and not va.requires_grad
        assert all(t.dtype == torch.float64 and t.dim() == 0 for t in (kl, vl, va))
        ((w * dec_in).sum() + gout * kl).backward()
        assert [T.LATENT_LAUNCHES[k] - before[k] for k in ('forward', 'backward', 'prior')] == [1, 1, 0]
        if given is None:
            assert np.array_equal(dec_in.detach().cpu().numpy()[..., :2], cr.to_layout(case['x'][case['idx']])[..., :2])
            continue
        f = case['forward']
        for got, k in ((kl, 0), (vl, 1), (va, 2)):
            assert abs(float(got.detach()) - f['stats'][k]) <= f['stat_bounds'][k]
        assert float(kl.detach()) == pytest.approx(float(loss_KL.detach()), rel=1e-6)
        assert float(va.detach()) == pytest.approx(float(var_aggr.detach()), rel=1e-6)
        assert (np.abs(dec_in.detach().cpu().numpy() - f['dec_in']) <= lr.ELEMENTWISE * f['A_dec_in']).all()
        # torch's gradient differs from the restatement's by the float32 rounding of the scale alone, and 0.375 / 3 is exact
        grad = ed.grad.cpu().numpy().astype(np.float64)
        assert (np.abs(grad - cr.to_layout(et.grad.numpy())) <= lr.ELEMENTWISE * case['A_d_enc'] + 1e-12).all()
        assert not grad[..., 4:].any()
    # only the KL term, and only the sample, are fine too
    ed = enc.clone().requires_grad_(True)
    T.latent_sample(ed, x, idx, SEED, STEP, eps)[1].backward()
    assert torch.isfinite(ed.grad).all() and float(ed.grad[..., :4].abs().max()) > 0
    n = len(T._WORK)
    T.latent_sample(enc, x, idx, SEED, STEP, eps)
    assert len(T._WORK) == n
    before = dict(T.LATENT_LAUNCHES)
    prior = T.latent_prior(x, idx, SEED, STEP)
    assert T.LATENT_LAUNCHES['prior'] - before['prior'] == 1 and not prior.requires_grad
    assert np.abs(cr.from_layout(prior.cpu().numpy(), 4)[:, 2:] - lr.normals(SEED, STEP, B, N)).max() <= 2e-5
    assert T.latent_prior(x, None, SEED, STEP).shape == (case['n'], N, N, 8)
    with pytest.raises(ValueError, match='do not fit'):
        T.latent_sample(enc, x, idx[:2], SEED, STEP, eps)
    with pytest.raises(ValueError, match='eps'):
        T.latent_sample(enc, x, idx, SEED, STEP, eps[:2])
    with pytest.raises(ValueError, match='int64'):
        T.latent_sample(enc, x, idx.to(torch.int32), SEED, STEP)
    with pytest.raises(ValueError, match='seed'):
        T.latent_sample(enc, x, idx, -1, STEP)
    with pytest.raises(ValueError, match='engine layout'):
        T.latent_sample(x, x, idx, SEED, STEP)
