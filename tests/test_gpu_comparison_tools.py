"""GPU: tools/comparison_tools.py — the exact 1-Wasserstein distance of csrc/metrics.hip against
scipy.stats.wasserstein_distance (sizes around the tile and merge-block sizes, float32 / float64, signed zeros, ties,
skewed exponents), its determinism, non-finite inputs and 64-bit indexing; and diagnostic_differences_Perezhogin
against oracle/metrics_ref.py on runs of this engine."""
import os

import numpy as np
import pytest
import torch
from scipy.stats import wasserstein_distance as scipy_w1

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _ct():
    from pyqg_generative_amd.tools import comparison_tools
    return comparison_tools


def _check(u, v, tol=1e-11):
    got = _ct().wasserstein_distance(u, v)
    want = scipy_w1(np.asarray(u, dtype='float64').ravel(), np.asarray(v, dtype='float64').ravel())
    if want == 0:
        assert got == 0.0, (got, want)
    else:
        assert abs(got - want) <= tol * abs(want), (got, want, abs(got - want) / abs(want))
    return got


SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (255, 257), (4095, 4097), (4096, 8192), (8191, 8193), (12345, 54321),
         (4_000_000, 3_000_001)]


@pytest.mark.parametrize('nu,nv', SIZES)
@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_w1_matches_scipy(nu, nv, dtype):
    rs = np.random.RandomState(nu + 7 * nv)
    u = (rs.randn(nu) * 3 - 0.5).astype(dtype)
    v = (rs.standard_t(3, nv) * 2 + 0.25).astype(dtype)
    _check(u, v)


def test_w1_signed_zeros_ties_and_identical_multisets():
    rs = np.random.RandomState(1)
    z = np.array([0.0, -0.0] * 500 + [1.0, -1.0] * 10)
    _check(z, rs.permutation(z) * 0.5)
    _check(z, -z[::-1].copy())
    q = np.round(rs.randn(200_001) * 4) / 4              # heavy ties: 1/4-quantised
    r = np.round(rs.randn(150_000) * 4 + 0.3) / 4
    _check(q, r)
    _check(q.astype('float32'), r.astype('float32'))
    for a in (q, rs.randn(9000), np.array([3.5])):
        assert _ct().wasserstein_distance(a, rs.permutation(a)) == 0.0
    assert _ct().wasserstein_distance(z, -z) == 0.0      # the multisets agree: -0.0 == 0.0


def test_w1_skewed_exponents():
    rs = np.random.RandomState(2)
    u = 10 ** rs.uniform(-12, -2, 500_000)               # KE-like
    v = 10 ** rs.uniform(-11.5, -2.5, 300_000)
    _check(u, v)
    _check(u, -v)


def test_w1_mixed_precisions_and_device_tensors():
    rs = np.random.RandomState(3)
    u, v = rs.randn(70_000), rs.randn(50_000).astype('float32')
    want = _check(u, v)
    tu = torch.as_tensor(u).cuda().reshape(700, 100)
    tv = torch.as_tensor(v).cuda()
    assert _ct().wasserstein_distance(tu, tv) == want
    np.testing.assert_array_equal(tu.cpu().numpy().ravel(), u)   # the inputs are not touched


def test_w1_is_deterministic():
    rs = np.random.RandomState(4)
    u = rs.randn(1_000_003) * np.exp(rs.randn(1_000_003))
    v = rs.randn(777_777) + 0.1
    w1 = _ct().wasserstein_distance
    ref = w1(u, v)
    for _ in range(3):
        assert w1(u, v) == ref
    assert w1(rs.permutation(u), rs.permutation(v)) == ref
    tu, tv = torch.as_tensor(u).cuda(), torch.as_tensor(v).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = w1(tu, tv)
    assert got == ref


def test_w1_non_finite_inputs_give_nan():
    w1 = _ct().wasserstein_distance
    a = np.arange(10.0)
    for bad in (np.nan, np.inf, -np.inf):
        b = a.copy()
        b[3] = bad
        assert np.isnan(w1(b, a)) and np.isnan(w1(a, b))
        assert np.isnan(w1(b.astype('float32'), a.astype('float32')))


def test_w1_beyond_2_31_elements():
    """u = (p(k) mod 1024) over a bijection p of [0, 2^31 + 1024), v = 0.5, 1.5, ..., 1023.5: W1 = 0.5 exactly"""
    M = 2 ** 31 + 1024
    need = M * 4 * 3 + (M // 4096 + 1) * 256 * 12 + (1 << 28)      # values, keys, sort buffer, tile tables, slack
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free')
    a = 2147483647                  # prime, coprime with M = 2^10 (2^21 + 1)
    u = torch.empty(M, dtype=torch.float32, device='cuda')
    step = 1 << 27
    for s in range(0, M, step):
        k = torch.arange(s, min(s + step, M), dtype=torch.int64, device='cuda')
        u[s:s + k.numel()] = ((k * a + 12345) % M % 1024).to(torch.float32)
        del k
    v = torch.arange(1024, dtype=torch.float32, device='cuda') + 0.5
    assert _ct().wasserstein_distance(u, v) == 0.5
    assert _ct().wasserstein_distance(v, u) == 0.5


# ---- diagnostic_differences_Perezhogin ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def runs():
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.simulate import run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    from pyqg_generative_amd.tools.comparison_tools import coarsegrain_reference_dataset
    nets, xs, ys = weights.load_npz(os.path.join(ROOT, 'tests', 'golden', 'weights_gan.npz'), 'gan')
    gan = CGANRegression.from_arrays(nets, xs, ys)
    lo = EDDY_PARAMS.nx(48)._update({'tmax': 14400. * 240, 'tavestart': 14400. * 100, 'log_level': 0})
    hi = EDDY_PARAMS.nx(96)._update({'tmax': 7200. * 480, 'tavestart': 7200. * 200, 'log_level': 0})
    out = {
        'lores': run_simulation(dict(lo), sampling_freq=14400. * 6, n_members=3, seeds=[0, 1, 2]),
        'gan': run_simulation(dict(lo), parameterization=dict(self=gan, sampling='AR1', nsteps=1),
                              sampling_freq=14400. * 6, n_members=3, seeds=[3, 4, 5], seed=11),
        'single': run_simulation(dict(lo), sampling_freq=14400. * 6, n_members=1, seeds=[6]),
        'hires': run_simulation(dict(hi), sampling_freq=7200. * 12, n_members=2, seeds=[7, 8]),
    }
    out['target'] = coarsegrain_reference_dataset(out['hires'], 48, 'Operator1')
    return out


def _as_oracle_run(ds, T):
    """the dataset as the oracle's dict: runs x last T snapshots pooled along the first axis, run-mean spectra"""
    r = {}
    for k in ('q', 'u', 'v'):
        a = np.asarray(ds[k].values)
        a = a[None] if a.ndim == 4 else a
        a = a[:, -T:]
        r[k] = a.reshape((-1,) + a.shape[2:])
    for k in ('KEspec', 'KEflux', 'APEflux', 'APEgenspec', 'paramspec_KEflux', 'paramspec_APEflux'):
        if k in ds.data_vars:
            a = np.asarray(ds[k].values)
            r[k] = a.mean(0) if 'run' in ds[k].dims else a
    return r


def _oracle(ds1, ds2, T):
    from oracle import metrics_ref
    r1, r2 = _as_oracle_run(ds1, T), _as_oracle_run(ds2, T)
    norm = metrics_ref.diagnostic_differences(r1, r2, T_last=10 ** 9)
    diff, scale = {}, {}
    for z in (0, 1):
        f1, f2 = metrics_ref._features(r1, z, 10 ** 9), metrics_ref._features(r2, z, 10 ** 9)
        for label in ('q', 'u', 'v', 'KE', 'Ens'):
            a, b = f1[label].ravel(), f2[label].ravel()
            diff[f'distrib_diff_{label}{z + 1}'] = scipy_w1(a, b)
            scale[f'distrib_diff_{label}{z + 1}'] = float(np.sqrt(np.mean(b ** 2)))
    return norm, diff, scale


def _compare(ds1, ds2, T):
    ct = _ct()
    norm, diff, scale = ct.diagnostic_differences_Perezhogin(ds1, ds2, T=T)
    keys = [f'distrib_diff_{l}{z}' for l in ('q', 'u', 'v', 'KE', 'Ens') for z in (1, 2)] + \
        ['spectral_diff_KEspec1', 'spectral_diff_KEspec2', 'spectral_diff_Eflux', 'spectral_diff_APEgenspec']
    assert list(norm) == keys and list(diff) == keys and list(scale) == keys
    onorm, odiff, oscale = _oracle(ds1, ds2, T)
    for k in keys:
        assert np.isfinite(norm[k]) and norm[k] > 0, k
        assert abs(norm[k] - onorm[k]) <= 1e-9 * abs(onorm[k]), (k, norm[k], onorm[k])
        if k in odiff:
            assert abs(diff[k] - odiff[k]) <= 1e-9 * abs(odiff[k]), (k, diff[k], odiff[k])
            assert abs(scale[k] - oscale[k]) <= 1e-9 * abs(oscale[k]), (k, scale[k], oscale[k])
    for f in (ct.distrib_score, ct.spectral_score):
        assert np.isfinite(f(norm))
    return norm


def test_diagnostic_differences_match_oracle(runs):
    assert 'paramspec_KEflux' in runs['gan'].data_vars
    n_gan = _compare(runs['gan'], runs['target'], T=32)
    n_lores = _compare(runs['lores'], runs['target'], T=32)
    assert n_gan['spectral_diff_Eflux'] != n_lores['spectral_diff_Eflux']


def test_diagnostic_differences_single_member_and_long_T(runs):
    assert 'run' not in runs['single'].dims
    _compare(runs['single'], runs['target'], T=16)
    assert np.asarray(runs['lores']['q'].values).shape[1] < 128
    _compare(runs['lores'], runs['target'], T=128)
