"""CPU: the flow-statistics entry points of include/qgx_stats.h (declarations, bindings, argument refusals), the numpy
restatement the GPU tests compare with against an analytic flow, the netCDF readers of tools/xr_lite.py and cache_path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytest.importorskip('torch')

from conftest import ROOT


def test_header_declares_what_stats_symbols_binds():
    """include/qgx_stats.h (included by qgx.h) declares what _lib.STATS_SYMBOLS binds, and the library exports it"""
    from pyqg_generative_amd import _lib
    assert '#include "qgx_stats.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_stats.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.STATS_SYMBOLS) == ['qgx_flow_features', 'qgx_flow_features_workspace']
    assert 'int qgx_flow_features_workspace(const qgx_model *plan, int64_t S, size_t *bytes);' in code
    proto = re.search(r'int qgx_flow_features\((.*?)\);', code, flags=re.S).group(1)
    args = [a.strip() for a in proto.replace('\n', ' ').split(',')]
    assert args == ['qgx_model *plan', 'const void *u_dev', 'const void *v_dev', 'int is_double', 'int64_t S', 'double *omega_dev',
                    'void *ke_dev', 'double *ens_dev', 'void *vabs_dev', 'double *ke_sum_dev', 'void *work_dev', 'size_t work_bytes',
                    'void *stream']
    assert len(dict((n, a) for n, _, a in _lib.STATS_SYMBOLS)['qgx_flow_features']) == len(args)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    # the new source and header are part of the library's fingerprint
    mk = open(os.path.join(ROOT, 'pyqg_generative_amd', 'csrc', 'Makefile')).read()
    assert 'flow.hip' in re.search(r'^SRCS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    assert '../../include/qgx_stats.h' in re.search(r'^HDRS\s*:=\s*(.*)$', mk, flags=re.M).group(1).split()
    for doc in ('INTEGRATION.md', 'README.md'):
        assert 'qgx_flow_features' in open(os.path.join(ROOT, doc)).read()


def test_refusals_before_any_device_call():
    from pyqg_generative_amd._lib import lib
    fake = C.c_void_p(256)       # never dereferenced: every call below must be refused first
    nbytes = C.c_size_t()
    assert lib.qgx_flow_features_workspace(None, 4, C.byref(nbytes)) == -1
    assert lib.qgx_flow_features_workspace(fake, 4, None) == -1
    assert lib.qgx_flow_features_workspace(fake, 0, C.byref(nbytes)) == -1
    assert lib.qgx_flow_features_workspace(fake, -3, C.byref(nbytes)) == -1
    assert lib.qgx_flow_features_workspace(fake, 2 ** 30, C.byref(nbytes)) == -1
    assert b'qgx_flow_features_workspace' in lib.qgx_last_error()

    def call(plan=fake, u=fake, v=fake, is_double=1, S=3, outs=(fake,) * 5):
        return lib.qgx_flow_features(plan, u, v, is_double, S, *outs, fake, 1 << 30, None)
    assert call(plan=None) == -1 and call(u=None) == -1 and call(v=None) == -1
    assert call(S=0) == -1 and call(S=-1) == -1 and call(S=2 ** 30) == -1
    assert call(is_double=2) == -1 and call(is_double=-1) == -1
    assert b'is_double' in lib.qgx_last_error()
    assert call(outs=(None,) * 5) == -1
    assert b'every output is NULL' in lib.qgx_last_error()


# ---- the restatement against an analytic flow -----------------------------------------------------------------------
def _wave(N, A, mx, my, phase, L=1e6):
    """psi = A cos(k x + l y + phase) on the N x N grid: (psi, u = -psi_y, v = psi_x, K^2)"""
    k, l = 2 * np.pi * mx / L, 2 * np.pi * my / L
    x = (np.arange(N) + 0.5) * L / N
    th = k * x[None, :] + l * x[:, None] + phase
    return A * np.cos(th), A * l * np.sin(th), -A * k * np.sin(th), k * k + l * l


@pytest.mark.parametrize('N', [8, 12, 48])
def test_restatement_reproduces_an_analytic_wave(N):
    import flow_statistics_restatement as fr
    R, T, delta = 2, 3, 0.25
    u, v = np.zeros((R, T, 2, N, N)), np.zeros((R, T, 2, N, N))
    omega, ke_mean = np.zeros_like(u), np.zeros((R, T, 2))
    rs = np.random.RandomState(N)
    for r in range(R):
        for t in range(T):
            for z in range(2):
                A, ph = 1e3 * (1 + rs.rand()), rs.rand() * 6
                mx, my = rs.randint(1, N // 2), -rs.randint(1, N // 2)          # below the 2h harmonics
                psi, u[r, t, z], v[r, t, z], K2 = _wave(N, A, mx, my, ph)
                omega[r, t, z] = -K2 * psi
                ke_mean[r, t, z] = A * A * K2 / 4                                # mean of sin^2 over whole periods
    f = fr.flow_features(u, v)
    scale = np.abs(omega).max(axis=(-2, -1), keepdims=True)
    assert (np.abs(f['omega'] - omega) <= 1e-12 * scale).all()
    np.testing.assert_allclose(f['Ens'], 0.5 * omega ** 2, rtol=0, atol=2e-12 * (scale ** 2).max())
    np.testing.assert_allclose(f['KE'], 0.5 * (u * u + v * v), rtol=1e-15)
    np.testing.assert_allclose(f['Vabs'], np.hypot(u, v), rtol=1e-14)
    np.testing.assert_allclose(f['KE_sum'], ke_mean * N * N, rtol=1e-12)
    w = np.array([delta / (1 + delta), 1 / (1 + delta)])
    want = (ke_mean * w).sum(-1).mean(0)
    run = {'u': u, 'v': v, 'q': omega, 'time': np.arange(T) * 360.0}
    stats = fr.dataset_statistics(run, delta)
    np.testing.assert_allclose(stats['KE_time'], want, rtol=1e-12)
    np.testing.assert_allclose(stats['time'], np.arange(T))
    assert np.ndim(stats['Energysumr']) == 0 and stats['Energysumr'] == 0       # no diagnostics in the run
    last = fr.dataset_smart_read(run, delta, compute_all=False)
    assert 'omega' not in last and 'PDF_Ens1' not in last and last['PDF_KE2'].shape == (30,)
    np.testing.assert_allclose(last['KE_time'], want, rtol=1e-12)
    # a density integrates to the fraction of values inside the range
    x = u[:, -1:, 0]
    inside = ((x >= x.mean() - 4 * x.std()) & (x <= x.mean() + 4 * x.std())).mean()
    np.testing.assert_allclose(last['PDF_u1'].sum() * (last['u_0'][1] - last['u_0'][0]), inside, rtol=1e-12)


def test_restatement_spectra_and_budget():
    import flow_statistics_restatement as fr
    from oracle.qg_ref import QGModelRef
    from oracle.spectral_ref import calc_ispec
    N, R, delta = 12, 3, 0.25
    rs = np.random.RandomState(5)
    run = {'u': rs.randn(R, 2, 2, N, N), 'v': rs.randn(R, 2, 2, N, N), 'time': np.arange(2.0)}
    for key in ('KEspec', 'Ensspec'):
        run[key] = rs.rand(R, 2, N, N // 2 + 1)
    for key in ('KEflux', 'APEflux', 'APEgenspec', 'KEfrictionspec', 'paramspec_KEflux', 'Dissspec'):
        run[key] = rs.randn(R, N, N // 2 + 1)
    s = fr.dataset_statistics(run, delta)
    g = QGModelRef(nx=N)
    assert s['KEspecr'].shape == (2,) + s['kr'].shape and s['KEspecr_mean'].shape == s['kr'].shape
    m = run['KEspec'].mean(0)
    np.testing.assert_allclose(s['KEspecr'][1], calc_ispec(g, m[1])[1], rtol=1e-14)
    np.testing.assert_allclose(s['KEspecr_mean'], calc_ispec(g, 0.2 * m[0] + 0.8 * m[1])[1], rtol=1e-13)
    assert 'KEfluxr_mean' not in s and 'Dissspecr' in s
    np.testing.assert_allclose(s['Energysumr'], s['KEfluxr'] + s['APEfluxr'] + s['APEgenspecr'] + s['KEfrictionspecr'] +
                               s['paramspec_KEfluxr'], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(s['Efluxr'], s['KEfluxr'] + s['APEfluxr'] + s['paramspec_KEfluxr'], rtol=1e-13, atol=1e-15)
    # keyword arguments reach calc_ispec
    s2 = fr.dataset_statistics(run, delta, averaging=False, truncate=False)
    assert s2['KEfluxr'].shape != s['KEfluxr'].shape


# ---- xr_lite: to_netcdf -> open_dataset / open_mfdataset / merge ----------------------------------------------------
def _snapshot_file(tmp_path, name, seed, run_dim=False):
    from pyqg_generative_amd.tools import xr_lite as xr
    rs = np.random.RandomState(seed)
    lead, dims = ((2,), ('run',)) if run_dim else ((), ())
    ds = xr.Dataset({'q': (dims + ('time', 'lev', 'y', 'x'), rs.randn(*lead, 3, 2, 8, 8).astype('float32')),
                     'KEspec': (dims + ('lev', 'l', 'k'), rs.rand(*lead, 2, 8, 5)),
                     'qh': (dims + ('lev', 'l', 'k'), rs.randn(*lead, 2, 8, 5) + 1j)},            # complex: not written
                    coords={'time': (('time',), np.array([10., 20., 30.], dtype='float32'), {'units': 'days'}),
                            'lev': (('lev',), np.arange(1, 3)), 'x': (('x',), np.arange(8) + 0.5)},
                    attrs={'pyqg_params': "{'nx': 8}", 'pyqg:rek': 5.787e-7})
    path = str(tmp_path / name)
    ds.to_netcdf(path)
    return ds, path


def test_netcdf_round_trip(tmp_path):
    from pyqg_generative_amd.tools import xr_lite as xr
    ds, path = _snapshot_file(tmp_path, 'run_0.nc', 0)
    back = xr.open_dataset(path, decode_times=False)
    assert set(back.keys()) == {'q', 'KEspec'} and set(back.coords) == {'time', 'lev', 'x'}
    for k in ('q', 'KEspec', 'time', 'lev', 'x'):
        assert back[k].dims == ds[k].dims
        np.testing.assert_array_equal(back[k].values, ds[k].values)
    assert back['q'].dtype == np.float32 and back['q'].values.dtype.isnative
    assert back['time'].attrs == {'units': 'days'}
    assert back.attrs['pyqg_params'] == "{'nx': 8}" and back.attrs['pyqg:rek'] == 5.787e-7
    back['q'] = back['q'] * 2                       # the values are in memory: the file is closed
    with pytest.raises(Exception):
        xr.open_dataset(str(tmp_path / 'missing.nc'))


def test_open_mfdataset_and_merge(tmp_path):
    from pyqg_generative_amd.tools import xr_lite as xr
    parts = [_snapshot_file(tmp_path, f'run_{i}.nc', i)[0] for i in (1, 0, 2)]       # written out of order: the glob sorts
    both = xr.open_mfdataset(str(tmp_path / 'run_*.nc'), combine='nested', concat_dim='run', decode_times=False,
                             chunks={'time': 1, 'run': 1})
    assert both['q'].dims == ('run', 'time', 'lev', 'y', 'x') and both['q'].shape == (3, 3, 2, 8, 8)
    assert both['KEspec'].dims == ('run', 'lev', 'l', 'k')
    for i, j in ((0, 1), (1, 0), (2, 2)):
        np.testing.assert_array_equal(both['q'].values[i], parts[j]['q'].values)
    assert both['time'].dims == ('time',)
    # files that already hold a 'run' dimension are concatenated along it
    _, p2 = _snapshot_file(tmp_path, 'ens_a.nc', 7, run_dim=True)
    _, p3 = _snapshot_file(tmp_path, 'ens_b.nc', 8, run_dim=True)
    assert xr.open_mfdataset([p2, p3], combine='nested', concat_dim='run')['q'].shape == (4, 3, 2, 8, 8)
    with pytest.raises(OSError):
        xr.open_mfdataset(str(tmp_path / 'none_*.nc'), combine='nested', concat_dim='run')
    with pytest.raises(NotImplementedError):
        xr.open_mfdataset(str(tmp_path / 'run_*.nc'))

    stats = xr.Dataset({'KE_time': xr.DataArray(np.arange(3.), dims=['time'], coords=[both['time']]),
                        'PDF_q1': xr.DataArray(np.ones(4), dims='q_0', coords=[np.arange(4.)])})
    m = xr.merge([both, stats])
    assert set(m.keys()) == {'q', 'KEspec', 'KE_time', 'PDF_q1'} and {'time', 'lev', 'x', 'q_0'} <= set(m.coords)
    assert m.attrs == both.attrs
    np.testing.assert_array_equal(m['KE_time'].values, np.arange(3.))
    clash = xr.Dataset({'q': both['q'] + 1})
    with pytest.raises(ValueError):
        xr.merge([both, clash])
    assert set(xr.merge([both, xr.Dataset({'q': both['q']})]).keys()) == {'q', 'KEspec'}      # the same values: no conflict


def test_cache_path():
    from pyqg_generative_amd.tools.comparison_tools import cache_path
    assert cache_path('/data/eddy/run_*.nc') == '/data/eddy/' + 'run_*.nc'.encode().hex() + '.cache_netcdf'
    assert cache_path('/data/eddy/run_*.nc') == '/data/eddy/72756e5f2a2e6e63.cache_netcdf'
    assert cache_path('[0-9].nc') == '5b302d395d2e6e63.cache_netcdf'
