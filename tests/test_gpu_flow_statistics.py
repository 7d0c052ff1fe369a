"""GPU: the derived flow fields of csrc/flow.hip (qgx_flow_features) against the float64 restatement
(tests/flow_statistics_restatement.py) on both of its paths, its guard bands (tests/redzone.py), repeatability and NaN
containment; dataset_statistics / dataset_smart_read / the command line of tools/comparison_tools.py on a run of this engine.

Bounds.  omega: 1e-11 of the plane's max |omega| (the bound of tests/test_gpu_backscatter.py for LDS-transform closures);
Ens = omega^2 / 2: 4e-11 max|omega|^2 (d Ens = omega d omega <= 1e-11 max^2, with room for the restatement's own transform
error); KE, Vabs: one float32 ulp of the float64 value for float32 outputs (the value is computed in float64 and rounded
once), 1e-13 relative for float64 ones; KE_sum: 1e-12 relative (at most 128^2 non-negative float64 terms)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

import redzone
import flow_statistics_restatement as fr

DEV = 'cuda'
NAMES = ('omega', 'KE', 'Ens', 'Vabs', 'KE_sum')
# (N, members of the plan, snapshots S): every compile-time plan, two run-time plans, and the batched path of N > 96 with
# chunks of 2 planes (the issue's case) and of 3 planes, whose last chunk of the 10 planes is short
CASES = [(8, 1, 3), (12, 1, 3), (48, 1, 3), (64, 1, 3), (96, 1, 2), (128, 2, 5), (128, 3, 5)]


def _L():
    from pyqg_generative_amd import _lib
    return _lib


def _ct():
    from pyqg_generative_amd.tools import comparison_tools
    return comparison_tools


def _plan(N, members):
    from pyqg_generative_amd.tools.operators import Dev
    return Dev.plan(N, 2 * members)._h


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _noise(N, S, dtype, seed=0):
    """white noise: energy in every wavenumber, the Nyquist row and column included"""
    rs = np.random.RandomState(1000 * N + seed)
    return (rs.randn(S, 2, N, N) * 0.05).astype(dtype), (rs.randn(S, 2, N, N) * 0.03).astype(dtype)


def _workspace(plan, S):
    n = C.c_size_t()
    _L().check(_L().lib.qgx_flow_features_workspace(plan, S, C.byref(n)))
    return n.value


def _shapes(S, N, dtype):
    td = torch.float64 if dtype == 'float64' else torch.float32
    return {'omega': ((S, 2, N, N), torch.float64), 'KE': ((S, 2, N, N), td), 'Ens': ((S, 2, N, N), torch.float64),
            'Vabs': ((S, 2, N, N), td), 'KE_sum': ((S, 2), torch.float64)}


def _run(plan, ud, vd, outs, work=None, nbytes=None):
    """outs: dict name -> tensor (a missing name is passed as NULL)"""
    S = ud.shape[0]
    if nbytes is None:
        nbytes = _workspace(plan, S)
    if work is None and nbytes:
        work = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return _L().lib.qgx_flow_features(plan, P(ud), P(vd), int(ud.dtype == torch.float64), S, *(P(outs.get(k)) for k in NAMES),
                                      P(work), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _features(plan, u, v, want=NAMES):
    ud, vd = torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    S, _, N, _ = u.shape
    outs = {k: torch.empty(s, dtype=d, device=DEV) for k, (s, d) in _shapes(S, N, str(u.dtype)).items() if k in want}
    _L().check(_run(plan, ud, vd, outs))
    return outs


def _check(got, ref, dtype, report=None):
    """got: dict of host arrays; ref: the restatement's float64 dict; asserts the module's bounds plane by plane"""
    top = np.abs(ref['omega']).max(axis=(-2, -1), keepdims=True)
    figures = {}
    if 'omega' in got:
        figures['omega'] = (np.abs(got['omega'] - ref['omega']) / top).max()
        assert figures['omega'] <= 1e-11, figures
    if 'Ens' in got:
        figures['Ens'] = (np.abs(got['Ens'] - ref['Ens']) / top ** 2).max()
        assert figures['Ens'] <= 4e-11, figures
    for k in ('KE', 'Vabs'):
        if k not in got:
            continue
        assert got[k].dtype == np.dtype(dtype)
        if dtype == 'float32':
            figures[k] = (np.abs(got[k].astype(np.float64) - ref[k]) / np.spacing(np.abs(ref[k]).astype(np.float32))).max()
            assert figures[k] <= 1.0, figures
        else:
            figures[k] = (np.abs(got[k] - ref[k]) / np.abs(ref[k])).max()
            assert figures[k] <= 1e-13, figures
    if 'KE_sum' in got:
        figures['KE_sum'] = (np.abs(got['KE_sum'] - ref['KE_sum']) / ref['KE_sum']).max()
        assert figures['KE_sum'] <= 1e-12, figures
    if report is not None:
        print(report, {k: float(f'{v:.3g}') for k, v in figures.items()})
    return figures


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N,members,S', CASES)
def test_kernel_matches_restatement(N, members, S, dtype):
    u, v = _noise(N, S, dtype)
    got = {k: t.cpu().numpy() for k, t in _features(_plan(N, members), u, v).items()}
    _check(got, fr.flow_features(u, v), dtype, report=f'N={N} members={members} S={S} {dtype}:')


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_fused_agrees_with_composed_route_at_64(dtype):
    """the route of the engine's building blocks: rfft2 -> qgx_spec_curl -> irfft2 (what _Snapshots.curl does), torch
    elementwise for the rest"""
    from pyqg_generative_amd.tools.operators import Dev
    from pyqg_generative_amd.engine import _ptr, _stream
    N, S = 64, 3
    u, v = _noise(N, S, dtype, seed=1)
    got = {k: t.cpu().numpy() for k, t in _features(_plan(N, 1), u, v).items()}
    ud, vd = (torch.from_numpy(a).to(DEV).to(torch.float64).reshape(-1, N, N) for a in (u, v))
    uh, vh = Dev.rfft2(ud), Dev.rfft2(vd)
    ch = torch.empty_like(uh)
    _L().check(_L().lib.qgx_spec_curl(_ptr(uh), _ptr(vh), _ptr(ch), ch.shape[0], N, Dev.L, _stream()))
    omega = Dev.irfft2(ch).reshape(S, 2, N, N)
    ke = 0.5 * (ud * ud + vd * vd).reshape(S, 2, N, N)
    composed = {'omega': omega, 'KE': ke, 'Ens': 0.5 * omega * omega, 'Vabs': torch.sqrt(2 * ke), 'KE_sum': ke.sum(dim=(-2, -1))}
    _check(got, {k: t.cpu().numpy() for k, t in composed.items()}, dtype, report=f'fused against composed, {dtype}:')


# ---- guard bands ----------------------------------------------------------------------------------------------------
def _twice(launch, outs, works, ins):
    """launch() with outputs and workspaces prefilled 0xFF, then 0x00: guards intact, inputs frozen, every output element
    written, and bitwise equal payloads -> the payloads"""
    runs = []
    frozen = [redzone.frozen(t) for t in ins]
    for fill in (0xFF, 0x00):
        for g in list(outs) + list(works):
            g.refill(fill)
        launch()
        torch.cuda.synchronize()
        for i, g in enumerate(outs):
            g.check(written=fill == 0xFF, what=f'output #{i}')
        for i, g in enumerate(works):
            g.check(what=f'workspace #{i}')
        for i, f in enumerate(frozen):
            f.check(what=f'input #{i}')
        runs.append([g.bits() for g in outs])
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a, b), f'output #{i} depends on what the buffers held before the call'
    return runs[0]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('N,members,S', [(12, 1, 2), (64, 1, 2), (128, 2, 3), (128, 3, 2)])
def test_guard_bands(N, members, S, dtype):
    plan = _plan(N, members)
    u, v = _noise(N, S, dtype, seed=2)
    ud, vd = torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    nbytes = _workspace(plan, S)
    assert (nbytes == 0) == (N <= 96)
    works = [redzone.guarded((nbytes,), torch.uint8, DEV)] if nbytes else []
    work = works[0].t if works else None
    g = {k: redzone.guarded(s, d, DEV) for k, (s, d) in _shapes(S, N, dtype).items()}
    full = _twice(lambda: _L().check(_run(plan, ud, vd, {k: x.t for k, x in g.items()}, work, nbytes)),
                  [g[k] for k in NAMES], works, [ud, vd])
    got = {k: g[k].t.cpu().numpy() for k in NAMES}
    _check(got, fr.flow_features(u, v), dtype)
    # NULL outputs: what is passed is bitwise what the full call gave, what is not passed is not touched
    for subset in (('omega',), ('Ens',), ('KE', 'KE_sum'), ('Vabs',), ('KE_sum',), ('omega', 'Vabs')):
        for k in NAMES:
            if k not in subset:
                g[k].refill(0xFF)
        part = _twice(lambda: _L().check(_run(plan, ud, vd, {k: g[k].t for k in subset}, work, nbytes)),
                      [g[k] for k in subset], works, [ud, vd])
        for k, bits in zip(subset, part):
            assert np.array_equal(bits, full[NAMES.index(k)]), (subset, k)
        for k in NAMES:
            if k not in subset:
                g[k].check(what=f'{k} (passed as NULL)')
                n_el = int(np.prod(g[k].shape))
                assert g[k].unwritten() == n_el, f'{k} was passed as NULL and written all the same'


def test_refusals_with_a_real_plan():
    lib = _L().lib
    u, v = _noise(128, 2, 'float64')
    ud, vd = torch.from_numpy(u).to(DEV), torch.from_numpy(v).to(DEV)
    out = {'KE_sum': torch.full((2, 2), -1.0, dtype=torch.float64, device=DEV)}
    large, small = _plan(128, 2), _plan(48, 1)
    need = _workspace(large, 2)
    assert need > 0 and _workspace(small, 2) == 0
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert _run(large, ud, vd, out, work, need - 1) == -1
    assert b'work space' in lib.qgx_last_error()
    assert lib.qgx_flow_features(large, P(ud), P(vd), 1, 2, None, None, None, None, P(out['KE_sum']), None, need, None) == -1
    assert _run(large, ud, vd, {}, work, need) == -1
    torch.cuda.synchronize()
    assert (out['KE_sum'] == -1.0).all()                 # refused before any device call
    assert _run(large, ud, vd, out, work, need) == 0


# ---- other kernel properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,members', [(48, 1), (18, 1), (128, 3)])
def test_bitwise_repeatable_on_a_side_stream(N, members):
    plan = _plan(N, members)
    u, v = _noise(N, 4, 'float32', seed=3)
    first = _features(plan, u, v)
    again = _features(plan, u, v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _features(plan, u, v)
    side.synchronize()
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], other[k]), k


@pytest.mark.parametrize('N,members', [(12, 1), (48, 1), (128, 2)])
def test_nan_stays_in_its_plane(N, members):
    plan = _plan(N, members)
    u, v = _noise(N, 3, 'float64', seed=4)
    clean = {k: t.cpu().numpy() for k, t in _features(plan, u, v).items()}
    ub = u.copy()
    ub[1, 1, N // 3, 2] = np.nan
    bad = {k: t.cpu().numpy() for k, t in _features(plan, ub, v).items()}
    for k in NAMES:
        keep = np.ones(bad[k].shape[:2], dtype=bool)
        keep[1, 1] = False
        assert np.array_equal(bad[k][keep], clean[k][keep]), f'{k}: a NaN in plane (1, 1) changed another plane'
    assert np.isnan(bad['omega'][1, 1]).all() and np.isnan(bad['Ens'][1, 1]).all() and np.isnan(bad['KE_sum'][1, 1])
    assert np.isnan(bad['KE'][1, 1]).sum() == 1 and np.isnan(bad['Vabs'][1, 1]).sum() == 1


def test_flow_features_facade():
    ct = _ct()
    N = 48
    u, v = _noise(N, 6, 'float32', seed=5)
    u5, v5 = u.reshape(2, 3, 2, N, N), v.reshape(2, 3, 2, N, N)
    ref = fr.flow_features(u5, v5)
    f = ct.flow_features(u5, torch.from_numpy(v5).to(DEV))
    assert list(f) == list(NAMES) and f['omega'].shape == (2, 3, 2, N, N) and f['KE_sum'].shape == (2, 3, 2)
    assert f['KE'].dtype == torch.float32 and f['omega'].dtype == torch.float64
    _check({k: t.cpu().numpy() for k, t in f.items()}, ref, 'float32')
    some = ct.flow_features(u5.astype('float64'), v5, want=('Ens', 'KE'))            # mixed dtypes: float64
    assert list(some) == ['Ens', 'KE'] and some['KE'].dtype == torch.float64
    _check({k: t.cpu().numpy() for k, t in some.items()}, ref, 'float64')
    for bad in (dict(want=('omega', 'zeta')), dict(want=())):
        with pytest.raises(ValueError):
            ct.flow_features(u5, v5, **bad)
    with pytest.raises(ValueError):
        ct.flow_features(u5, v5[:1])
    with pytest.raises(ValueError):
        ct.flow_features(u5[:, :, :1], v5[:, :, :1])


# ---- dataset_statistics / dataset_smart_read ------------------------------------------------------------------------
T_SNAP = 48         # snapshots of the run: index 44, where the PDFs' window starts, is passed


@pytest.fixture(scope='module')
def run():
    """a short run of this engine, 48 x 48, 2 members, with the time-averaged diagnostics"""
    from pyqg_generative_amd.tools.simulate import run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    p = EDDY_PARAMS.nx(48)._update({'tmax': 14400. * 6 * T_SNAP, 'tavestart': 14400. * 100, 'log_level': 0})
    ds = run_simulation(dict(p), sampling_freq=14400. * 6, n_members=2, seeds=[0, 1])
    assert ds['q'].dims == ('run', 'time', 'lev', 'y', 'x') and ds['q'].shape[:2] == (2, T_SNAP)
    return ds


def _as_restatement(ds):
    """the dataset as the restatement's dict of plain arrays with a leading run axis"""
    out = {'time': np.asarray(ds['time'].values)}
    lead = 0 if 'run' in ds['q'].dims else None
    for k in ('q', 'u', 'v'):
        a = np.asarray(ds[k].values)
        out[k] = a if lead == 0 else a[None]
    for k in fr.DIAGNOSTICS:
        if k in ds.keys():
            a = np.asarray(ds[k].values)
            out[k] = a if 'run' in ds[k].dims else a[None]
    return out


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, top = np.abs(got - ref).max(), np.abs(ref).max()          # (an unparameterized run's paramspec is all zeros)
    assert err <= tol * top, (what, err, top)


def _check_spectra(stats, ref):
    names = [k for k in ref if k != 'kr' and (k.endswith('r') or k.endswith('r_mean'))]
    assert {'KEspecr', 'KEspecr_mean', 'KEfluxr', 'APEgenspecr', 'Energysumr', 'Efluxr', 'Dissspecr'} <= set(names)
    assert sorted(k for k in stats.keys() if k.endswith('r') or k.endswith('r_mean')) == sorted(names)
    for k in names:
        _close(stats[k].values, ref[k], 1e-12, k)
    assert stats['KEspecr'].dims == ('lev', 'kr') and stats['KEspecr_mean'].dims == ('kr',) and stats['Efluxr'].dims == ('kr',)
    _close(stats['kr'].values, ref['kr'], 1e-14, 'kr')
    assert stats['kr'].attrs['long_name'] == 'wavenumber, $m^{-1}$'
    np.testing.assert_array_equal(stats['lev'].values, [1, 2])


@pytest.mark.parametrize('layout', ['ensemble', 'single'])
def test_dataset_statistics(run, layout):
    ct = _ct()
    ds = run if layout == 'ensemble' else run.isel(run=1)
    assert ('run' in ds['q'].dims) == (layout == 'ensemble')
    ref = fr.dataset_statistics(_as_restatement(ds), delta=0.25)
    stats = ct.dataset_statistics(ds, delta=0.25)
    _check_spectra(stats, ref)
    assert stats['KE_time'].dims == ('time',)
    _close(stats['KE_time'].values, ref['KE_time'], 1e-12, 'KE_time')
    _close(stats['time'].values, ref['time'], 1e-7, 'time')                       # (a float32 coordinate)
    assert stats['time'].attrs == {'long_name': 'time [$years$]'}
    assert float(ds['time'].values[-1]) == pytest.approx(360. * float(stats['time'].values[-1]))     # ds itself is untouched
    # the keyword arguments are calc_ispec's
    ref2 = fr.dataset_statistics(_as_restatement(ds), delta=0.1, averaging=False, truncate=False)
    stats2 = ct.dataset_statistics(ds, delta=0.1, averaging=False, truncate=False)
    _close(stats2['KEspecr_mean'].values, ref2['KEspecr_mean'], 1e-12, 'KEspecr_mean, other binning')
    _close(stats2['KE_time'].values, ref2['KE_time'], 1e-12, 'KE_time, delta = 0.1')


def _check_smart(ds, out, ref, compute_all):
    xr_dims = ds['q'].dims
    lead = () if 'run' in xr_dims else (0,)
    for k in ds.keys():
        assert k in out.keys(), k                                                  # the run itself is part of the result
    _check_spectra(out, ref)
    _close(out['KE_time'].values, ref['KE_time'], 1e-12, 'KE_time')
    feats = {}
    if compute_all:
        for k in ('omega', 'KE', 'Ens', 'Vabs'):
            assert out[k].dims == xr_dims, k
            a = np.asarray(out[k].values)
            feats[k] = a if not lead else a[None]
        assert feats['KE'].dtype == np.float32 and feats['omega'].dtype == np.float64
        _check(feats, {k: ref[k] for k in feats}, 'float32')
    else:
        assert not {'omega', 'KE', 'Ens', 'Vabs', 'PDF_Ens1', 'PDF_Ens2'} & set(out.keys())
    window = slice(fr.T0, None) if compute_all else slice(-1, None)
    n = np.asarray(ds['q'].values).size // (2 * T_SNAP) * len(range(T_SNAP)[window])       # values in a PDF's view
    for var in ('q', 'u', 'v', 'KE', 'Ens') if compute_all else ('q', 'u', 'v', 'KE'):
        for lev in (0, 1):
            name, dim = f'PDF_{var}{lev + 1}', f'{var}_{lev}'
            assert out[name].dims == (dim,) and out[name].shape == (30,)
            points, dens = np.asarray(out[dim].values), np.asarray(out[name].values)
            if var in ('KE', 'Ens') and compute_all:
                # fixed range: exactly np.histogram of the feature array the GPU returned
                pr, dr = fr.pdf(feats[var][:, window, lev].astype(np.float64), 0, fr.PDF_XMAX[(var, lev)], 30)
                np.testing.assert_array_equal(dens, dr)
                np.testing.assert_allclose(points, pr, rtol=1e-15)
            elif var == 'KE':
                # the last snapshot's KE is not returned: against the restatement's float64 KE, where a float32 rounding
                # of the product's KE can move a value on an edge into the neighbouring bin
                np.testing.assert_allclose(dens, ref[name], rtol=0, atol=1.5 / n / (fr.PDF_XMAX[(var, lev)] / 30))
            else:
                # default range mean -+ 4 sigma from the device's own statistics: within 1.5 counts per bin
                pr, dr = ref[dim], ref[name]
                np.testing.assert_allclose(points, pr, rtol=0, atol=1e-9 * np.abs(pr).max())
                np.testing.assert_allclose(dens, dr, rtol=0, atol=1.5 / n / (pr[1] - pr[0]))


@pytest.mark.parametrize('layout,compute_all', [('ensemble', True), ('single', True), ('ensemble', False)])
def test_dataset_smart_read_of_a_dataset(run, layout, compute_all):
    ds = run if layout == 'ensemble' else run.isel(run=0)
    ref = fr.dataset_smart_read(_as_restatement(ds), delta=0.25, compute_all=compute_all)
    out = _ct().dataset_smart_read(ds, delta=0.25, compute_all=compute_all)
    _check_smart(ds, out, ref, compute_all)
    np.testing.assert_array_equal(out['time'].values, ds['time'].values)           # a dataset argument: time as given


def test_pdfs_that_fill_their_fixed_ranges():
    """a synthetic dataset whose KE and Ens spread over the fixed ranges of the PDFs (a young run sits in their first
    bins), on a grid with a run-time transform plan"""
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    N, R, T = 12, 2, 46
    rs = np.random.RandomState(9)
    dims = ('run', 'time', 'lev', 'y', 'x')
    scale = np.array([0.08, 0.015])[:, None, None]
    fields = {k: (rs.randn(R, T, 2, N, N) * (scale if k != 'q' else 1e-5)).astype('float32') for k in ('q', 'u', 'v')}
    ds = xr.Dataset({k: (dims, a) for k, a in fields.items()},
                    coords={'time': (('time',), np.arange(T, dtype='float32') * 10), 'x': (('x',), np.arange(N) + 0.5)})
    ref = fr.dataset_smart_read(dict(fields, time=np.arange(T) * 10.), compute_all=True)
    out = _ct().dataset_smart_read(ds)
    for var, lev in fr.PDF_XMAX:
        feat = np.asarray(out[var].values)[:, fr.T0:, lev].astype(np.float64)
        pr, dr = fr.pdf(feat, 0, fr.PDF_XMAX[(var, lev)], 30)
        dens = np.asarray(out[f'PDF_{var}{lev + 1}'].values)
        np.testing.assert_array_equal(dens, dr)
        if var == 'KE':
            assert (dens > 0).sum() >= 10, (var, lev, dens)                        # the range is in use
        np.testing.assert_allclose(dens, ref[f'PDF_{var}{lev + 1}'], rtol=0, atol=1.5 / feat.size / (pr[1] - pr[0]))
    _check({k: np.asarray(out[k].values) for k in ('omega', 'KE', 'Ens', 'Vabs')}, ref, 'float32')


def _member_files(run, folder):
    for i in range(2):
        run.isel(run=i).to_netcdf(os.path.join(str(folder), f'member_{i}.nc'))
    return os.path.join(str(folder), 'member_*.nc')


def test_dataset_smart_read_of_files_and_its_cache(run, tmp_path):
    ct = _ct()
    path = _member_files(run, tmp_path)
    cache = ct.cache_path(path)
    assert not os.path.exists(cache)
    ref = fr.dataset_smart_read(_as_restatement(run), delta=0.25, compute_all=True)
    out = ct.dataset_smart_read(path)
    assert os.path.exists(cache)
    assert out['q'].dims == ('run', 'time', 'lev', 'y', 'x')
    _check_smart(run, out, ref, True)
    np.testing.assert_allclose(out['time'].values, np.asarray(run['time'].values) / 360, rtol=1e-6)
    assert out['time'].attrs == {'long_name': 'time [$years$]'}
    # read back from the cache: the same statistics without computing anything
    calls = []
    orig = ct.flow_features
    ct.flow_features = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        cached = ct.dataset_smart_read(path)
        assert not calls
        for k in out.keys():
            np.testing.assert_array_equal(np.asarray(cached[k].values), np.asarray(out[k].values), err_msg=k)
        np.testing.assert_array_equal(cached['time'].values, out['time'].values)
        # read_cache=False deletes it and computes anew: a cache that cannot be read is never opened
        with open(cache, 'wb') as f:
            f.write(b'not a netcdf file')
        fresh = ct.dataset_smart_read(path, read_cache=False, compute_all=False)
        assert calls and 'omega' not in fresh.keys() and 'PDF_KE1' in fresh.keys()
    finally:
        ct.flow_features = orig
    from pyqg_generative_amd.tools.simulate import dataset_backend
    back = dataset_backend().open_dataset(cache)
    assert 'omega' not in back.keys() and 'KE_time' in back.keys()                 # the cache was written anew
    # dataset_statistics of a path: the files as they are, time in years
    ds = ct.dataset_statistics(path)
    assert ds['q'].shape == run['q'].shape and 'KE_time' not in ds.keys()
    np.testing.assert_allclose(ds['time'].values, np.asarray(run['time'].values) / 360, rtol=1e-6)


# ---- command line ---------------------------------------------------------------------------------------------------
def test_command_line(run, tmp_path, capsys):
    ct = _ct()
    path = _member_files(run, tmp_path)
    target = os.path.join(str(tmp_path), 'target.nc')
    run.isel(run=0).to_netcdf(target)
    save = os.path.join(str(tmp_path), 'difference.json')
    got = ct.main(['--model_path', path, '--target_path', target, '--save_file', save, '--key', 'eddy-48'])
    assert 'difference calculated' in capsys.readouterr().out
    with open(save) as f:
        stored = json.load(f)
    assert stored == got and stored['key'] == 'eddy-48'
    want, _, _ = ct.diagnostic_differences_Perezhogin(run, run.isel(run=0), T=128)
    assert set(stored) == set(want) | {'key'}
    for k, val in want.items():
        # the files hold what the datasets hold (float32 snapshots, float64 spectra)
        assert stored[k] == pytest.approx(val, rel=1e-12, abs=1e-300), k
