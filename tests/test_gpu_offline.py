"""GPU: the offline metrics (csrc/offline.hip, tools/computational_tools.py, Parameterization.test_offline).

Each kernel against numpy at N = 32, 48, 64 with time windows across t = 44 and float32 / float64 inputs; bitwise
repeatability on the default and on a side stream; test_offline of GAN, GZ and OLS against the test-side restatement
(tests/offline_restatement.py); NaN propagation; and the reference's published offline numbers
(Google-Colab/offline-analysis.ipynb) from test_offline itself.
"""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restatement():
    spec = importlib.util.spec_from_file_location('offline_restatement',
                                                  os.path.join(ROOT, 'tests', 'offline_restatement.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ct():
    from pyqg_generative_amd.tools import computational_tools
    return computational_tools


def _fields(N, dtype_t, dtype_mg, R=2, T=47, seed=0):
    rs = np.random.RandomState(seed + N)
    t = (rs.randn(R, T, 2, N, N) * 3e-11).astype(dtype_t)
    m = (0.7 * t + 1e-11 * rs.randn(R, T, 2, N, N)).astype(dtype_mg)
    g = (m + 2e-11 * rs.randn(R, T, 2, N, N)).astype(dtype_mg)
    psi = (rs.randn(R, T, 2, N, N) * 1e3).astype(dtype_t)
    return t, m, g, psi


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]


def _numpy_planes(t, m, g, psi, t0):
    N = t.shape[-1]
    f = [np.fft.rfftn(np.asarray(x, 'float64'), axes=(-2, -1)) / (N * N) for x in (t, g, m, psi)]
    T_, G, M, P = f
    X = [T_, G, M, T_ - M, G - M]
    planes = np.zeros((2, 22) + T_.shape[-2:])
    for w, sl in enumerate((slice(0, t0), slice(t0, None))):
        for k, x in enumerate(X):
            for z in (0, 1):
                planes[w, 2 * k + z] = (np.abs(x[:, sl, z]) ** 2).sum((0, 1))
                planes[w, 10 + 2 * k + z] = np.real(np.conj(P[:, sl, z]) * x[:, sl, z]).sum((0, 1))
        planes[w, 20] = np.real(np.conj(X[3][:, sl, 0]) * X[3][:, sl, 1]).sum((0, 1))
        planes[w, 21] = np.real(np.conj(X[4][:, sl, 0]) * X[4][:, sl, 1]).sum((0, 1))
    return planes


def _numpy_moments(t, m, g):
    t, m, g = (np.asarray(x, 'float64') for x in (t, m, g))
    out = {}
    for name, ax in (('spatial', (0, 1)), ('temporal', (0, 3, 4)), ('global', (0, 1, 3, 4))):
        tc = t - t.mean(ax, keepdims=True)
        mc = m - m.mean(ax, keepdims=True)
        q = [((t - m) ** 2).sum(ax), (t ** 2).sum(ax), (tc ** 2).sum(ax), (mc ** 2).sum(ax), (tc * mc).sum(ax),
             ((g - m) ** 2).sum(ax)]
        out[name] = np.stack(q)
    return out


def _close(a, b, rtol):
    a, b = np.asarray(a), np.asarray(b)
    scale = np.abs(b).max(axis=tuple(range(1, b.ndim)), keepdims=True) if b.ndim > 1 else np.abs(b).max()
    assert np.all(np.abs(a - b) <= rtol * scale), float((np.abs(a - b) / scale).max())


@pytest.mark.parametrize('N', [32, 48, 64])
@pytest.mark.parametrize('dt', ['float32', 'float64'])
def test_kernels_against_numpy(N, dt):
    ct = _ct()
    t, m, g, psi = _fields(N, dt, 'float64' if dt == 'float32' else 'float32')
    td, md, gd, pd = _dev(t, m, g, psi)
    # spectra: both windows of every plane, one snapshot chunk and several
    ref = _numpy_planes(t, m, g, psi, 44)
    got = ct.spectra_sums(td, md, gd, pd, t0=44)
    for w in (0, 1):
        _close(got[w], ref[w], 1e-9)
    old = ct.CHUNK
    try:
        ct.CHUNK = 40
        got2 = ct.spectra_sums(td, md, gd, pd, t0=44)
    finally:
        ct.CHUNK = old
    for w in (0, 1):
        _close(got2[w], got[w], 1e-13)      # snapshot s is added to group s % 32 in the same order for any chunking
    # moments
    mom = ct.moment_sums(td, md, gd)
    ref = _numpy_moments(t, m, g)
    _close(mom['spatial'], ref['spatial'].reshape(6, 2, N, N), 1e-9)
    _close(mom['temporal'], ref['temporal'], 1e-9)
    _close(mom['global'], ref['global'], 1e-9)
    # histogram of layer z over t >= 44 in units of its population std: exact counts
    edges = np.linspace(-5, 5, 71)
    for z in (0, 1):
        counts, stats = ct.histogram(td, edges, z=z, t0=44, shape=(2, 47, 2, N * N))
        view = np.asarray(t[:, 44:, z], 'float64')
        assert stats[3] == stats[1] and abs(stats[1] - view.std()) <= 1e-12 * view.std()
        assert abs(stats[0] - view.mean()) <= 1e-12 * np.abs(view).max() and stats[2] == 0
        np.testing.assert_array_equal(counts, np.histogram(view / stats[3], bins=70, range=(-5, 5))[0])
        counts, stats = ct.histogram(gd, edges, z=z, t0=44, scale=float(stats[1]), shape=(2, 47, 2, N * N))
        np.testing.assert_array_equal(counts, np.histogram(np.asarray(g[:, 44:, z], 'float64') / stats[3], bins=70,
                                                           range=(-5, 5))[0])


def test_histogram_on_edges_and_pdf_histogram():
    ct = _ct()
    edges = np.linspace(-5, 5, 71)
    rs = np.random.RandomState(5)
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), rs.randn(100000) * 2,
                        [-7., 7.]])
    counts, stats = ct.histogram(torch.from_numpy(x).cuda(), edges, scale=1.0)
    np.testing.assert_array_equal(counts, np.histogram(x, bins=70, range=(-5, 5))[0])
    rst = _restatement()
    for arr in (x, torch.from_numpy(x).cuda()):
        p, d = ct.PDF_histogram(arr)
        pr, dr = rst.pdf(x)
        np.testing.assert_allclose(p, pr, rtol=0, atol=1e-12)
        np.testing.assert_allclose(d, dr, rtol=0, atol=1.5 / x.size / ((pr[1] - pr[0])))
    p, d = ct.PDF_histogram(x, -5, 5, 70)
    pr, dr = rst.pdf(x, -5, 5, 70)
    np.testing.assert_array_equal(d, dr)


def test_bitwise_repeatable_on_any_stream():
    ct = _ct()
    t, m, g, psi = _fields(48, 'float32', 'float64', T=50)
    td, md, gd, pd = _dev(t, m, g, psi)
    edges = np.linspace(-5, 5, 71)

    def run():
        sp = ct.spectra_sums(td, md, gd, pd)
        mo = ct.moment_sums(td, md, gd)
        h = ct.histogram(gd, edges, z=1, t0=44, shape=(2, 50, 2, 48 * 48))
        return [sp] + [mo[k] for k in ('spatial', 'temporal', 'global')] + list(h)
    a = run()
    b = run()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = run()
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8))


def test_nan_propagates():
    ct = _ct()
    t, m, g, psi = _fields(32, 'float32', 'float64')
    t[1, 45, 0, 3, 4] = np.nan
    td, md, gd, pd = _dev(t, m, g, psi)
    mom = ct.moment_sums(td, md, gd)
    with_t, without_t = [0, 1, 2, 4], [3, 5]         # (m - m')^2 and (g - m)^2 do not read the truth
    assert np.isnan(mom['global'][with_t, 0]).all() and np.isfinite(mom['global'][without_t, 0]).all()
    assert np.isfinite(mom['global'][:, 1]).all()
    assert np.isnan(mom['temporal'][with_t, 45, 0]).all() and np.isfinite(mom['temporal'][:, 44, 0]).all()
    assert np.isfinite(mom['temporal'][without_t, 45, 0]).all()
    assert np.isnan(mom['spatial'][with_t, 0, 3, 4]).all() and np.isfinite(mom['spatial'][:, 0, 3, 5]).all()
    sp = ct.spectra_sums(td, md, gd, pd)
    assert np.isnan(sp[1, 0]).all() and np.isfinite(sp[0]).all()
    counts, stats = ct.histogram(td, np.linspace(-5, 5, 71), z=0, t0=44, shape=(2, 47, 2, 32 * 32))
    assert stats[2] == 1 and np.isnan(stats[1])
    assert np.isnan(ct.PDF_histogram(t[:, :, 0])[1]).all()
    assert np.isnan(ct.PDF_histogram(t[:, :, 0], -1, 1, 10)[1]).all()
    st = ct.OfflineStats(t, m, g, psi, pdfs=True, res=t.astype('float64') - m, gen_res=g - m)
    assert np.isnan(st.pdf['0']).all() and np.isfinite(st.pdf['1']).all()


# ---- test_offline -------------------------------------------------------------------------------------------------
FIELD_VARS = ['q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var', 'q',
              'q_forcing_advection_gen', 'q_forcing_advection_std', 'q_forcing_advection_res',
              'q_forcing_advection_gen_res']
SCORES = ['R2_mean', 'R2_total', 'R2_residual', 'L2_mean', 'L2_total', 'L2_residual']
GROUPED = [p + q for q in ('mse', 'nmse', 'skill', 'correlation') for p in ('spatial_', 'temporal_', '')] + \
    ['temporal_sgs_ms', 'temporal_var_ratio', 'var_ratio']
SPECTRA = [n + s for n in ('PSD', 'Eflux') for s in ('', '_gen', '_res', '_gen_res', '_mean')]
PDFS = {'PDF' + s + str(z): ('q_' if s in ('', '_gen', '_mean') else 'dq_') + str(z)
        for s in ('', '_gen', '_mean', '_res', '_gen_res') for z in (0, 1)}


def _dataset(N=48, R=2, T=46, seed=3):
    from pyqg_generative_amd.tools.simulate import dataset_backend
    from oracle.qg_ref import QGModelRef
    xr = dataset_backend()
    rs = np.random.RandomState(seed)
    m0 = QGModelRef(nx=N)
    q = rs.randn(R, T, 2, N, N) * np.array([8e-6, 1e-6])[None, None, :, None, None]
    q = np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (m0.wv < 2. / 3. * m0.kk[-1]), axes=(-2, -1)) * 3
    dims = ['run', 'time', 'lev', 'y', 'x']
    return xr.Dataset({'q': (dims, q.astype('float32')),
                       'q_forcing_advection': (dims, (rs.randn(R, T, 2, N, N) * 3e-11).astype('float32')),
                       'psi': (dims, (rs.randn(R, T, 2, N, N) * 1e3).astype('float32'))},
                      coords={'time': (('time',), np.arange(T, dtype='float32') * 1000.)},
                      attrs={'source': 'synthetic'})


def _model(kind):
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression, MeanVarModel, OLSModel
    if kind == 'ols':           # GZ's net_mean as an AndrewCNN(2, 2), the net of tests/golden/ols.npz
        path = os.path.join(ROOT, 'tests', 'golden', 'weights_gz.npz')
        d = np.load(path)
        return OLSModel.from_arrays([weights.net_from_npz(d, 'net0_')], np.asarray(d['x_std'], np.float32),
                                    np.asarray(d['y_std'], np.float32))
    cls = {'gan': CGANRegression, 'gz': MeanVarModel}[kind]
    nets, xs, ys = weights.load_npz(os.path.join(ROOT, 'tests', 'golden', f'weights_{kind}.npz'), kind)
    return cls.from_arrays(nets, xs, ys)


@pytest.mark.parametrize('kind', ['gan', 'gz', 'ols'])
def test_test_offline_against_the_restatement(kind):
    rst = _restatement()
    ds = _dataset()
    before = {k: np.array(ds[k].values, copy=True) for k in ('q', 'q_forcing_advection', 'psi')}
    model = _model(kind)
    kw = {} if kind == 'ols' else {'seed': 11}
    out = model.test_offline(ds, 8, **kw)
    for k, v in before.items():
        assert np.array_equal(np.asarray(ds[k].values), v)          # ds is not modified
    preds = model.predict(ds, 8, **kw)
    gen, mean = (np.asarray(preds['q_forcing_advection' + s].values) for s in ('', '_mean'))
    true, psi = (np.asarray(ds[k].values) for k in ('q_forcing_advection', 'psi'))
    ref = rst.test_offline(true, mean, gen, psi)

    names = FIELD_VARS + SCORES + GROUPED + SPECTRA + ['L2_PSD', 'L2_Eflux', 'CSD_res', 'CSD_gen_res'] + list(PDFS)
    assert sorted(out.keys()) == sorted(names)
    assert out.attrs == ds.attrs
    np.testing.assert_array_equal(np.asarray(out['time'].values), np.asarray(ds['time'].values))
    for k in names:
        assert out[k].dtype == np.float32, k
    for k in FIELD_VARS[:3]:
        assert out[k].dims == ('run', 'time', 'lev', 'y', 'x')
    np.testing.assert_array_equal(out['q_forcing_advection'].values, true)
    np.testing.assert_array_equal(out['q_forcing_advection_gen'].values, gen.astype('float32'))
    np.testing.assert_array_equal(out['q_forcing_advection_res'].values, (true.astype('float64') - mean).astype('float32'))
    dims = {'spatial_': ('lev', 'y', 'x'), 'temporal_': ('time', 'lev')}
    for k in GROUPED:
        pre = next((p for p in dims if k.startswith(p)), '')
        assert out[k].dims == dims.get(pre, ('lev',)), k
    for k in SCORES:
        assert out[k].dims == ()
    for k in SPECTRA:
        assert out[k].dims == ('lev', 'k')
    for k in ('CSD_res', 'CSD_gen_res'):
        assert out[k].dims == ('k',)
    for k, d in PDFS.items():
        assert out[k].dims == (d,)
        assert out[k].coords[d].attrs['long_name'] == 'RMS units'
        np.testing.assert_allclose(np.asarray(out[k].coords[d].values), ref['points'], atol=1e-12)

    n_late = true.shape[0] * (true.shape[1] - 44) * true.shape[-1] ** 2
    for k in SCORES + GROUPED + SPECTRA + ['L2_PSD', 'L2_Eflux', 'CSD_res', 'CSD_gen_res'] + list(PDFS):
        a, b = np.asarray(out[k].values, 'float64'), np.asarray(ref[k], 'float64')
        assert a.shape == b.shape, k
        if k in PDFS:           # a value within an ulp of a bin edge may move: one count per bin at most
            assert np.abs(a - b).max() <= 1.01 / n_late / (10 / 70), k
            continue
        scale = np.nanmax(np.abs(b)) if np.isfinite(b).any() else 1.0
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-6 * scale, err_msg=k)
    if kind == 'ols':
        for k in ('q_forcing_advection_gen_res', 'PSD_gen_res', 'Eflux_gen_res', 'CSD_gen_res'):
            assert (np.asarray(out[k].values) == 0).all(), k
        assert (np.asarray(out['var_ratio'].values) == 0).all()


def test_published_offline_numbers_from_test_offline():
    """test_published_offline_metrics_are_reproduced (tests/test_gpu_online_metrics.py) with the product's
    test_offline(ds, 1000, seed=17) in place of predict + the oracle: the published numbers within 20 % + 0.01, and the
    oracle's subgrid_scores on the float32 fields test_offline returned within 1e-5 relative."""
    from oracle import metrics_ref
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression, CVAERegression, MeanVarModel
    from pyqg_generative_amd.tools.simulate import generate_subgrid_forcing
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    PUBLISHED = {'gan': (0.46184033155441284, 0.06294532194827125, 0.18853315029762688, 0.8986635),
                 'vae': (0.33586910367012024, 0.1662856531487818, 0.6100610325995228, 0.39741874),
                 'gz': (0.30553340911865234, 0.10004083600607486, 0.5773028112953991, 0.99088895)}
    ds = generate_subgrid_forcing([48], dict(EDDY_PARAMS.nx(256), log_level=0), n_members=2, seeds=[250, 251],
                                  operators=('Operator1',), dealias='none')['Operator1-48']
    for kind, cls in (('gan', CGANRegression), ('vae', CVAERegression), ('gz', MeanVarModel)):
        nets, xs, ys = weights.load_npz(os.path.join(ROOT, 'tests', 'golden', f'weights_{kind}.npz'), kind)
        out = cls.from_arrays(nets, xs, ys).test_offline(ds, 1000, seed=17)
        got = tuple(float(out[k].values) for k in ('L2_mean', 'L2_total', 'L2_residual')) + \
            (float(np.asarray(out['var_ratio'].values).mean()),)
        print(f'\n{kind}: {got} (published {PUBLISHED[kind]})')
        for g, p in zip(got, PUBLISHED[kind]):
            assert abs(g - p) <= 0.2 * p + 0.01, (kind, got, PUBLISHED[kind])
        sc = metrics_ref.subgrid_scores(*(np.asarray(out['q_forcing_advection' + s].values) for s in ('', '_mean', '_gen')))
        ora = (sc['L2_mean'], sc['L2_total'], sc['L2_residual'], float(sc['var_ratio'].mean()))
        np.testing.assert_allclose(got, ora, rtol=1e-5)
