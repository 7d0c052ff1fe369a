"""CPU: the offline metrics without a GPU — the test-side restatement (tests/offline_restatement.py) against the oracle's
subgrid_scores and against np.histogram, the refusals of the offline entry points of the C ABI (they return before any
device call), and test_offline's input checks (raised before predict)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from oracle import metrics_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restatement():
    spec = importlib.util.spec_from_file_location('offline_restatement',
                                                  os.path.join(ROOT, 'tests', 'offline_restatement.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fields(seed, R=2, T=5, N=16):
    rs = np.random.RandomState(seed)
    true = rs.randn(R, T, 2, N, N).astype('float32')
    mean = 0.6 * true + 0.3 * rs.randn(R, T, 2, N, N)
    gen = mean + 0.5 * rs.randn(R, T, 2, N, N)
    return true, mean, gen


def test_restatement_subgrid_scores_equal_the_oracle():
    rst = _restatement()
    for seed in (0, 1):
        true, mean, gen = _fields(seed)
        a = rst.subgrid_scores(true, mean, gen)
        b = metrics_ref.subgrid_scores(true, mean, gen)
        for k in ('L2_mean', 'L2_total', 'L2_residual'):
            assert a[k] == pytest.approx(b[k], rel=1e-12), k
        np.testing.assert_allclose(a['var_ratio'], b['var_ratio'], rtol=1e-12)


def test_restatement_histogram_equals_numpy_on_edges():
    rst = _restatement()
    rs = np.random.RandomState(3)
    edges = np.linspace(-5, 5, 71)
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), rs.randn(5000) * 2,
                        [-7., 7., np.nan]])
    np.testing.assert_array_equal(rst.uniform_histogram(x, -5.0, 5.0, 70), np.histogram(x, bins=70, range=(-5, 5))[0])
    e2 = np.linspace(-1.3, 2.9, 31)
    y = np.concatenate([e2, rs.rand(3000) * 5 - 1.8])
    np.testing.assert_array_equal(rst.uniform_histogram(y, -1.3, 2.9, 30), np.histogram(y, bins=30, range=(-1.3, 2.9))[0])


def test_offline_refusals_before_any_device_call():
    from pyqg_generative_amd._lib import lib, WORK_SPECTRA, WORK_MOMENTS, WORK_HISTOGRAM, HIST_SCALE_STD
    nbytes = C.c_size_t()
    fake = C.c_void_p(256)       # never dereferenced: every call below must be refused first
    assert lib.qgx_offline_workspace(WORK_SPECTRA, 0, 0, 64, 0, C.byref(nbytes)) == 0
    assert nbytes.value == 32 * 2 * 22 * 64 * 33 * 8
    assert lib.qgx_offline_workspace(WORK_SPECTRA, 0, 0, 63, 0, C.byref(nbytes)) == -1
    assert lib.qgx_offline_workspace(WORK_MOMENTS, 0, 5, 64, 0, C.byref(nbytes)) == -1
    assert lib.qgx_offline_workspace(WORK_HISTOGRAM, 0, 0, 0, -1, C.byref(nbytes)) == -1
    assert lib.qgx_offline_workspace(WORK_HISTOGRAM, 0, 0, 0, 5000, C.byref(nbytes)) == -1
    assert lib.qgx_offline_workspace(7, 1, 1, 64, 0, C.byref(nbytes)) == -1
    assert lib.qgx_offline_workspace(WORK_SPECTRA, 0, 0, 64, 0, None) == -1

    def spectra(th=fake, S=4, N=64, s0=0, T=4, t0=0, acc=1, acc_dev=fake):
        return lib.qgx_offline_spectra(th, fake, fake, None, S, N, s0, T, t0, acc, acc_dev, None)
    assert spectra(th=None) == -1 and spectra(acc_dev=None) == -1
    assert spectra(S=0) == -1 and spectra(N=63) == -1 and spectra(N=0) == -1 and spectra(T=0) == -1
    assert spectra(s0=-1) == -1 and spectra(t0=-1) == -1 and spectra(acc=2) == -1
    assert b'qgx_offline_spectra' in lib.qgx_last_error()
    assert lib.qgx_offline_spectra_finish(None, 64, fake, None) == -1
    assert lib.qgx_offline_spectra_finish(fake, 7, fake, None) == -1

    assert lib.qgx_offline_workspace(WORK_MOMENTS, 2, 3, 16, 0, C.byref(nbytes)) == 0
    mom_bytes = nbytes.value

    def moments(t=fake, dtypes=0, R=2, T=3, N=16, work_bytes=mom_bytes):
        return lib.qgx_offline_moments(t, fake, fake, dtypes, R, T, N, fake, work_bytes, fake, None)
    assert moments(t=None) == -1 and moments(dtypes=8) == -1 and moments(dtypes=-1) == -1
    assert moments(R=0) == -1 and moments(T=-2) == -1 and moments(N=0) == -1
    assert moments(work_bytes=mom_bytes - 1) == -1
    assert b'work space' in lib.qgx_last_error()

    assert lib.qgx_offline_workspace(WORK_HISTOGRAM, 0, 0, 0, 70, C.byref(nbytes)) == 0
    hb = nbytes.value

    def hist(is_double=1, R=1, T=3, nlev=2, P=16, z=0, t0=0, edges=fake, nbins=70, flags=0, work_bytes=hb, x=fake):
        return lib.qgx_histogram(x, is_double, R, T, nlev, P, z, t0, edges, nbins, flags, 1.0, fake, work_bytes, fake,
                                 fake, None)
    assert hist(is_double=2) == -1 and hist(x=None) == -1 and hist(edges=None) == -1
    assert hist(flags=HIST_SCALE_STD) == -1 and hist(flags=4) == -1 and hist(flags=-1) == -1
    assert hist(nbins=0) == -1 and hist(nbins=5000) == -1
    assert hist(R=0) == -1 and hist(P=0) == -1 and hist(z=2) == -1 and hist(z=-1) == -1
    assert hist(t0=3) == -1 and hist(t0=-1) == -1 and hist(nlev=0) == -1
    assert hist(work_bytes=hb - 1) == -1
    assert b'qgx_histogram' in lib.qgx_last_error()


def test_test_offline_input_checks_raise_before_predict():
    from pyqg_generative_amd.models.parameterization import Parameterization
    from pyqg_generative_amd.tools import xr_lite
    from pyqg_generative_amd.tools.computational_tools import check_fields

    class _Model(Parameterization):
        kind = 'gan'

        def predict(self, ds, M=1000, **kw):
            raise AssertionError('predict must not run on refused input')

    model = _Model.__new__(_Model)

    def ds_of(shape, drop=None):
        dims = ['run', 'time', 'lev', 'y', 'x'][-len(shape):]
        ds = xr_lite.Dataset({k: (dims, np.zeros(shape, 'float32')) for k in ('q', 'q_forcing_advection', 'psi')
                              if k != drop})
        return ds
    for shape in ((3, 2, 16, 16), (1, 3, 3, 16, 16), (1, 3, 2, 16, 32), (1, 3, 2, 14, 14), (1, 3, 2, 10, 10),
                  (1, 3, 2, 1024, 1024), (0, 3, 2, 16, 16)):
        with pytest.raises(ValueError):
            model.test_offline(ds_of(shape), 10)
    with pytest.raises(ValueError):
        model.test_offline(ds_of((1, 3, 2, 16, 16), drop='psi'), 10)
    assert check_fields(np.zeros((1, 3, 2, 48, 48))) == (1, 3, 2, 48, 48)
    with pytest.raises(ValueError):
        check_fields(np.zeros((1, 3, 2, 48, 48)), np.zeros((1, 4, 2, 48, 48)))
