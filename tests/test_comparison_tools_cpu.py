"""CPU: tools/comparison_tools.py without a GPU — the reference's key lists and scores, the operator check, the spectral
half of coarsegrain_reference_dataset and the spectral RMSE against oracle/metrics_ref.py, and the refusals of the
W1 entry points of the C ABI (they return before any device call)."""
import ctypes as C

import numpy as np
import pytest

from oracle import metrics_ref
from oracle.qg_ref import QGModelRef

REFERENCE_DISTRIB_KEYS = ['distrib_diff_q1', 'distrib_diff_q2', 'distrib_diff_u1', 'distrib_diff_u2', 'distrib_diff_v1',
                          'distrib_diff_v2', 'distrib_diff_KE1', 'distrib_diff_KE2', 'distrib_diff_Ens1',
                          'distrib_diff_Ens2']
REFERENCE_SPECTRAL_KEYS = ['spectral_diff_KEspec1', 'spectral_diff_KEspec2', 'spectral_diff_KEflux',
                           'spectral_diff_APEflux', 'spectral_diff_APEgenspec', 'spectral_diff_KEfrictionspec',
                           'spectral_diff_Eflux']


def _ct():
    from pyqg_generative_amd.tools import comparison_tools
    return comparison_tools


def test_key_lists_are_the_reference_lists():
    ct = _ct()
    assert ct.DISTRIB_KEYS == REFERENCE_DISTRIB_KEYS
    assert ct.SPECTRAL_KEYS == REFERENCE_SPECTRAL_KEYS


def test_scores():
    ct = _ct()
    d = {k: float(i + 1) for i, k in enumerate(REFERENCE_DISTRIB_KEYS)}
    d.update({'spectral_diff_KEspec1': 0.5, 'spectral_diff_Eflux': 1.5, 'other': 100.})
    assert ct.distrib_score(d) == pytest.approx(5.5)
    assert ct.spectral_score(d) == pytest.approx(1.0)
    assert np.isnan(ct.distrib_score({'other': 1.0}))
    assert np.isnan(ct.spectral_score({}))
    assert np.isnan(ct.distrib_score({'spectral_diff_KEspec1': 1.0}))


def test_unknown_operator_is_refused():
    ct = _ct()
    for op in ('Operator3', 'operator1', None):
        with pytest.raises(ValueError, match='operator must be Operator1 or Operator2'):
            ct.coarsegrain_reference_dataset({}, 48, op)
        with pytest.raises(ValueError, match='operator must be Operator1 or Operator2'):
            ct.coarsegrain_spectrum(np.zeros((96, 49)), 48, op)


@pytest.mark.parametrize('operator', ['Operator1', 'Operator2'])
def test_coarse_spectra_match_oracle(operator):
    ct = _ct()
    rs = np.random.RandomState(3)
    hires = {'KEspec': rs.rand(4, 2, 96, 49), 'KEflux': rs.randn(4, 96, 49)}
    want = metrics_ref.coarsegrain_reference_spectra(hires, 48, operator)
    for name, a in hires.items():
        np.testing.assert_allclose(ct.coarsegrain_spectrum(a, 48, operator), want[name], rtol=1e-15, atol=0)   # x*f*f vs x*f**2


def test_operators_4_and_5_only_cut_the_spectra():
    ct = _ct()
    a = np.random.RandomState(4).rand(2, 2, 64, 33)
    for op in ('Operator4', 'Operator5'):
        out = ct.coarsegrain_spectrum(a, 32, op)
        np.testing.assert_array_equal(out, np.concatenate((a[..., :16, :17], a[..., -16:, :17]), axis=-2))


@pytest.mark.parametrize('N', [32, 48, 64, 96, 256])
def test_two_thirds_nyquist_and_spectral_rmse(N):
    from pyqg_generative_amd.tools.spectral_tools import _Grid, twothirds_nyquist
    g, ref = _Grid(N), QGModelRef(nx=N)
    np.testing.assert_array_equal(g.filtr, ref.filtr)
    assert twothirds_nyquist(g) == metrics_ref.twothirds_nyquist(ref)
    ct = _ct()
    rs = np.random.RandomState(N)
    s1, s2 = rs.rand(N, N // 2 + 1), rs.rand(48, 25)
    got = ct._spectral_rmse(s1, s2)
    want = metrics_ref.spectral_rmse(s1, s2)
    np.testing.assert_allclose(got, want, rtol=1e-13)


def test_w1_workspace_query():
    from pyqg_generative_amd._lib import lib
    nbytes = C.c_size_t()
    assert lib.qgx_w1_workspace(1000, 10, 64, C.byref(nbytes)) == 0
    b64 = nbytes.value
    assert b64 >= 1000 * 8
    assert lib.qgx_w1_workspace(1000, 10, 32, C.byref(nbytes)) == 0
    assert 1000 * 4 <= nbytes.value < b64
    assert lib.qgx_w1_workspace(10, 1000, 64, C.byref(nbytes)) == 0 and nbytes.value == b64
    assert lib.qgx_w1_workspace(37748736, 37748736, 64, C.byref(nbytes)) == 0
    assert nbytes.value >= 37748736 * 8


def test_w1_refusals_before_any_device_call():
    from pyqg_generative_amd._lib import lib, W1_IDENTITY, W1_SUMSQ2, W1_SQUARE
    nbytes = C.c_size_t()
    fake = C.c_void_p(256)       # never dereferenced: every call below must be refused first
    assert lib.qgx_w1_workspace(0, 5, 64, C.byref(nbytes)) == -1
    assert lib.qgx_w1_workspace(5, 0, 64, C.byref(nbytes)) == -1
    assert lib.qgx_w1_workspace(5, 5, 16, C.byref(nbytes)) == -1

    def keys(is_double=1, feature=W1_IDENTITY, key_bits=64, R=1, T=1, P=10, y=fake):
        return lib.qgx_w1_keys(fake, y, is_double, feature, key_bits, R, T, P, 0, 0, fake, fake, fake, None)
    assert keys(is_double=2) == -1
    assert keys(feature=3) == -1 and keys(feature=-1) == -1
    assert keys(key_bits=32) == -1                          # 32-bit keys: float identity only
    assert keys(is_double=0, feature=W1_SQUARE, key_bits=32) == -1
    assert keys(is_double=0, feature=W1_SUMSQ2, y=None) == -1
    assert keys(R=0) == -1 and keys(T=0) == -1 and keys(P=0) == -1 and keys(P=-4) == -1
    assert b'qgx_w1_keys' in lib.qgx_last_error()

    def sorted_(nu=10, nv=10, key_bits=64, work_bytes=None):
        if work_bytes is None:
            assert lib.qgx_w1_workspace(max(nu, 1), max(nv, 1), 64, C.byref(nbytes)) == 0
            work_bytes = nbytes.value
        return lib.qgx_w1_sorted(fake, nu, None, fake, nv, None, key_bits, fake, work_bytes, fake, None)
    assert sorted_(nu=0) == -1 and sorted_(nv=0) == -1
    assert sorted_(key_bits=8) == -1
    assert lib.qgx_w1_workspace(10, 10, 64, C.byref(nbytes)) == 0
    assert sorted_(work_bytes=nbytes.value - 1) == -1
    assert b'work space' in lib.qgx_last_error()
    assert lib.qgx_spec_curl(fake, fake, fake, 1, 47, 1e6, None) == -1


def test_empty_inputs_raise_value_error():
    ct = _ct()
    with pytest.raises(ValueError):
        ct.wasserstein_distance(np.array([]), np.array([1.0]))
    with pytest.raises(ValueError):
        ct.wasserstein_distance([1.0, 2.0], [])
