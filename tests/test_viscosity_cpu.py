"""No GPU: the molecular-viscosity closure (models/laplace.py, qgx_set_viscosity) — its ABI surface and, on the CPU oracle,
the spectral form of the term against the transform-round-trip form the reference's Laplace class evaluates
(pyqg_generative/tools/simulate.py:207-225), restated here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import qg_ref


class RoundTripLaplace:
    """Test-local restatement of the reference's closure: the Laplacian applied in spectral space, the result taken to
    real space (the model transforms it forward again):  nu lap(q)  or  nu lap(lap(psi))."""

    def __init__(self, nu, PV):
        self.nu, self.PV = nu, PV

    def __call__(self, m):
        lap = -(m.k ** 2 + m.l ** 2)
        field = m.qh if self.PV else lap * m.ph
        return self.nu * m.ifft(lap * field)


def _ic(N, seed):
    m = qg_ref.QGModelRef(nx=N)
    rs = np.random.RandomState(seed)
    q = rs.randn(2, N, N) * np.array([8e-6, 1e-6])[:, None, None]
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1]), axes=(-2, -1)) * 3.0


def _run(N, param, filterfac, nsteps=12):
    m = qg_ref.QGModelRef(nx=N, dt=14400., filterfac=filterfac, parameterization=param)
    m.set_q(_ic(N, N))
    out = []
    for _ in range(nsteps):
        m._step_forward()
        out.append(m.qh.copy())
    return out


def test_header_declares_and_lib_binds_the_viscosity_entry_points():
    from pyqg_generative_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for fn in ('qgx_set_viscosity', 'qgx_get_viscosity'):
        assert re.search(r'^int %s\(' % fn, header, flags=re.M), fn
        assert fn in bound and hasattr(_lib.lib, fn), fn
    assert 'simulate.py:207' in header                     # the reference citation of the entry point
    # viscosity is a property of the handle: the two pinned structs did not grow
    assert C.sizeof(_lib.qgx_param) == 64 and C.sizeof(_lib.qgx_config) == 96
    assert 'nu' not in {f[0] for f in _lib.qgx_param._fields_} | {f[0] for f in _lib.qgx_config._fields_}


@pytest.mark.parametrize('filterfac', [23.6, 1e20])
@pytest.mark.parametrize('PV', [False, True])
@pytest.mark.parametrize('N', [32, 48])
def test_spectral_form_equals_the_round_trip_form_on_the_oracle(N, PV, filterfac):
    from pyqg_generative_amd.models import Laplace
    nu = 50.
    ours = _run(N, Laplace(nu, PV), filterfac)
    ref = _run(N, RoundTripLaplace(nu, PV), filterfac)
    off = _run(N, None, filterfac)
    for s, (a, b) in enumerate(zip(ours, ref)):
        # the two forms differ by rounding alone (measured 3 ... 6e-16 of max|qh|; the margin covers other FFT builds)
        assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), (s, np.abs(a - b).max() / np.abs(b).max())
    # ... and the term is no rounding matter at this nu: a test of it cannot pass with the term missing
    assert np.abs(ours[-1] - off[-1]).max() > 1e-2 * np.abs(off[-1]).max()


def test_call_returns_the_real_space_field_of_the_formulas():
    from pyqg_generative_amd.models import Laplace
    N = 32
    m = qg_ref.QGModelRef(nx=N)
    m.set_q(_ic(N, 1))
    m._invert()
    K2 = m.wv2
    np.testing.assert_array_equal(Laplace(30., False)(m), m.ifft(30. * (K2 * K2) * m.ph))
    np.testing.assert_array_equal(Laplace(30., True)(m), m.ifft(-30. * K2 * m.qh))
    assert Laplace(30.)(m).shape == (2, N, N)
    with pytest.raises(ValueError):
        Laplace([1., 2.])(m)            # one nu per member needs a model with that many members


def test_a_weighted_laplace_is_a_laplace_of_the_weighted_viscosity():
    from pyqg_generative_amd.models import Laplace
    from pyqg_generative_amd.qgmodel import QParameterization
    half = 0.5 * Laplace(40., True)
    assert isinstance(half, Laplace) and isinstance(half, QParameterization)
    assert half.nu == 20. and half.PV is True and (Laplace(40.) * 0.5).nu == 20.
    a, b = _run(32, 0.5 * Laplace(40.), 23.6), _run(32, Laplace(20.), 23.6)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    per_member = 2. * Laplace([0., 10., 25.], fused=False)
    np.testing.assert_array_equal(per_member.nu, [0., 20., 50.])
    assert per_member.fused is False


def test_repr_has_the_reference_form():
    from pyqg_generative_amd.models import Laplace
    assert repr(Laplace()) == 'Laplace(nu=0.0, PV=False)'
    assert repr(Laplace(50, PV=True)) == 'Laplace(nu=50, PV=True)'
    assert str({'parameterization': Laplace(12.5)}) == "{'parameterization': Laplace(nu=12.5, PV=False)}"
    assert Laplace.parameterization_type == 'q_parameterization'
