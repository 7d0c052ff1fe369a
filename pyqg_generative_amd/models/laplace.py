"""Molecular viscosity as a q-parameterization: the third kind of online run of the reference
(``--molecular_viscosity``, pyqg_generative/tools/simulate.py:206-236), beside the unparameterized
runs and the runs with a trained model.

Per spectral element, with K^2 = k^2 + l^2 (the model's ``wv2``; the Laplacian is -K^2):

    PV = False:  dqh_k =  nu K^4 ph_k      nu lap(zeta),  zeta = lap(psi)
    PV = True :  dqh_k = -nu K^2 qh_k      nu lap(q)

Attached to a ``QGModel`` of this package the object is NOT called per step: the model hands (nu, PV)
to the engine once (``EnsembleEngine.set_viscosity``) and the step kernels add the term to the
tendency, so the run steps like an unparameterized one — multi-step launches, no host call, no
transform.  ``nu`` may be one value per ensemble member: a viscosity sweep is one ensemble.
``__call__(m)`` keeps the stand-alone plug-in semantics (a real-space PV tendency from ``m.qh`` /
``m.ph`` / ``m.ifft``) for any pyqg-like model; ``fused=False`` makes a ``QGModel`` use that path too
(one host call per step: the A/B reference of tests and bench_tools/visc_time.py).
"""
import numpy as np

from ..qgmodel import QParameterization


class Laplace(QParameterization):
    def __init__(self, nu=0., PV=False, fused=True):
        self.nu = nu
        self.PV = PV
        self.fused = bool(fused)

    def _nu_like(self, field):
        """nu shaped to multiply a ([B,] 2, ny, nk) spectral field: a scalar, or one value per member on the leading axis"""
        nu = np.asarray(self.nu, dtype='float64')
        if nu.ndim == 0:
            return float(nu)
        if nu.size == 1 and field.ndim == 3:
            return float(nu.reshape(-1)[0])
        if field.ndim != 4 or nu.shape != (field.shape[0],):
            raise ValueError(f'nu has shape {nu.shape}: one value per member needs a model with that many members')
        return nu[:, None, None, None]

    def spectral(self, m):
        """the term as the step kernels form it: dqh ([B,] 2, ny, nk) complex"""
        K2 = np.asarray(m.wv2)
        if self.PV:
            qh = np.asarray(m.qh)
            return -self._nu_like(qh) * K2 * qh
        ph = np.asarray(m.ph)
        return self._nu_like(ph) * (K2 * K2) * ph

    def __call__(self, m):
        return m.ifft(self.spectral(m))

    def __mul__(self, w):
        """w * Laplace(nu) is Laplace(w nu): the weight of a viscosity is a viscosity"""
        nu = np.asarray(self.nu, dtype='float64') * float(w)
        return Laplace(float(nu) if nu.ndim == 0 else nu, self.PV, self.fused)
    __rmul__ = __mul__

    def __repr__(self):
        return f"Laplace(nu={self.nu}, PV={self.PV})"
