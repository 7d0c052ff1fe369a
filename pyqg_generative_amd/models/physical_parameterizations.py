"""Physical parameterizations: the fourth kind of online run of the reference (``--parameterization BackscatterEddy``,
pyqg_generative/tools/simulate.py:243-244 runs ``model_weight * eval(name)()`` with the classes of
pyqg_generative/models/physical_parameterizations.py), the baseline the generative models are compared against.

``BackscatterBiharmonic`` restates pyqg 0.7.2 parameterizations.py::{Smagorinsky.__call__(m, just_viscosity=True),
BackscatterBiharmonic.__call__} (Jansen & Held 2014), evaluated behind ``_invert``:

    uh = fft(u); vh = fft(v)
    Sxx = ifft(uh ik); Syy = ifft(vh il); Sxy = ifft(uh il + vh ik) / 2
    nu  = (C_S dx)^2 sqrt(2 (Sxx^2 + Syy^2 + 2 Sxy^2))
    lap = ik^2 + il^2;  psi = ifft(ph);  llp = ifft(lap^2 ph)
    D   = -ifft(lap fft(llp dx^2 nu))
    R   = sum_i H_i <psi_i D_i> / (sum_i H_i <psi_i llp_i> + eps)        one scalar per member
    dq  = D - C_B llp R

Attached to a ``QGModel`` of this package with ``fused`` on, the object is NOT called per step: (C_S, C_B, eps) go to the
engine once (``EnsembleEngine.set_backscatter``) and every step recomputes the closure on the device from the current
state (csrc/backscatter.hip), so the run steps like an unparameterized one — multi-step calls, no host call.  The two
constants may be one value per ensemble member: a (C_S, C_B) tuning sweep is one ensemble.  ``__call__(m)`` keeps the
stand-alone numpy semantics on any pyqg-like model through ``m.fft`` / ``m.ifft``; ``fused=False`` makes a ``QGModel`` use
that path too (one host call per step: the A/B reference of tests and bench_tools/backscatter_time.py).

``ZannaBolton``, ``ReynoldsStress``, ``HybridSymbolic`` and ``ADM`` of the reference wrap classes of a pyqg fork
(``ZannaBolton2020_q``, ``Reynolds_stress``, ``HybridSymbolic``, ``ADM``) that is not part of the reference tree: there is
nothing to restate them from, and they raise ``NotImplementedError``.
"""
import numpy as np

from ..qgmodel import QParameterization, _unwrap
from .parameterization import Parameterization


class BackscatterBiharmonic(QParameterization):
    def __init__(self, smag_constant=0.08, back_constant=0.99, eps=1e-32, fused=True):
        self.smag_constant = smag_constant
        self.back_constant = back_constant
        self.eps = eps
        self.fused = bool(fused)

    @staticmethod
    def _like(c, field, name):
        """a constant shaped to multiply a ([B,] 2, ny, nx) field: a scalar, or one value per member on the leading axis"""
        c = np.asarray(c, dtype='float64')
        if c.ndim == 0:
            return float(c)
        if c.size == 1 and field.ndim == 3:
            return float(c.reshape(-1)[0])
        if field.ndim != 4 or c.shape != (field.shape[0],):
            raise ValueError(f'{name} has shape {c.shape}: one value per member needs a model with that many members')
        return c[:, None, None, None]

    def __call__(self, m, ratio=False):
        ik, il = np.asarray(m.ik), np.asarray(m.il)
        uh, vh = m.fft(np.asarray(m.u)), m.fft(np.asarray(m.v))
        Sxx, Syy, Sxy = m.ifft(uh * ik), m.ifft(vh * il), 0.5 * m.ifft(uh * il + vh * ik)
        nu = (self._like(self.smag_constant, Sxx, 'smag_constant') * m.dx) ** 2 * np.sqrt(2 * (Sxx ** 2 + Syy ** 2 + 2 * Sxy ** 2))
        lap = ik ** 2 + il ** 2
        ph = np.asarray(m.ph)
        psi, llp = m.ifft(ph), m.ifft(lap ** 2 * ph)
        D = -m.ifft(lap * m.fft(llp * m.dx ** 2 * nu))
        H = np.asarray(m.Hi, dtype='float64')[:, None, None]

        def budget(x):
            return (H * (psi * x).mean(axis=(-2, -1), keepdims=True)).sum(axis=-3, keepdims=True)
        R = budget(D) / (budget(llp) + self.eps)
        dq = D - self._like(self.back_constant, llp, 'back_constant') * llp * R
        return (dq, R[..., 0, 0, 0]) if ratio else dq

    def __mul__(self, w):
        """w * closure is BackscatterBiharmonic(C_S sqrt(w), C_B): dq is linear in C_S^2 (D is, and R with it)"""
        w = float(w)
        if w < 0:
            raise ValueError(f'a backscatter closure cannot be weighted by {w}: its weight is a factor of C_S^2')
        cs = np.asarray(self.smag_constant, dtype='float64') * np.sqrt(w)
        return BackscatterBiharmonic(float(cs) if cs.ndim == 0 else cs, self.back_constant, self.eps, self.fused)
    __rmul__ = __mul__

    def __repr__(self):
        return f'BackscatterBiharmonic(smag_constant={self.smag_constant}, back_constant={self.back_constant}, eps={self.eps})'


def fused_closure(parameterization):
    """-> the BackscatterBiharmonic a (weighted) BackscatterBiharmonic, or a (weighted) PhysicalParameterization that wraps
    one, amounts to — the weight folded into C_S — or None for anything else"""
    param, weight = _unwrap(parameterization)
    if isinstance(param, PhysicalParameterization):
        param = getattr(param, 'subgrid_model', None)
    if not isinstance(param, BackscatterBiharmonic):
        return None
    return param if weight == 1.0 else weight * param


class PhysicalParameterization(Parameterization):
    """A deterministic closure behind the reference's Parameterization interface: no latent noise, the snapshot
    prediction is the closure itself, offline prediction has mean = sample and var = 0."""
    subgrid_model = None
    device_generator = None      # no network: fused, the closure runs inside qgx_step; else QGModel takes the host plug-in path
    PREDICT_CHUNK = 128          # snapshots evaluated as members of one engine

    def generate_latent_noise(self, ny, nx):
        return 0

    def predict_snapshot(self, m, noise=None):
        return self.subgrid_model(m)

    def __call__(self, m):
        """the plug-in call of models/parameterization.py:23-34 with this class's hooks"""
        if getattr(m, 'sampling_type', 'AR1') == 'deterministic':
            S = self.predict_mean_snapshot(m)
        elif not hasattr(m, 'noise_sampler') or m.noise_sampler.update(lambda: self.generate_latent_noise(m.ny, m.nx)):
            S = np.asarray(self.predict_snapshot(m, getattr(getattr(m, 'noise_sampler', None), 'noise', 0)), dtype='float64')
        else:
            return self._last
        self._last = S - S.mean(axis=(-2, -1), keepdims=True)
        return self._last

    def predict(self, ds, M=1000, device=0):
        """Offline prediction for a dataset with q (run, time, lev, y, x): the reference builds one model per snapshot;
        here all run x time snapshots are members of one ensemble per chunk and the closure is one
        ``backscatter_forcing`` call.  The model parameters are those of ds.attrs['pyqg_params'] (pyqg's defaults without it)."""
        import ast
        import torch
        from ..engine import EnsembleEngine, PYQG_DEFAULTS
        from ..tools.simulate import dataset_backend
        c = self.subgrid_model
        if not isinstance(c, BackscatterBiharmonic):
            raise NotImplementedError('predict needs a BackscatterBiharmonic as subgrid_model')
        if np.ndim(c.smag_constant) or np.ndim(c.back_constant):
            raise ValueError('predict takes scalar constants: the members of its ensembles are the snapshots')
        xr = dataset_backend()
        X = np.asarray(ds['q'].values)
        if X.ndim != 5 or X.shape[2] != 2 or X.shape[-1] != X.shape[-2]:
            raise ValueError(f'predict expects q (run, time, lev=2, y, x) on a square grid, got {X.shape}')
        given = ds.attrs.get('pyqg_params')
        if given is not None and not isinstance(given, dict):
            try:
                given = ast.literal_eval(given)
            except (ValueError, SyntaxError) as e:
                raise ValueError("ds.attrs['pyqg_params'] is not a dictionary of plain values") from e
        params = {k: v for k, v in (given or {}).items() if k in PYQG_DEFAULTS}
        snaps = X.reshape((-1,) + X.shape[-3:]).astype('float64')
        n, nx = len(snaps), X.shape[-1]
        chunk = min(n, self.PREDICT_CHUNK)
        Y = np.zeros(snaps.shape, dtype=X.dtype)
        eng = EnsembleEngine(nx=nx, n_members=chunk, device=device, **params)
        try:
            eng.set_backscatter(float(c.smag_constant), float(c.back_constant), c.eps)
            for s0 in range(0, n, chunk):
                q = np.zeros((chunk,) + snaps.shape[1:])          # (a short last chunk is filled with states at rest)
                q[:min(chunk, n - s0)] = snaps[s0:s0 + chunk]
                eng.set_q(q)
                S = eng.backscatter_forcing().cpu().numpy()
                Y[s0:s0 + chunk] = S[:min(chunk, n - s0)]
        finally:
            eng.close()
        Y = Y.reshape(X.shape)
        dims = ['run', 'time', 'lev', 'y', 'x']
        return xr.Dataset({'q_forcing_advection': (dims, Y), 'q_forcing_advection_mean': (dims, Y),
                           'q_forcing_advection_var': (dims, Y * 0)})


class BackscatterEddy(PhysicalParameterization):
    def __init__(self, fused=True):
        self.subgrid_model = BackscatterBiharmonic(np.sqrt(0.007), 1.2, fused=fused)


class BackscatterJet(PhysicalParameterization):
    def __init__(self, fused=True):
        self.subgrid_model = BackscatterBiharmonic(np.sqrt(0.005), 0.8, fused=fused)


class _ForkOnly(PhysicalParameterization):
    wraps = None

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            f'{type(self).__name__} wraps {self.wraps} of a pyqg fork that is not part of the reference tree: there is '
            'nothing to restate it from (available physical parameterizations: BackscatterEddy, BackscatterJet)')


class ZannaBolton(_ForkOnly):
    wraps = 'ZannaBolton2020_q'


class ReynoldsStress(_ForkOnly):
    wraps = 'Reynolds_stress'


class HybridSymbolic(_ForkOnly):
    wraps = 'HybridSymbolic'


class ADM(_ForkOnly):
    wraps = 'ADM'
