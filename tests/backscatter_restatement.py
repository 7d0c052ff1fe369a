"""Test-local restatement of the Jansen-Held backscatter closure as pyqg 0.7.2 writes it (parameterizations.py::
Smagorinsky.__call__(m, just_viscosity=True) and BackscatterBiharmonic.__call__(m)), a callable for oracle.qg_ref.QGModelRef.
Written from the formulas alone, field by field, through m.fft / m.ifft: every transform pyqg makes is made here, nothing
is simplified (Syy is its own transform, both means are taken in real space)."""
import numpy as np


class BackscatterRestated:
    def __init__(self, smag_constant=0.08, back_constant=0.99, eps=1e-32):
        self.C_S, self.C_B, self.eps = smag_constant, back_constant, eps

    def smagorinsky_viscosity(self, m):
        uh, vh = m.fft(m.u), m.fft(m.v)
        Sxx = m.ifft(uh * m.ik)
        Syy = m.ifft(vh * m.il)
        Sxy = 0.5 * m.ifft(uh * m.il + vh * m.ik)
        return (self.C_S * m.dx) ** 2 * np.sqrt(2 * (Sxx ** 2 + Syy ** 2 + 2 * Sxy ** 2))

    def parts(self, m):
        """-> (dq, D, llp, psi, R)"""
        lap = m.ik ** 2 + m.il ** 2
        psi = m.ifft(m.ph)
        llp = m.ifft(lap ** 2 * m.ph)
        D = -m.ifft(lap * m.fft(llp * m.dx ** 2 * self.smagorinsky_viscosity(m)))
        num = sum(m.Hi[i] * np.mean(psi[i] * D[i]) for i in range(2))
        den = sum(m.Hi[i] * np.mean(psi[i] * llp[i]) for i in range(2))
        R = num / (den + self.eps)
        return D - self.C_B * llp * R, D, llp, psi, R

    def __call__(self, m):
        return self.parts(m)[0]


def inverted(N, q, **params):
    """an oracle model holding q with ph, u, v of that state"""
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N, **params)
    m.set_q(q)
    m._invert()
    return m
