"""GPU: every grid size qgx_create admits — nx = 2^a 3^b, even, 8 ... 512: 25 sizes — and not only the eight with compile-time
specialisations (32, 48, 64, 96, 128, 256, 384; 192 in the transforms).  The other seventeen run the generic run-time-N
kernels (spectral_small.hip `<0>` instances up to 96, spectral_large.hip above), radix-3 / 6 / 12 passes WITH twiddles,
digit-reversal maps of three to five unequal radices, the large path with 4 and with 2 lines per workgroup, and the
composed diagnostics increment.  Here:

  * the admitted set itself;
  * transforms (plan-only handles and the model's setters) on white noise and on unit impulses with closed-form spectra,
    against numpy at 1e-12 of the maximum and, up to N = 72, against a direct O(N^2) DFT in extended precision
    (GPU error <= 4 x numpy's own error + 1e-15 of the maximum);
  * unparameterized steps (Euler, AB2, AB3 start-up, two steady AB3 steps) against the oracle, 1e-12 x steps;
  * every launch shape of the generic small kernel (member counts 1 ... 257, layer split, thread counts);
  * an external forcing in the tendency; the sixteen time-averaged diagnostics; the 512 x 512 kernel options;
  * the AndrewCNN generator's grid-size contract: a size is either run (float32-class against the float64 oracle CNN, one
    online step against the oracle) or refused by qgx_generator_forward, qgx_cnn_forward and qgx_step before anything is
    launched or changed.

Tolerances are the project's: F64_TOL = 1e-12 of the field maximum (x steps), 1e-11 / 1e-10 for derived fields, 1e-9 for
the diagnostics, 2e-5 / 5e-5 / 2e-6 for the float32 generator (tests/test_gpu_parity.py, tests/test_gpu_diagnostics.py).
Every test prints its worst error (pytest -s) — DESIGN's testing section holds a table of them."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from conftest import GOLDEN, golden, load_generator
from oracle import qg_ref, gen_ref, samplers_ref

F64_TOL = 1e-12
# float32 generator: forcing S (of the layer maximum) and qh after one step.  TIGHT where the measured worst error is at most
# a third of it (every admitted kind, size and member count: S <= 3.7e-6, qh <= 4.9e-8) except GZ at 128 x 128 with two
# members, which measured S 3.8e-5, qh 2.8e-7 (its 5x5 layer's kernel at that size carries 8e-6 of the net output) and keeps
# LOOSE, the earlier bound.  DESIGN.md section 4
TIGHT, LOOSE = (2e-5, 5e-7), (5e-5, 2e-6)
JET = dict(dt=7200., rek=7e-8, delta=0.1, beta=1e-11)      # tools/parameters.py:26-27,37

ALL = [8, 12, 16, 18, 24, 32, 36, 48, 54, 64, 72, 96, 108, 128, 144, 162, 192, 216, 256, 288, 324, 384, 432, 486, 512]
# of these, 8, 12, 16, 18, 24, 36, 54, 72 run k_step_small<0> and its siblings; 108, 288, 324, 432 the large path with four
# lines per workgroup and no specialisation; 162, 486, 512 with two lines per workgroup: large_step_unfused always


def dt_of(N):
    """a time step the explicit scheme takes at this resolution with the amplitudes of _eddy_like_q (CFL < 0.2)"""
    return 14400. if N <= 64 else 7200. if N <= 128 else 3600. if N <= 384 else 1800.


def _engine(N, B, **kw):
    import pyqg_generative_amd as qa
    return qa.EnsembleEngine(nx=N, n_members=B, **kw)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _random_q(rs, B, N):
    return rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]


def _eddy_like_q(rs, B, N):
    """smooth fields with eddy-like amplitudes (white noise band-limited to 2/3 Nyquist)"""
    m = qg_ref.QGModelRef(nx=N)
    qh = np.fft.rfftn(_random_q(rs, B, N), axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    return np.fft.irfftn(qh, axes=(-2, -1)) * 3.0


def _members(B):
    return sorted({0, B // 2, B - 1})


# ------------------------------------------------------------------------------------------------ the admitted set
def test_admitted_grid_sizes_are_exactly_the_25_of_the_table():
    from pyqg_generative_amd._lib import QgxError
    tried = list(range(2, 516, 2)) + [7, 9]
    assert {10, 14, 20, 30, 40, 80, 100, 160, 320, 510, 514} <= set(tried)
    admitted = []
    for N in tried:
        try:
            e = _engine(N, 1, plan_only=True)
        except QgxError as err:
            assert 'qgx error -1' in str(err) and str(N) in str(err), (N, str(err))      # QGX_ERR_INVALID, naming nx
            continue
        e.close()
        admitted.append(N)
    assert admitted == ALL
    # a model (not only a plan) at both ends of the range, and the same refusal
    for N in (8, 512):
        _engine(N, 1).close()
    for N in (10, 514, 7):
        with pytest.raises(QgxError, match='qgx error -1'):
            _engine(N, 1)


# ------------------------------------------------------------------------------------------------ transforms
def _impulse_positions(N):
    """(y, x) that differ in every digit of the mixed-radix plan: the corners, the Nyquist column, thirds where they exist;
    an even count, so that impulses pair with impulses in the packed transforms"""
    pos = [(0, 0), (1, 0), (0, 1), (N - 1, N // 2)]
    if N % 3 == 0:
        pos += [(N // 3, 2 * N // 3), (N // 2, N - 1)]
    return pos


def _impulse_spectrum(N, y0, x0):
    """rfft2 of a unit impulse at (y0, x0): exp(-2 pi i (j y0 + k x0) / N), the phase reduced mod N in integers"""
    j, k = np.meshgrid(np.arange(N), np.arange(N // 2 + 1), indexing='ij')
    ang = -2.0 * np.pi * ((j * y0 + k * x0) % N) / N
    return np.cos(ang) + 1j * np.sin(ang)


def _transform_fields(N):
    """(M, N, N), M even: two white-noise fields (they excite the Nyquist row and column), then the impulses.  Two real
    fields travel through one complex transform as x + i y, so the rounding error of either is a fraction of the LARGER
    spectrum of the pair: the noise is scaled by 1 / N, which puts its spectrum at the impulses' O(1), and every bound
    below is then a bound for each field by itself"""
    rs = np.random.RandomState(7000 + N)
    pos = _impulse_positions(N)
    X = [rs.randn(N, N) / N, rs.randn(N, N) / N]
    for (y0, x0) in pos:
        f = np.zeros((N, N))
        f[y0, x0] = 1.0
        X.append(f)
    assert len(X) % 2 == 0
    return np.stack(X), pos


def _dft_matrix_ld(N):
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    jk = (np.arange(N)[:, None] * np.arange(N)[None, :]) % N
    ang = -(ld(2) * pi) * jk.astype(ld) / ld(N)
    return np.cos(ang) + 1j * np.sin(ang)           # clongdouble


def _rfft2_ld(X):
    """direct O(N^2)-per-output DFT in extended precision: (M, N, N) real -> (M, N, N/2+1)"""
    N = X.shape[-1]
    W = _dft_matrix_ld(N)
    return np.stack([(W @ x.astype(np.longdouble) @ W)[:, :N // 2 + 1] for x in X])


def _irfft2_ld(Xh):
    """the inverse of a Hermitian-consistent half spectrum, same way: (M, N, N/2+1) -> (M, N, N) longdouble"""
    N, NK = Xh.shape[-2], Xh.shape[-1]
    Wc = np.conj(_dft_matrix_ld(N))
    out = []
    jm = (-np.arange(N)) % N
    for xh in Xh:
        full = np.zeros((N, N), dtype=np.clongdouble)
        full[:, :NK] = xh
        for k in range(NK, N):
            full[:, k] = np.conj(xh[jm, N - k])
        out.append((Wc @ full @ Wc).real / (np.longdouble(N) * N))
    return np.stack(out)


def _hermitian_consistent(Xh):
    """columns k = 0 and k = N/2 of a half spectrum made exactly self-conjugate (conjugation and copies are exact), so that
    every real inverse transform is asked the same question"""
    Xh = Xh.copy()
    N = Xh.shape[-2]
    for k in (0, Xh.shape[-1] - 1):
        for j in range(N // 2 + 1, N):
            Xh[:, j, k] = np.conj(Xh[:, N - j, k])
        Xh[:, 0, k] = Xh[:, 0, k].real
        Xh[:, N // 2, k] = Xh[:, N // 2, k].real
    return Xh


@pytest.mark.parametrize('N', ALL)
def test_transforms_on_noise_and_impulses(N):
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd.tools.operators import Dev
    X, pos = _transform_fields(N)
    M = X.shape[0]
    ref = np.fft.rfftn(X, axes=(-2, -1))
    Xh_in = _hermitian_consistent(ref)
    back_ref = np.fft.irfftn(Xh_in, s=(N, N), axes=(-2, -1))
    # plan-only handles (qgx_rfft2 / qgx_irfft2) and a model's setters: the same kernels under two entry points
    fwd, inv = {}, {}
    fwd['plan'] = Dev.rfft2(torch.as_tensor(X).cuda()).cpu().numpy()
    inv['plan'] = Dev.irfft2(torch.as_tensor(Xh_in).cuda()).cpu().numpy()
    Dev.close()
    e = _engine(N, M // 2)
    e.set_q(X.reshape(M // 2, 2, N, N))
    fwd['model'] = e.get(L.F_QH).cpu().numpy().reshape(M, N, N // 2 + 1)
    e.set_qh(Xh_in.reshape(M // 2, 2, N, N // 2 + 1))
    inv['model'] = e.get(L.F_Q).cpu().numpy().reshape(M, N, N)
    e.close()
    worst = 0.0
    for how in ('plan', 'model'):
        for f in range(M):
            ef, ei = _rel(fwd[how][f], ref[f]), _rel(inv[how][f], back_ref[f])
            worst = max(worst, ef, ei)
            assert ef < F64_TOL and ei < F64_TOL, (how, f, ef, ei)
        for i, (y0, x0) in enumerate(pos):          # closed forms: a mis-placed output cannot hide in noise
            got = fwd[how][2 + i]
            exact = _impulse_spectrum(N, y0, x0)
            assert np.abs(got - exact).max() < F64_TOL, (how, (y0, x0), np.abs(got - exact).max())
    # ... and the inverse of each closed form is the impulse again, zero everywhere else
    imp = np.stack([_impulse_spectrum(N, y0, x0) for (y0, x0) in pos])
    back = Dev.irfft2(torch.as_tensor(_hermitian_consistent(imp)).cuda()).cpu().numpy()
    Dev.close()
    for i in range(imp.shape[0]):
        y0, x0 = pos[i]
        want = np.zeros((N, N))
        want[y0, x0] = 1.0
        assert np.abs(back[i] - want).max() < F64_TOL, ((y0, x0), np.abs(back[i] - want).max())
    line = f'\nGRID transforms N={N}: worst error vs numpy {worst:.2e}'
    if N <= 72:
        # the truth: a direct DFT in extended precision.  The GPU may be 4 x as far from it as numpy is (+ 1e-15 of the max)
        t_f, t_i = _rfft2_ld(X), _irfft2_ld(Xh_in)
        worst_g = worst_n = 0.0
        for how in ('plan', 'model'):
            for f in range(M):
                for got, npy, truth in ((fwd[how][f], ref[f], t_f[f]), (inv[how][f], back_ref[f], t_i[f])):
                    mx = float(np.abs(truth).max())
                    eg = float(np.abs(got - truth).max())
                    en = float(np.abs(npy - truth).max())
                    worst_g, worst_n = max(worst_g, eg / mx), max(worst_n, en / mx)
                    assert eg <= 4.0 * en + 1e-15 * mx, (how, f, eg / mx, en / mx)
        line += f'; against the extended-precision DFT: GPU {worst_g:.2e}, numpy {worst_n:.2e}'
    print(line)


# ------------------------------------------------------------------------------------------------ unparameterized steps
def _steps_against_oracle(N, B, nsteps, params, opts=None, members=None, every_step=True):
    """the body of tests/test_gpu_parity.py::test_unparameterized_steps_match_oracle for any size, member count and kernel
    options -> (engine, worst q / qh error in units of F64_TOL x steps)"""
    import pyqg_generative_amd._lib as L
    members = _members(B) if members is None else members
    rs = np.random.RandomState(100 + N)
    q0 = _eddy_like_q(rs, B, N)
    e = _engine(N, B, **params)
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    e.set_q(q0)
    refs = {}
    for b in members:
        m = qg_ref.QGModelRef(nx=N, **params)
        m.set_q(q0[b])
        refs[b] = m
    worst = 0.0
    for s in range(nsteps):
        e.step(1)
        for m in refs.values():
            m._step_forward()
        if not every_step and s not in (0, 1, 2, nsteps - 1):
            continue
        qh = e.get(L.F_QH).cpu().numpy()
        q = e.get(L.F_Q).cpu().numpy()
        for b, m in refs.items():
            eh, eq = _rel(qh[b], m.qh), _rel(q[b], m.q)
            worst = max(worst, eh / (s + 1), eq / (s + 1))
            assert eh < F64_TOL * (s + 1), (N, B, opts, s, b, eh)
            assert eq < F64_TOL * (s + 1), (N, B, opts, s, b, eq)
    # fields pyqg keeps from the last inversion + tendencies
    ph, u, v = (e.get(f).cpu().numpy() for f in (L.F_PH, L.F_U, L.F_V))
    dq = e.get(L.F_DQHDT).cpu().numpy()
    dqpp = e.get(L.F_DQHDT_PP).cpu().numpy()
    ke, cfl = e.status()
    for b, m in refs.items():
        assert _rel(ph[b], m.ph) < 1e-11 and _rel(u[b], m.u) < 1e-11 and _rel(v[b], m.v) < 1e-11, (N, B, opts, b)
        assert _rel(dq[b], m.dqhdt_p) < 1e-10 and _rel(dqpp[b], m.dqhdt_pp) < 1e-10, (N, B, opts, b)
        assert abs(ke[b] - m._calc_ke()) < 1e-11 * m._calc_ke(), (N, B, opts, b)
        assert abs(cfl[b] - m._calc_cfl()) < 1e-11, (N, B, opts, b)
    assert e.tc == nsteps
    return e, worst / F64_TOL, q0


def _step_params(N):
    # non-default physics (the jet configuration) at one small-generic, one lpb = 4 and one unfused size
    if N in (72, 108, 162):
        return dict(JET, dt=min(JET['dt'], dt_of(N)))
    return dict(dt=dt_of(N))


@pytest.mark.parametrize('N', ALL)
def test_unparameterized_steps_match_oracle_at_every_size(N):
    """Euler -> AB2 -> AB3 start-up and steady AB3 steps, filter, friction: q and qh after every step, ph, u, v, both
    tendencies, KE and CFL at the end.  B = 3 up to 128, 2 above; 8 steps"""
    B, nsteps = (3, 8) if N <= 128 else (2, 8)
    e, worst, _ = _steps_against_oracle(N, B, nsteps, _step_params(N))
    e.close()
    print(f'\nGRID steps N={N} B={B}: worst q / qh error {worst * F64_TOL:.2e} per step')


@pytest.mark.parametrize('N', [24, 72, 162, 512])
def test_many_steps_in_one_call_equal_single_steps(N):
    import pyqg_generative_amd._lib as L
    B, k = 2, 9
    q0 = _eddy_like_q(np.random.RandomState(5 + N), B, N)
    e1, e2 = _engine(N, B, dt=dt_of(N)), _engine(N, B, dt=dt_of(N))
    e1.set_q(q0)
    e2.set_q(q0)
    e1.step(k)
    for _ in range(k):
        e2.step(1)
    for f in (L.F_QH, L.F_Q, L.F_PH, L.F_U, L.F_DQHDT):
        assert torch.equal(e1.get(f), e2.get(f)), f       # deterministic: bit-identical
    assert e1.tc == e2.tc == k
    e1.close()
    e2.close()


# ------------------------------------------------------------------------------------------------ launch shapes, generic small kernel
# (B, options): the layer-split form (two workgroups per member while 2 B <= 256), one workgroup per member with 1024
# threads (up to 256 members, and always above 64 x 64) and with 512; each forced explicitly as well
def _shapes(N):
    auto257 = 512 if N <= 64 else 1024            # spectral_small.hip::small_threads
    return [(1, {}), (3, {}), (3, dict(lsplit=1)), (3, dict(lsplit=0)), (3, dict(lsplit=0, spec_threads=256)),
            (3, dict(lsplit=0, spec_threads=512)), (3, dict(lsplit=0, spec_threads=1024)),
            (128, {}), (129, {}), (129, dict(lsplit=0, spec_threads=1024)), (129, dict(lsplit=0, spec_threads=512)),
            (257, {}), (257, dict(lsplit=0, spec_threads=auto257)), (257, dict(lsplit=0, spec_threads=1536 - auto257))]


@pytest.mark.parametrize('N', [24, 72])
def test_every_launch_shape_of_the_generic_small_kernel(N):
    import pyqg_generative_amd._lib as L
    nsteps = 6
    out = {}
    worst = 0.0
    for i, (B, opts) in enumerate(_shapes(N)):
        e, w, q0 = _steps_against_oracle(N, B, nsteps, dict(dt=dt_of(N)), opts, every_step=False)
        worst = max(worst, w)
        # the setters and the inversion at this shape (k_q_to_qh_small<0>, k_qh_to_q_small<0>, k_invert_small<0>)
        e.set_q(q0)
        qh0 = np.fft.rfftn(q0, axes=(-2, -1))
        assert _rel(e.get(L.F_QH).cpu().numpy(), qh0) < F64_TOL, (B, opts)
        e.invert()
        ph, u = e.get(L.F_PH).cpu().numpy(), e.get(L.F_U).cpu().numpy()
        for b in _members(B):
            m = qg_ref.QGModelRef(nx=N, dt=dt_of(N))
            m.set_q(q0[b])
            m._invert()
            assert _rel(ph[b], m.ph) < F64_TOL and _rel(u[b], m.u) < F64_TOL, (B, opts, b)
        e.set_qh(qh0)
        assert _rel(e.get(L.F_Q).cpu().numpy(), q0) < F64_TOL, (B, opts)
        e.step(nsteps)
        out[i] = [e.get(f).clone() for f in (L.F_QH, L.F_Q, L.F_U, L.F_PH, L.F_DQHDT)]
        e.close()
    # what the dispatch takes by itself is what the same shape forced explicitly computes: bit for bit
    # (tests/test_gpu_many_members.py asserts the same at 64 x 64)
    shapes = _shapes(N)
    for a, b in ((1, 2), (8, 9), (11, 12)):
        assert shapes[a][0] == shapes[b][0]
        for x, y in zip(out[a], out[b]):
            assert torch.equal(x, y), (shapes[a], shapes[b])
    print(f'\nGRID launch shapes N={N}: worst q / qh error {worst * F64_TOL:.2e} per step over {len(shapes)} shapes')


# ------------------------------------------------------------------------------------------------ a forcing in the tendency
@pytest.mark.parametrize('demean', [False, True], ids=['raw', 'demean'])
@pytest.mark.parametrize('N', [36, 72, 108, 288, 162, 512])
def test_external_forcing_in_the_tendency_matches_oracle(N, demean):
    """has_S at sizes without a specialisation, weight != 1, with and without the de-meaning of parameterization.py:25 (the
    forcing has a mean, so it matters): 1e-11 as tests/test_gpu_parity.py::test_external_forcing_matches_oracle_q_parameterization"""
    import pyqg_generative_amd._lib as L
    B, nsteps, dt = 2, 4, dt_of(N)
    rs = np.random.RandomState(9 + N)
    q0 = _eddy_like_q(rs, B, N)
    amp = np.array([7e-12, 2e-13])[None, :, None, None]
    Ss = [rs.randn(B, 2, N, N) * amp + 0.5 * amp for _ in range(nsteps)]

    def param(it):
        def f(mm):
            S = next(it)
            return 0.5 * (S - S.mean(axis=(-2, -1), keepdims=True) if demean else S)
        return f
    e = _engine(N, B, dt=dt)
    e.set_q(q0)
    refs = []
    for b in range(B):
        m = qg_ref.QGModelRef(nx=N, dt=dt, parameterization=param(iter([s[b] for s in Ss])))
        m.set_q(q0[b])
        refs.append(m)
    worst = 0.0
    for s in range(nsteps):
        e.step(1, forcing=torch.as_tensor(Ss[s]).cuda(), weight=0.5, demean=demean)
        for m in refs:
            m._step_forward()
        qh = e.get(L.F_QH).cpu().numpy()
        for b, m in enumerate(refs):
            worst = max(worst, _rel(qh[b], m.qh))
            assert _rel(qh[b], m.qh) < 1e-11, (s, b)
    e.close()
    print(f'\nGRID forcing N={N} demean={demean}: worst qh error {worst:.2e}')


# ------------------------------------------------------------------------------------------------ diagnostics
def _diag_cases():
    cases = [(N, 2, True, {}) for N in ALL]
    cases += [(N, 2, False, {}) for N in (24, 72, 144, 192, 512)]
    for N in (24, 72):
        # 6 B <= 256 or not: both automatic choices of diag_wide, each forced the other way too, and one launch per transform
        cases += [(N, 50, True, {}), (N, 50, False, {}), (N, 2, True, dict(diag_wide=0)), (N, 50, True, dict(diag_wide=1)),
                  (N, 2, True, dict(diag_fused=0)), (N, 50, True, dict(diag_fused=0)), (N, 2, False, dict(diag_fused=0))]
    cases += [(512, 2, True, dict(large_fused=0)), (512, 2, False, dict(large_fused=0)), (512, 2, True, dict(large_fused=1))]
    return cases


def _diag_id(v):
    if isinstance(v, dict):
        return '-'.join(f'{k}{x}' for k, x in v.items()) or 'auto'
    if isinstance(v, bool):
        return 'forced' if v else 'free'
    return str(v)


@pytest.mark.parametrize('N,B,forced,opts', _diag_cases(), ids=_diag_id)
def test_sixteen_diagnostics_match_oracle(N, B, forced, opts):
    """as tests/test_gpu_diagnostics.py::test_large_grid_increment_with_a_forcing_matches_oracle: seven steps, increments at
    steps 2, 4, 6, every diagnostic at 1e-9 of its maximum; without a forcing the parameterization spectra do not exist"""
    import pyqg_generative_amd._lib as L
    dt, nsteps = dt_of(N), 7
    rs = np.random.RandomState(N + B)
    q0 = _eddy_like_q(rs, B, N)
    Ss = [rs.randn(B, 2, N, N) * np.array([7e-12, 2e-13])[None, :, None, None] for _ in range(nsteps)]
    e = _engine(N, B, dt=dt)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_q(q0)
    e.diag_config(2, 2)
    refs = {}
    for b in _members(B):
        kw = dict(parameterization=(lambda it: lambda mm: 0.5 * next(it))(iter([s[b] for s in Ss]))) if forced else {}
        r = qg_ref.QGModelRef(nx=N, dt=dt, tavestart=2 * dt, taveint=2 * dt, **kw)
        r.set_q(q0[b])
        refs[b] = r
    for s in range(nsteps):
        if forced:
            e.step(1, forcing=torch.as_tensor(Ss[s]).cuda(), weight=0.5, demean=False)
        else:
            e.step(1)
        for r in refs.values():
            r._step_forward()
    assert e.diag_count == refs[0].diag_count == 3
    worst = 0.0
    for name in L.DIAGS:
        if not forced and (name.startswith('paramspec') or name == 'ENSparamspec'):
            continue
        got = e.diag(name).cpu().numpy()
        for b, r in refs.items():
            ref = r.get_diagnostic(name)
            err = np.abs(got[b] - ref).max() / np.abs(ref).max()
            worst = max(worst, err)
            assert got[b].shape == ref.shape and err <= 1e-9, (name, b, err)
    e.close()
    print(f'\nGRID diagnostics N={N} B={B} forcing={forced} {opts}: worst error {worst:.2e} of the maximum')


# ------------------------------------------------------------------------------------------------ large-grid step options
@pytest.mark.parametrize('opt', ['large_fused', 'large_lazy_q', 'large_specialised'])
@pytest.mark.parametrize('N', [128, 144])
def test_large_step_options_match_oracle(N, opt):
    """each step option switched off where it does select another path: 128 is the smallest grid with compile-time-N
    kernels, 144 the smallest run-time-N grid with four lines per workgroup.  large_specialised = 0: the run-time-N
    kernels at a size that has a specialisation; large_lazy_q = 0: the eager unparameterized step; large_fused = 0: the
    unfused step at a size that normally fuses"""
    e, worst, _ = _steps_against_oracle(N, 2, 6, _step_params(N), {opt: 0})
    e.close()
    print(f'\nGRID large options N={N} {opt}=0: worst q / qh error {worst * F64_TOL:.2e} per step')


# ------------------------------------------------------------------------------------------------ 512 x 512
@pytest.mark.parametrize('opt', ['large_fused', 'large_lazy_q', 'large_specialised'])
@pytest.mark.parametrize('value', [0, 1])
def test_512_kernel_options_compute_the_same_state(opt, value):
    """lines_per_block(512) = 2: every 512 x 512 step is large_step_unfused whatever these say — which is what
    this holds the options to: the same state within 1e-12 x steps of the oracle, and of each other bit for bit"""
    import pyqg_generative_amd._lib as L
    e, worst, q0 = _steps_against_oracle(512, 2, 6, dict(dt=dt_of(512)), {opt: value})
    ref = _engine(512, 2, dt=dt_of(512))
    ref.set_q(q0)
    ref.step(6)
    assert torch.equal(ref.get(L.F_QH), e.get(L.F_QH))
    e.close()
    ref.close()
    print(f'\nGRID 512 {opt}={value}: worst q / qh error {worst * F64_TOL:.2e} per step')


# ------------------------------------------------------------------------------------------------ the generator's grid sizes
KINDS = ('gan', 'vae', 'gz', 'ols')
_GENS = {}


def _gpu_generator(kind):
    """one device generator per kind for the module (creation calibrates: tens of launches)"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    if kind not in _GENS:
        if kind == 'ols':
            d = golden('weights_gz.npz')
            _GENS[kind] = qa.Generator('ols', [weights.net_from_npz(d, 'net0_')], np.asarray(d['x_std'], np.float32),
                                       np.asarray(d['y_std'], np.float32))
        else:
            nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, f'weights_{kind}.npz'), kind)
            _GENS[kind] = qa.Generator(kind, nets, xs, ys)
    return _GENS[kind]


def _oracle_generator(kind):
    if kind == 'ols':
        from ols_restatement import OLSRef
        return OLSRef.from_fixture()
    return load_generator(kind)


def _lib_cnn_forward(gen, x, inet):
    """qgx_cnn_forward itself (Generator.cnn_forward raises ValueError for a refused size before it gets there)"""
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    B, _, N, _ = x.shape
    y = torch.empty((B, 2, N, N), dtype=torch.float32, device=x.device)
    check(lib.qgx_cnn_forward(gen._h, inet, _ptr(x), _ptr(y), B, N, _stream()))
    torch.cuda.synchronize()
    return y


def _lib_generator_forward(gen, q, z):
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    B, _, N, _ = q.shape
    S = torch.empty_like(q)
    check(lib.qgx_generator_forward(gen._h, _ptr(q), _ptr(z), _ptr(S), B, N, 1, _stream()))
    torch.cuda.synchronize()
    return S


def _noise(kind, rs, B, N):
    if kind == 'ols':
        return None
    return rs.randn(B, 2, N, N) if kind == 'gz' else rs.randn(B, 2, N, N).astype('float32')


def _oracle_model(kind, ora, N, params, q0b, xib):
    class _Rng:
        def randn(self, *shape):
            return xib.astype('float64').reshape(shape)
    m = qg_ref.QGModelRef(nx=N, **params)
    m.sampling_type = 'AR1'
    m.noise_sampler = samplers_ref.make_sampler('AR1', 1)
    m.q_parameterization = gen_ref.ParameterizationRef(ora, rng=_Rng())
    m.set_q(q0b)
    return m


def _refusal(err, N):
    """QGX_ERR_INVALID with a message naming N"""
    s = str(getattr(err, 'value', err))
    assert 'qgx error -1' in s and re.search(rf'N ?= ?{N}\b', s), s


ADMITTED = {}        # (kind, N, B) -> True / False, as found; test_the_admitted_generator_sizes_are_the_documented_ones reads it


@pytest.mark.parametrize('N', ALL)
@pytest.mark.parametrize('kind', KINDS)
def test_generator_grid_size_contract(kind, N):
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd._lib import QgxError
    gen, ora = _gpu_generator(kind), _oracle_generator(kind)
    n_in = 2 if kind in ('gz', 'ols') else 4
    params = dict(dt=dt_of(N))
    for B in (1, 2):
        rs = np.random.RandomState(4000 + 10 * N + B)
        x = rs.randn(B, n_in, N, N).astype('float32')
        xd = torch.as_tensor(x).cuda()
        q0 = _eddy_like_q(rs, B, N)
        xi = _noise(kind, rs, B, N)
        xid = torch.as_tensor(xi).cuda() if xi is not None else None
        try:
            y0 = _lib_cnn_forward(gen, xd, 0)
            admitted = True
        except QgxError as err:
            admitted = False
            first = err
        ADMITTED[(kind, N, B)] = admitted
        if admitted:
            # ---- run: every net float32-class against the float64 evaluation of the same float32 parameters
            worst_y = 0.0
            for inet, net in enumerate(ora.nets):
                y = (y0 if inet == 0 else _lib_cnn_forward(gen, xd, inet)).cpu().numpy()
                assert np.array_equal(y, gen.cnn_forward(xd, inet).cpu().numpy())       # the facade reaches the same kernels
                ref = gen_ref.cnn_forward(net, x, dtype='float64')
                err = np.abs(y - ref).max() / np.abs(ref).max()
                worst_y = max(worst_y, err)
                assert err < 2e-5, (kind, N, B, inet, err)
            # ---- one online step with external noise against the oracle
            e = _engine(N, B, **params)
            e.set_q(q0)
            e.step(1, generator=gen, sampling='AR1', nsteps_decor=1, z_external=xid)
            qh, S = e.get(L.F_QH).cpu().numpy(), e.get(L.F_S).cpu().numpy()
            worst_S = worst_q = 0.0
            for b in range(B):
                m = _oracle_model(kind, ora, N, params, q0[b], xi[b] if xi is not None else None)
                m._step_forward()
                sc = np.abs(m.PV_forcing).max(axis=(1, 2), keepdims=True)
                eS, eq = (np.abs(S[b] - m.PV_forcing) / sc).max(), _rel(qh[b], m.qh)
                worst_S, worst_q = max(worst_S, eS), max(worst_q, eq)
                s_bound, qh_bound = LOOSE if (kind, N, B) == ('gz', 128, 2) else TIGHT
                assert eS < s_bound, (kind, N, B, b, eS)
                assert eq < qh_bound, (kind, N, B, b, eq)
            assert gen.range_ok() is None
            e.close()
            print(f'\nGRID generator {kind} N={N} B={B}: admitted; net error {worst_y:.2e}, S {worst_S:.2e}, qh {worst_q:.2e}')
            continue
        # ---- refused: by all three entry points, with QGX_ERR_INVALID and a message naming N ...
        _refusal(first, N)
        for inet in range(1, len(ora.nets)):
            with pytest.raises(QgxError) as err:
                _lib_cnn_forward(gen, xd, inet)
            _refusal(err, N)
        with pytest.raises(QgxError) as err:
            _lib_generator_forward(gen, torch.as_tensor(q0).cuda(), xid)
        _refusal(err, N)
        with pytest.raises(ValueError, match=rf'N = {N}\b'):        # the facade says so before it allocates anything
            gen.cnn_forward(xd)
        with pytest.raises(ValueError, match=rf'N = {N}\b'):
            gen.forward(torch.as_tensor(q0).cuda(), xid)
        e = _engine(N, B, **params)
        e.set_q(q0)
        e.step(2)
        with pytest.raises(ValueError, match=rf'N = {N}\b'):
            e.step(1, generator=gen, sampling='AR1', nsteps_decor=1, seed=3)
        before = [e.tc] + [e.get(f).clone() for f in (L.F_QH, L.F_Z, L.F_Q, L.F_S)]
        gen.check_size = lambda *a, **k: None            # past the facade: qgx_step itself
        try:
            for kw in (dict(sampling='AR1', nsteps_decor=2, seed=3),                      # a Philox draw
                       dict(sampling='constant', nsteps_decor=3, seed=3),                 # the constant sampler's counter
                       dict(sampling='AR1', nsteps_decor=1, z_external=xid)):             # external noise
                if kw.get('z_external', 0) is None:
                    continue
                with pytest.raises(QgxError) as err:
                    e.step(1, generator=gen, **kw)
                _refusal(err, N)
        finally:
            del gen.check_size
        # ... and before anything was launched or changed: the model is bitwise where it was
        torch.cuda.synchronize()
        after = [e.tc] + [e.get(f).clone() for f in (L.F_QH, L.F_Z, L.F_Q, L.F_S)]
        assert before[0] == after[0] == 2
        for a, b in zip(before[1:], after[1:]):
            assert torch.equal(a, b)
        # a following unparameterized step matches the oracle
        e.step(1)
        qh = e.get(L.F_QH).cpu().numpy()
        for b in range(B):
            m = qg_ref.QGModelRef(nx=N, **params)
            m.set_q(q0[b])
            for _ in range(3):
                m._step_forward()
            assert _rel(qh[b], m.qh) < F64_TOL * 3, (kind, N, B, b)
        e.close()
        # the handle is not poisoned: a parameterized step of a fresh engine on an admitted grid works
        e = _engine(64, 2, dt=14400.)
        q64 = _eddy_like_q(rs, 2, 64)
        z64 = _noise(kind, rs, 2, 64)
        e.set_q(q64)
        e.step(1, generator=gen, sampling='AR1', nsteps_decor=1,
               z_external=torch.as_tensor(z64).cuda() if z64 is not None else None)
        qh = e.get(L.F_QH).cpu().numpy()
        m = _oracle_model(kind, ora, 64, dict(dt=14400.), q64[1], z64[1] if z64 is not None else None)
        m._step_forward()
        eq = _rel(qh[1], m.qh)
        print(f'\nBOUND generator {kind} after a refusal at N={N} B={B}: qh at 64 x 64 {eq:.2e}')
        assert eq < TIGHT[1], (kind, N, B, eq)           # measured <= 6.5e-8 over all kinds and refused sizes
        assert gen.range_ok() is None
        e.close()
    print(f'\nGRID generator {kind} N={N}: ' + ', '.join(f'B={B} ' + ('admitted' if ADMITTED[(kind, N, B)] else 'refused') for B in (1, 2)))


def test_the_size_query_follows_the_options_in_force():
    """qgx_generator_size_ok answers for the options in force, not from a list (no device call): with 16 input channels
    staged per pass (option "chunk") the 5x5 layer's patch fits at 192 and 256 as well; 384 stays refused (the last layer's
    patch), by the query and by the facade.  (Nothing is RUN at 192 or 256 here: those sizes are not the shipped options'.)"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    from pyqg_generative_amd._lib import lib
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    gen = qa.Generator('gan', nets, xs, ys)
    for B in (1, 2, 64):
        assert [N for N in ALL if lib.qgx_generator_size_ok(gen._h, -1, B, N) == 0] == [16, 32, 48, 64, 96, 128], B
    gen.set_option('chunk', 16)
    assert [N for N in ALL if lib.qgx_generator_size_ok(gen._h, -1, 1, N) == 0] == [16, 32, 48, 64, 96, 128, 192, 256]
    with pytest.raises(ValueError, match='N = 384'):
        gen.cnn_forward(torch.zeros((1, 4, 384, 384), dtype=torch.float32, device='cuda'))
    gen.close()


def test_the_admitted_generator_sizes_are_the_documented_ones():
    """what the contract test found (it runs before this one in file order; run alone, this probes by itself) is what
    include/qgx.h states next to qgx_generator_create and what the facade checks"""
    from pyqg_generative_amd._lib import QgxError
    found = set()
    for N in ALL:
        for kind in KINDS:
            for B in (1, 2):
                if (kind, N, B) not in ADMITTED:
                    gen = _gpu_generator(kind)
                    x = torch.zeros((B, 2 if kind in ('gz', 'ols') else 4, N, N), dtype=torch.float32, device='cuda')
                    try:
                        _lib_cnn_forward(gen, x, 0)
                        ADMITTED[(kind, N, B)] = True
                    except QgxError:
                        ADMITTED[(kind, N, B)] = False
        verdicts = {ADMITTED[(kind, N, B)] for kind in KINDS for B in (1, 2)}
        assert len(verdicts) == 1, (N, 'kinds or member counts disagree')
        if verdicts.pop():
            found.add(N)
    print(f'\nGRID generator sizes admitted: {sorted(found)}')
    assert sorted(found) == [16, 32, 48, 64, 96, 128]
    header = open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'qgx.h')).read()
    assert 'run N = ' + ', '.join(str(n) for n in sorted(found)[:-1]) + f' and {max(found)}' in header
