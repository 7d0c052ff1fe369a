"""Two sets of physical constants in which EVERY constant of qgx_config is off pyqg's default and the two layers differ
(U1 != U2, del1 != del2, Qy1 != Qy2), with the time step, the initial condition and the option tables that
tests/test_gpu_physics_constants.py and the oracle tests of tests/test_oracle_qg.py run them with.  A plain helper module
like tests/redzone.py: it imports numpy and the oracle only.

pyqg's default has U2 = 0, L = 1e6 and filterfac = 23.6, so kx U2 q, every factor 1e6 / L and the filter's exponent vanish
or coincide there.  H1 is passed off default too but CANNOT be pinned: only H_k / H enters the equations, so changing H1
alone moves qh, KE and every diagnostic by exactly 0."""
import numpy as np

A = dict(L=7.5e5, rd=20000., delta=0.4, beta=2.2e-11, U1=0.04, U2=0.015, rek=2e-7, H1=700., filterfac=17.0)
B = dict(L=2e6, rd=11000., delta=0.6, beta=0.0, U1=-0.01, U2=0.03, rek=9e-7, H1=300., filterfac=30.0)
SETS = dict(A=A, B=B)


def dt_of(N):
    """tests/test_gpu_grid_sizes.py::dt_of (the GPU module asserts that the two agree)"""
    return 14400. if N <= 64 else 7200. if N <= 128 else 3600. if N <= 384 else 1800.


def dt_half(N):
    """with dt_of(N) sets A and B stay finite but reach a CFL of 0.40 (A at 64 x 64); with half of it 0.14 / 0.10 after
    8 steps at 32 x 32"""
    return dt_of(N) / 2.


def params(name, N, **more):
    """keyword arguments of QGModelRef / EnsembleEngine for set `name` at N x N"""
    return dict(SETS[name], dt=dt_half(N), **more)


def eddy_like_q(rs, n_members, N, L):
    """the suite's _eddy_like_q — white noise x (8e-6, 1e-6), band-limited to 2/3 Nyquist, x 3 — with the band limit taken
    on the model's OWN grid (wavenumbers of an L x L domain)"""
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N, L=L)
    q = rs.randn(n_members, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    qh = np.fft.rfftn(q, axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    return np.fft.irfftn(qh, axes=(-2, -1)) * 3.0


def forcing(rs, n_members, N, nsteps):
    """external forcings with the amplitudes (and the mean) of test_external_forcing_in_the_tendency_matches_oracle"""
    amp = np.array([7e-12, 2e-13])[None, :, None, None]
    return [rs.randn(n_members, 2, N, N) * amp + 0.5 * amp for _ in range(nsteps)]


# ---- the case tables: (grid, members, set, options)
# unparameterized steps, 8 from a cold start (4 from 384 x 384 up)
STEP_CASES = [
    (32, 3, 'A', {}), (32, 129, 'A', {}),                                        # 129: one workgroup per member
    (48, 2, 'A', dict(lsplit=1)),
    (64, 3, 'A', dict(lsplit=0)), (64, 3, 'B', {}),
    (96, 3, 'B', {}),
    (24, 3, 'B', {}), (24, 3, 'B', dict(lsplit=0, spec_threads=512)),            # run-time N
    (72, 2, 'A', {}), (72, 2, 'A', dict(lsplit=0, spec_threads=512)),
    (128, 2, 'A', {}), (128, 2, 'A', dict(large_fused=0)),
    (108, 2, 'A', {}), (162, 2, 'A', {}), (192, 2, 'A', {}),                     # four lines per workgroup / two, unfused / 192's transforms
    (384, 2, 'A', {}), (512, 2, 'A', {}), (512, 2, 'A', dict(large_fused=0)),
]
# 256 x 256: step(8) in one call; team = 1 is the XCD-resident run kernel where the device has it
TEAM_CASES = [('A', 1), ('B', 0)]
# an external forcing in the tendency, 4 steps
FORCING_CASES = [(64, 4, 'A', o) for o in ({}, dict(siblings=0), dict(siblings=2), dict(split_adv=1), dict(streams=2))] + \
                [(N, 2, 'A', {}) for N in (36, 128, 288)]
# all sixteen diagnostics with that forcing: (grid, members, set, options, steps, cadence)
DIAG_CASES = [(64, 3, 'A', o, 8, 2) for o in ({}, dict(diag_wide=0), dict(diag_wide=0, diag_reg=3), dict(diag_wide=0, diag_reg=0),
                                              dict(diag_wide=1), dict(diag_fused=0))] + \
             [(32, 2, 'A', dict(diag_wide=0), 8, 2),                             # the smallest register kernel
              (24, 2, 'B', {}, 8, 2),                                            # run-time N
              (128, 2, 'A', {}, 8, 2), (128, 2, 'A', dict(large_fused=0), 8, 2),
              (192, 2, 'A', {}, 8, 2), (256, 2, 'B', {}, 8, 2),
              (512, 2, 'A', {}, 4, 1)]
# every path the diagnostics increment can take on a small grid (tests/test_gpu_parity.py::SMALL_DIAG_PATHS)
SMALL_DIAG_PATHS = ({}, dict(diag_fused=0), dict(diag_wide=1), dict(diag_wide=0), dict(diag_wide=0, diag_reg=0),
                    dict(diag_wide=0, diag_reg=2), dict(diag_wide=0, diag_reg=3))


def case_id(v):
    if isinstance(v, dict):
        return '-'.join(f'{k}{x}' for k, x in v.items()) or 'auto'
    return str(v)
