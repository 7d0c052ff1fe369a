"""GPU: molecular viscosity inside the step kernels (qgx_set_viscosity; the reference's Laplace(nu, PV) q-parameterization,
pyqg_generative/tools/simulate.py:207-236) against the CPU oracle driven by a test-local restatement of that closure.

nu is per member and member 0 has nu = 0, so every case carries its own "term off" control.  Tolerances are the ones the
spectral core is held to elsewhere (tests/test_gpu_parity.py, tests/test_gpu_diagnostics.py): qh, q to F64_TOL (s + 1);
ph, u, v to 1e-11; diagnostics to 1e-9 of max|ref|."""
import os
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from conftest import GOLDEN
from oracle import qg_ref

F64_TOL = 1e-12


class RoundTripLaplace:
    """the closure as the reference evaluates it: Laplacian in spectral space, result handed over in real space"""

    def __init__(self, nu, PV):
        self.nu, self.PV = nu, PV

    def __call__(self, m):
        lap = -(m.k ** 2 + m.l ** 2)
        field = m.qh if self.PV else lap * m.ph
        return self.nu * m.ifft(lap * field)


def _engine(N, B, **kw):
    import pyqg_generative_amd as qa
    return qa.EnsembleEngine(nx=N, n_members=B, **kw)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _eddy_like_q(rs, B, N):
    """smooth fields with eddy-like amplitudes (white noise band-limited to 2/3 Nyquist)"""
    m = qg_ref.QGModelRef(nx=N)
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    qh = np.fft.rfftn(q, axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    return np.fft.irfftn(qh, axes=(-2, -1)) * 3.0


def _oracles(N, q0, nu, PV, extra=None, **params):
    """one oracle per member with the round-trip closure of that member's nu (extra(b): a callable whose result is added)"""
    refs = []
    for b in range(len(nu)):
        lap = RoundTripLaplace(nu[b], PV)
        add = extra(b) if extra is not None else None
        param = lap if add is None else (lambda lap, add: lambda mm: lap(mm) + add(mm))(lap, add)
        m = qg_ref.QGModelRef(nx=N, parameterization=param, **params)
        m.set_q(q0[b])
        refs.append(m)
    return refs


def _dt(N):
    return 14400. if N <= 64 else (7200. if N <= 128 else 3600.)


# ---- 1. small grids: every form of k_step_small (generic N, compile-time N, radix-3, one or two workgroups per member)
SMALL = [(N, PV, ls, 23.6) for N in (24, 32, 48, 64) for PV in (False, True) for ls in (0, 1)] + [(64, False, 1, 1e20), (48, True, 0, 1e20)]


@pytest.mark.parametrize('N,PV,lsplit,filterfac', SMALL)
def test_small_grid_steps_match_oracle(N, PV, lsplit, filterfac):
    import pyqg_generative_amd._lib as L
    B, nsteps, nu = 3, 12, [0., 20., 50.]
    params = dict(dt=_dt(N), filterfac=filterfac)
    q0 = _eddy_like_q(np.random.RandomState(300 + N), B, N)
    e, e2 = _engine(N, B, **params), _engine(N, B, **params)
    for x in (e, e2):
        x.set_option('lsplit', lsplit)
        x.set_q(q0)
        x.set_viscosity(nu, PV=PV)
    refs = _oracles(N, q0, nu, PV, **params)
    for s in range(nsteps):
        e.step(1)
        for m in refs:
            m._step_forward()
        qh, q = e.get(L.F_QH).cpu().numpy(), e.get(L.F_Q).cpu().numpy()
        for b, m in enumerate(refs):
            assert _rel(qh[b], m.qh) < F64_TOL * (s + 1), (s, b, _rel(qh[b], m.qh))
            assert _rel(q[b], m.q) < F64_TOL * (s + 1), (s, b)
    ph, u, v = (e.get(f).cpu().numpy() for f in (L.F_PH, L.F_U, L.F_V))
    for b, m in enumerate(refs):
        assert _rel(ph[b], m.ph) < 1e-11 and _rel(u[b], m.u) < 1e-11 and _rel(v[b], m.v) < 1e-11
    # the term did something: the viscous members left the inviscid one (same initial condition would be needed for a
    # number; here: the oracle with the term removed is far outside the tolerance)
    plain = qg_ref.QGModelRef(nx=N, **params)
    plain.set_q(q0[2])
    for _ in range(nsteps):
        plain._step_forward()
    assert _rel(qh[2], plain.qh) > 1e-3
    e2.step(nsteps)                                   # one call of many steps: bit for bit the single steps
    assert torch.equal(e2.get(L.F_QH), e.get(L.F_QH)) and torch.equal(e2.get(L.F_Q), e.get(L.F_Q))
    assert e.tc == e2.tc == nsteps


# ---- 2. large grids: k_l_rows_fwd_tend (run-time N at 192, compile-time N at 128 / 256) and k_l_tendency (large_fused = 0)
@pytest.mark.parametrize('N,fused,PV', [(128, 1, False), (128, 1, True), (128, 0, False), (128, 0, True), (192, 1, False), (192, 1, True)])
def test_large_grid_steps_match_oracle(N, fused, PV):
    import pyqg_generative_amd._lib as L
    B, nsteps, nu = 2, 6, [0., 50.]
    params = dict(dt=_dt(N))
    q0 = _eddy_like_q(np.random.RandomState(400 + N), B, N)
    e = _engine(N, B, **params)
    e.set_option('large_fused', fused)
    e.set_q(q0)
    e.set_viscosity(nu, PV=PV)
    refs = _oracles(N, q0, nu, PV, **params)
    for s in range(nsteps):
        e.step(1)
        for m in refs:
            m._step_forward()
        qh, q = e.get(L.F_QH).cpu().numpy(), e.get(L.F_Q).cpu().numpy()
        for b, m in enumerate(refs):
            assert _rel(qh[b], m.qh) < F64_TOL * (s + 1), (s, b, _rel(qh[b], m.qh))
            assert _rel(q[b], m.q) < F64_TOL * (s + 1), (s, b)
    ph, u, v = (e.get(f).cpu().numpy() for f in (L.F_PH, L.F_U, L.F_V))
    for b, m in enumerate(refs):
        assert _rel(ph[b], m.ph) < 1e-11 and _rel(u[b], m.u) < 1e-11 and _rel(v[b], m.v) < 1e-11


@pytest.mark.parametrize('PV', [False, True])
def test_256_run_of_steps_matches_oracle_and_takes_three_launches_per_step(PV):
    """One call of six steps that refresh nothing: on an inviscid model the single-launch run kernel's case.  A model with
    viscosity steps on the three-launch path (the run kernel's viscous instance spilled), so the run
    kernel is never probed — qgx_run_kernel_state stays 0 — and option team changes nothing."""
    import pyqg_generative_amd._lib as L
    N, B, nsteps, nu = 256, 2, 6, [0., 50.]
    params = dict(dt=_dt(N))
    q0 = _eddy_like_q(np.random.RandomState(656), B, N)
    outs = []
    for team in (1, 0):
        e = _engine(N, B, **params)
        e.set_option('team', team)
        e.set_q(q0)
        e.set_viscosity(nu, PV=PV)
        e.step(nsteps, refresh_diag=False)
        assert e.tc == nsteps and e.run_kernel_state == 0
        outs.append((e.get(L.F_QH), e.get(L.F_Q)))
        if team:          # switching the term off hands the model back to the run kernel, where the device has one
            e.set_viscosity(None)
            e.step(2, refresh_diag=False)
            assert e.run_kernel_state != 0
        e.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    refs = _oracles(N, q0, nu, PV, **params)
    qh, q = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    for b, m in enumerate(refs):
        for _ in range(nsteps):
            m._step_forward()
        assert _rel(qh[b], m.qh) < F64_TOL * nsteps, (b, _rel(qh[b], m.qh))
        assert _rel(q[b], m.q) < F64_TOL * nsteps, b


# ---- 3. diagnostics: the viscous dqh is the parameterization's tendency
DIAG_CASES = [(64, {}, False), (64, dict(diag_wide=0), False), (64, dict(diag_wide=0), True), (64, dict(diag_wide=0, diag_reg=3), False),
              (64, dict(diag_wide=0, diag_reg=0), False), (64, dict(diag_fused=0), True), (128, {}, False), (128, {}, True),
              (128, dict(large_fused=0), False)]


@pytest.mark.parametrize('N,opts,PV', DIAG_CASES, ids=lambda v: '-'.join(f'{k}{x}' for k, x in v.items()) or 'default' if isinstance(v, dict) else str(v))
def test_all_sixteen_diagnostics_match_oracle(N, opts, PV):
    """64 x 64: the (member, transform) increment with k_diag_accumulate (default at three members), the register increment
    k_diag_small_reg as one and as two workgroups per member, k_diag_small, the composed increment; 128 x 128: the
    three-launch increment (k_l_rows_diag_acc) and the composed one"""
    import pyqg_generative_amd._lib as L
    B, nsteps, nu = 3, 8, [0., 20., 50.]
    dt = _dt(N)
    q0 = _eddy_like_q(np.random.RandomState(500 + N), B, N)
    e = _engine(N, B, dt=dt)
    for k, x in opts.items():
        e.set_option(k, x)
    e.set_q(q0)
    e.set_viscosity(nu, PV=PV)
    e.diag_config(2, 2)
    refs = _oracles(N, q0, nu, PV, dt=dt, tavestart=2 * dt, taveint=2 * dt)
    e.step(nsteps)
    for m in refs:
        for _ in range(nsteps):
            m._step_forward()
    assert e.diag_count == refs[0].diag_count == 3
    got = {name: e.diag(name).cpu().numpy() for name in L.DIAGS}
    assert len(got) == 16
    for name in L.DIAGS:
        for b, m in enumerate(refs):
            ref = m.get_diagnostic(name)
            assert got[name][b].shape == ref.shape, name
            assert np.abs(got[name][b] - ref).max() <= 1e-9 * np.abs(ref).max(), (name, b, np.abs(got[name][b] - ref).max() / np.abs(ref).max())
    for b in (1, 2):
        total = got['paramspec'][b]
        assert np.abs(total).max() > 0
        assert np.abs(got['paramspec_APEflux'][b] + got['paramspec_KEflux'][b] - total).max() <= 1e-10 * np.abs(total).max()
    assert not got['paramspec'][0].any() and not got['ENSparamspec'][0].any()       # nu = 0: a tendency of zeros
    qh = e.get(L.F_QH).cpu().numpy()
    for b, m in enumerate(refs):
        assert _rel(qh[b], m.qh) < F64_TOL * nsteps


# ---- 4. composition with the forcings qgx_step already takes
@pytest.mark.parametrize('PV', [False, True])
def test_viscosity_with_an_external_forcing(PV):
    """forcing_dev with weight 0.5: the viscous term is added to the tendency, not to S — weight does not touch it"""
    import pyqg_generative_amd._lib as L
    N, B, nsteps, nu = 64, 3, 5, [0., 20., 50.]
    rs = np.random.RandomState(9)
    q0 = _eddy_like_q(rs, B, N)
    Ss = [rs.randn(B, 2, N, N) * np.array([7e-12, 2e-13])[None, :, None, None] for _ in range(nsteps)]
    e = _engine(N, B, dt=14400.)
    e.set_q(q0)
    e.set_viscosity(nu, PV=PV)
    e.diag_config(1, 2)
    refs = _oracles(N, q0, nu, PV, extra=lambda b: (lambda it: lambda mm: 0.5 * next(it))(iter([s[b] for s in Ss])), dt=14400.,
                    tavestart=14400., taveint=2 * 14400.)
    for s in range(nsteps):
        e.step(1, forcing=torch.as_tensor(Ss[s]).cuda(), weight=0.5, demean=False)
        for m in refs:
            m._step_forward()
        qh = e.get(L.F_QH).cpu().numpy()
        for b, m in enumerate(refs):
            assert _rel(qh[b], m.qh) < F64_TOL * (s + 1), (s, b, _rel(qh[b], m.qh))
    assert e.diag_count == refs[0].diag_count == 2
    for name in ('paramspec', 'ENSparamspec', 'Dissspec'):      # weight * S^ + the viscous term, each part present
        got = e.diag(name).cpu().numpy()
        for b, m in enumerate(refs):
            ref = m.get_diagnostic(name)
            assert np.abs(got[b] - ref).max() <= 1e-9 * np.abs(ref).max(), (name, b)


def _gan():
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    return qa.Generator('gan', nets, xs, ys)


def test_viscosity_with_the_gan_generator():
    """48 x 48, two members, external white noise: against the oracle fed the forcing qgx_generator_forward gives for the
    same PV and noise, plus the closure; then bit for bit with the generator's kernels folded into the step kernel or not,
    and as two half-ensembles on two streams (each half must see its own slice of nu)"""
    import pyqg_generative_amd._lib as L
    N, B, nsteps, nu = 48, 2, 3, [20., 50.]
    rs = np.random.RandomState(48)
    q0 = _eddy_like_q(rs, B, N)
    xis = [torch.as_tensor(rs.randn(B, 2, N, N).astype('float32')).cuda() for _ in range(nsteps)]
    gen = _gan()
    expected = {}
    refs = _oracles(N, q0, nu, False, extra=lambda b: (lambda mm: expected['S'][b]), dt=14400.)
    res = []
    for genfuse in (1, 0):
        e = _engine(N, B, dt=14400.)
        e.set_option('genfuse', genfuse)
        e.set_q(q0)
        e.set_viscosity(nu)
        for s in range(nsteps):
            if genfuse:
                expected['S'] = gen.forward(e.get(L.F_Q), xis[s], demean=True).cpu().numpy()
            e.step(1, generator=gen, sampling='constant', nsteps_decor=1, z_external=xis[s])
            if genfuse:
                qh = e.get(L.F_QH).cpu().numpy()
                for b, m in enumerate(refs):
                    m._step_forward()
                    assert _rel(qh[b], m.qh) < F64_TOL * (s + 1), (s, b, _rel(qh[b], m.qh))
        res.append([e.get(f).clone() for f in (L.F_QH, L.F_Q, L.F_S)])
        e.close()
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # on-device noise (an external draw is never stepped in halves); the exact-f32 generator kernels, whose results do not
    # depend on the number of members in a launch (a half is one member here)
    gen.set_option('precision', 0)
    res = []
    for streams in (1, 2):
        e = _engine(N, B, dt=14400.)
        e.set_option('streams', streams)
        e.set_q(q0)
        e.set_viscosity(nu)
        assert e.step_streams(gen) == streams
        e.step(nsteps, generator=gen, sampling='AR1', nsteps_decor=1, seed=3)
        res.append([e.get(f).clone() for f in (L.F_QH, L.F_Q, L.F_S)])
        e.close()
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # and a half that read the other half's nu would not have gone unnoticed
    e = _engine(N, B, dt=14400.)
    e.set_q(q0)
    e.set_viscosity(nu[::-1])
    e.step(nsteps, generator=gen, sampling='AR1', nsteps_decor=1, seed=3)
    assert not torch.equal(e.get(L.F_QH), res[0][0])


# ---- 5. off means off
def test_off_is_bitwise_off():
    import pyqg_generative_amd._lib as L
    N, B, nsteps = 64, 3, 12
    q0 = _eddy_like_q(np.random.RandomState(5), B, N)
    never, off, zero = _engine(N, B, dt=14400.), _engine(N, B, dt=14400.), _engine(N, B, dt=14400.)
    for e in (never, off, zero):
        e.set_q(q0)
    assert never.viscosity is None
    off.set_viscosity([0., 20., 50.], PV=True)
    off.set_viscosity(None)
    assert off.viscosity is None
    zero.set_viscosity(0.)
    nu0, pv0 = zero.viscosity
    assert not nu0.any() and nu0.shape == (B,) and pv0 is False        # "on, zero" is not "off"
    for e in (never, off, zero):
        e.step(nsteps)
    a, b, c = (e.get(L.F_QH) for e in (never, off, zero))
    assert torch.equal(a, b)
    # adding a product that is +-0 can only turn a -0 into a +0: equal as numbers
    assert bool((torch.view_as_real(a) == torch.view_as_real(c)).all())
    # between steps: the term takes effect at the next step and the AB history is kept
    never.set_viscosity([0., 20., 50.])
    never.step(3)
    r = qg_ref.QGModelRef(nx=N, dt=14400.)
    r.set_q(q0[2])
    for _ in range(nsteps):
        r._step_forward()
    r.q_parameterization = RoundTripLaplace(50., False)
    for _ in range(3):
        r._step_forward()
    assert never.tc == nsteps + 3
    assert _rel(never.get(L.F_QH).cpu().numpy()[2], r.qh) < F64_TOL * (nsteps + 3)


# ---- 6. the facade and the run script
def test_qgmodel_runs_a_laplace_fused_and_equals_the_host_plug_in():
    from pyqg_generative_amd.qgmodel import QGModel
    from pyqg_generative_amd.models import Laplace
    N, B, nsteps, dt = 64, 2, 12, 14400.
    q0 = _eddy_like_q(np.random.RandomState(6), B, N)
    kw = dict(nx=N, dt=dt, tmax=dt * nsteps, twrite=10000, tavestart=dt * 2, taveint=dt * 2, log_level=0, n_members=B)
    out = {}
    for fused in (True, False):
        m = QGModel(parameterization=0.5 * Laplace([0., 100.], PV=False, fused=fused), **kw)
        m.q = q0
        m.run()
        assert m.tc == nsteps
        out[fused] = (m.qh, m.get_diagnostic('paramspec'), m._eng.step_calls, m._eng.viscosity)
        m.close()
    assert _rel(out[True][0], out[False][0]) < 1e-11
    assert np.abs(out[True][1] - out[False][1]).max() <= 1e-9 * np.abs(out[False][1]).max()
    # the fused run steps as an unparameterized model: one multi-step call, viscosity set once; the plug-in one call per step
    assert out[True][2] == 1 and out[False][2] == nsteps
    nu, pv = out[True][3]
    np.testing.assert_array_equal(nu, [0., 50.])
    assert pv is False and out[False][3] is None
    refs = _oracles(N, q0, [0., 50.], False, dt=dt)
    for b, r in enumerate(refs):
        for _ in range(nsteps):
            r._step_forward()
        assert _rel(out[True][0][b], r.qh) < F64_TOL * nsteps


def test_run_molecular_viscosity_returns_the_dataset_of_a_sweep():
    from pyqg_generative_amd.tools.simulate import run_molecular_viscosity, run_simulation
    from pyqg_generative_amd.models import Laplace
    dt = 14400.
    given = dict(nx=32, dt=dt, tmax=8 * dt, tavestart=2 * dt, taveint=2 * dt, twrite=10000, log_level=0, nu=[0., 50.])
    ds = run_molecular_viscosity(given, sampling_freq=4 * dt, n_members=2, seeds=[0, 1])
    assert given['nu'] == [0., 50.] and 'parameterization' not in given          # the caller's dictionary is left alone
    assert ds['q'].shape == (2, 2, 2, 32, 32)                                     # (run, time, lev, y, x): two snapshots
    spec = np.asarray(ds['paramspec'].values)
    assert spec.shape == (2, 32, 17) and not spec[0].any() and np.abs(spec[1]).max() > 0
    want = {k: v for k, v in given.items() if k != 'nu'}
    want.update(parameterization=Laplace([0., 50.], False), filterfac=1e+20)
    assert ds.attrs['pyqg_params'] == str(want)                                   # the reference's attribute: the run's own parameters
    # the reference's spelling: the Laplace under pyqg_params['parameterization']
    ds2 = run_simulation(want, sampling_freq=4 * dt, n_members=2, seeds=[0, 1])
    np.testing.assert_array_equal(np.asarray(ds2['q'].values), np.asarray(ds['q'].values))
    np.testing.assert_array_equal(np.asarray(ds2['paramspec'].values), spec)


# ---- 7. refusals
def test_refusals_leave_the_setting_in_force():
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd._lib import QgxError
    N, B = 32, 3
    q0 = _eddy_like_q(np.random.RandomState(7), B, N)
    e, good = _engine(N, B, dt=14400.), _engine(N, B, dt=14400.)
    for x in (e, good):
        x.set_q(q0)
        x.set_viscosity([1., 20., 50.], PV=True)
    for bad in ([1., -2., 3.], [1., float('nan'), 3.], [float('inf'), 0., 0.], -1.0):
        with pytest.raises(QgxError):
            e.set_viscosity(bad)
    for bad in ([1., 2.], [1., 2., 3., 4.], [[1., 2., 3.]]):
        with pytest.raises(ValueError):
            e.set_viscosity(bad)
    nu, pv = e.viscosity
    np.testing.assert_array_equal(nu, [1., 20., 50.])
    assert pv is True
    e.step(4)
    good.step(4)
    assert torch.equal(e.get(L.F_QH), good.get(L.F_QH))
    plan = _engine(N, 1, plan_only=True)
    with pytest.raises(QgxError, match='plan'):
        plan.set_viscosity(5.)
