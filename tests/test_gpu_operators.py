"""GPU parity of the coarse-graining / re-gridding / subgrid-forcing operators (config 5's second
half) against the oracle restatement (itself pinned by tests/golden/operators.npz) and against the
golden vectors directly.  float64: 1e-12 of the field maximum."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from conftest import golden
from oracle import operators_ref as ref, qg_ref

TOL = 1e-12


def _close(a, b, tol=TOL):
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), np.abs(a - b).max() / np.abs(b).max()


def test_regridding_matches_reference_golden():
    from pyqg_generative_amd.tools import operators as op
    g = golden('operators.npz')
    X = g['X']
    _close(op.cut_off(X, 32), g['cut_off_32'])
    _close(op.cut_off(X, 48), g['cut_off_48'])
    _close(op.clean_2h(X), g['clean_2h'])
    _close(op.fft_interpolate(X, 64, 96), g['interp_64_96'])
    _close(op.fft_interpolate(X, 64, 32), g['interp_64_32'])
    _close(op.fft_interpolate(X, 64, 96, truncate_2h=False), g['interp_64_96_keep2h'])
    _close(op.Operator5(X, 32), g['op5_32'])
    _close(op.cut_off(X[0], 32), g['cut_off_32'][0])          # 2-D input form
    with pytest.raises(ValueError):
        op.cut_off(X, 31)
    with pytest.raises(ValueError):
        op.fft_interpolate(X, 32, 64)


@pytest.mark.parametrize('N,nc', [(64, 32), (128, 48), (256, 64), (256, 96),
                                  (72, 24), (144, 48), (216, 72), (512, 64)])     # ... and grids without specialised kernels
def test_operators_match_oracle(N, nc):
    from pyqg_generative_amd.tools import operators as op
    rs = np.random.RandomState(N + nc)
    X = rs.randn(2, N, N)
    for name in ('Operator1', 'Operator2', 'Operator4', 'Operator5'):
        _close(getattr(op, name)(X, nc), getattr(ref, name)(X, nc))
    _close(op.gauss_filter(X, nc), ref.gauss_filter(X, nc))
    _close(op.model_filter(X), ref.model_filter(X))
    Y = rs.randn(2, N, N)
    _close(op.divergence(X, Y), ref.divergence(X, Y), 1e-11)


def test_advect_and_subgrid_forcing_match_oracle():
    from pyqg_generative_amd.tools import operators as op
    rs = np.random.RandomState(5)
    N = 128
    m = qg_ref.QGModelRef(nx=N)
    qh = m.fft(rs.randn(2, N, N) * np.array([8e-6, 1e-6])[:, None, None]) * (m.wv < 0.95 * m.kk[-1])
    m.set_qh(qh)
    m._invert()
    for rule in ('none', '3/2-rule', '2/3-rule'):
        _close(op.advect(m.q, m.u, m.v, rule), ref.advect(m.q, m.u, m.v, rule), 1e-11)
    params = {}
    # subgrid fluxes (operators.py:269-281)
    uq, vq = op.PV_subgrid_flux(m.q, 64, op.Operator2, params)
    mm0 = ref.apply_operator_to_model(m.q, 1, ref.identity_operator, params)
    mf0 = ref.apply_operator_to_model(m.q, 64, ref.Operator2, params)
    _close(uq, mf0.u * mf0.q - ref.Operator2(mm0.u * mm0.q, 64), 1e-10)
    _close(vq, mf0.v * mf0.q - ref.Operator2(mm0.v * mm0.q, 64), 1e-10)
    for oper, roper in ((op.Operator2, ref.Operator2), (op.Operator5, ref.Operator5), (op.Operator1, ref.Operator1)):
        f, mf, mm = op.PV_subgrid_forcing(m.q, 64, oper, params, '3/2-rule')
        fr, mfr, mmr = ref.PV_subgrid_forcing(m.q, 64, roper, params, '3/2-rule')
        _close(f, fr, 1e-10)
        _close(mf.q, mfr.q)
        _close(mf.u, mfr.u, 1e-11)
        mf.close()
        mm.close()
    # notebook identity (3-2-dealiasing.ipynb cells 48-51) on the device path
    SGS, mf, mm = op.PV_subgrid_forcing(m.q, 64, op.Operator5, params, '3/2-rule')
    advf = -op.advect(mf.q, mf.u, mf.v, '3/2-rule')
    adv = -op.cut_off(op.advect(m.q, m.u, m.v, '3/2-rule'), 64)
    assert np.linalg.norm(adv - (SGS + advf)) / np.linalg.norm(adv) < 1e-13


def test_batched_device_pipeline_config5_shapes():
    """hires 256^2 members -> 64^2 forcing with Operator2 and Operator5, 3/2-rule, all on device."""
    from pyqg_generative_amd.tools.operators import Dev
    rs = np.random.RandomState(1)
    B, N, nc = 3, 256, 64
    m = qg_ref.QGModelRef(nx=N)
    q = np.stack([m.ifft(m.fft(rs.randn(2, N, N) * 1e-6) * (m.wv < 0.9 * m.kk[-1])) for _ in range(B)])
    qd = torch.as_tensor(q).cuda()
    for dev_op, roper in ((Dev.Operator2, ref.Operator2), (Dev.Operator5, ref.Operator5)):
        forcing, qf, uf, vf = Dev.PV_subgrid_forcing(qd, nc, dev_op, {}, '3/2-rule')
        assert forcing.shape == (B, 2, nc, nc)
        for b in (0, B - 1):
            fr, mfr, _ = ref.PV_subgrid_forcing(q[b], nc, roper, {}, '3/2-rule')
            _close(forcing[b].cpu().numpy(), fr, 1e-10)
            _close(qf[b].cpu().numpy(), mfr.q)


def test_generate_subgrid_forcing_driver():
    """reference simulate.py:62-106 at reduced size: hires 128^2 x 2 members -> {32,48}^2 datasets."""
    from pyqg_generative_amd.tools.simulate import generate_subgrid_forcing
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    params = EDDY_PARAMS.nx(128)._update({'tmax': 7200. * 20, 'log_level': 0})
    out = generate_subgrid_forcing([32, 48], dict(params), sampling_freq=7200. * 10, n_members=2, seeds=[0, 1])
    assert sorted(out) == ['Operator2-32-dealias', 'Operator2-48-dealias', 'Operator5-32-dealias', 'Operator5-48-dealias']
    ds = out['Operator5-48-dealias']
    f = np.asarray(ds['q_forcing_advection'].values)
    assert f.shape == (2, 2, 2, 48, 48) and f.dtype == np.float32 and np.isfinite(f).all()
    # cross-check the last snapshot of member 1 against the oracle applied to the stored coarse PV's parent:
    # rerun the hires oracle with the same seed
    m = qg_ref.QGModelRef(nx=128, dt=7200., tmax=7200. * 20)
    qg_ref.set_initial_condition(m, np.random.RandomState(1))
    m.run()
    fr, mfr, _ = ref.PV_subgrid_forcing(m.q, 48, ref.Operator5, {}, '3/2-rule')
    q_c = np.asarray(ds['q'].values)[-1, 1]
    assert np.abs(q_c - mfr.q).max() < 1e-5 * np.abs(mfr.q).max()          # float32 storage
    assert np.abs(f[-1, 1] - fr).max() < 1e-4 * np.abs(fr).max()


@pytest.mark.parametrize('N,nc', [(64, 32), (256, 64), (144, 48)])
def test_spectral_subgrid_forcing_equals_the_composed_operators(N, nc):
    """Dev.PV_subgrid_forcing keeps the high-resolution tendency in spectral space and shares it between operators;
    composed=True runs the reference's sequence of grid-space operators.  Same operations: rounding-level agreement."""
    from pyqg_generative_amd.tools.operators import Dev
    rs = np.random.RandomState(3)
    B = 2
    m = qg_ref.QGModelRef(nx=N)
    q = np.stack([m.ifft(m.fft(rs.randn(2, N, N) * 1e-6) * (m.wv < 0.9 * m.kk[-1])) for _ in range(B)])
    qd = torch.as_tensor(q).cuda()
    ops = (Dev.Operator1, Dev.Operator2, Dev.Operator4, Dev.Operator5)
    for rule in ('none', '3/2-rule', '2/3-rule'):
        multi = Dev.PV_subgrid_forcing_multi(qd, nc, ops, {}, rule, return_psi=True)
        for dev_op, fast in zip(ops, multi):
            slow = Dev.PV_subgrid_forcing(qd, nc, dev_op, {}, rule, return_psi=True, composed=True)
            one = Dev.PV_subgrid_forcing(qd, nc, dev_op, {}, rule, return_psi=True)
            for a, b, c in zip(fast, slow, one):
                _close(a.cpu().numpy(), b.cpu().numpy(), 1e-11)
                assert torch.equal(a, c)
    # an operator without a spectral form takes the composed path
    ident = lambda X, n: X
    assert Dev.PV_subgrid_forcing_multi(qd, N, [ident], {}, 'none') is None
    f = Dev.PV_subgrid_forcing(qd, N, ident, {}, 'none')[0]
    assert np.abs(f.cpu().numpy()).max() < 1e-20
    Dev.close()


def test_plan_cache_holds_the_working_set_of_the_references_forcing_dataset_run(monkeypatch):
    """run_forcing_datasets.py sweeps Nc = [32, 48, 64, 96, 128] x (Operator2, Operator5) with the 3/2-rule at every
    snapshot: 15 plans / inversion models are live and the access is cyclic, so a cache smaller than that misses on
    EVERY lookup and rebuilds engines (about 25 hipMallocs + a device-synchronising hipFree each) twice per snapshot.
    After the first snapshot no engine may be created.  Transform plans are state-less handles (plan_only)."""
    from pyqg_generative_amd.tools import operators as op
    from pyqg_generative_amd import _lib
    Dev = op.Dev
    Dev.close()
    created = []
    real = op.EnsembleEngine

    def counting(*a, **kw):
        created.append((kw.get('nx'), kw.get('n_members'), bool(kw.get('plan_only'))))
        return real(*a, **kw)
    monkeypatch.setattr(op, 'EnsembleEngine', counting)
    B, N = 2, 256
    pp = {}
    rs = np.random.RandomState(4)
    for snap in range(3):
        q = torch.as_tensor(rs.randn(B, 2, N, N) * 1e-6, device='cuda')
        before = len(created)
        hat = Dev.hires_tendency_hat(q, pp, '3/2-rule')
        for o in (Dev.Operator2, Dev.Operator5):
            for nc in (32, 48, 64, 96, 128):
                Dev.subgrid_forcing_from_hat(hat[0], hat[1], nc, o, pp, '3/2-rule')
        if snap == 0:
            assert 10 <= len(created) <= Dev.MAX_PLANS
        else:
            assert len(created) == before, created[before:]
    assert any(p for _, _, p in created) and any(not p for _, _, p in created)
    # a plan-only handle transforms, and refuses everything that needs model state
    plan = Dev.plan(64, 4)
    x = torch.as_tensor(rs.randn(4, 64, 64), device='cuda')
    _close(Dev.rfft2(x).cpu().numpy(), np.fft.rfftn(x.cpu().numpy(), axes=(-2, -1)))
    with pytest.raises(_lib.QgxError, match='FFT plan only'):
        plan.step(1)
    with pytest.raises(_lib.QgxError, match='FFT plan only'):
        plan.get(_lib.F_Q)
    Dev.close()
