"""GPU: sampling='deterministic' on the device, for whole ensembles — qgx_generator_forward_mean and the step mode
QGX_SAMPLING_DETERMINISTIC against the CPU oracle's predict_mean_snapshot on the same Philox realisations
(parameterization.py:27-28, cgan_regression.py:164-171, cvae_regression.py:138-145, mean_var_model.py:111-115).

Tolerances are the project's: 2e-5 of the per-layer max|S_ref| for a forcing (test_gpu_parity.py, golden generator tests),
2e-6 relative for qh after a few steps (test_randomised_configurations_match_oracle).  On these fixtures the mean of M = 5
realisations keeps 0.90 ... 0.99 of one sample's magnitude and the float32-vs-float64 summation order moves it by 1e-7, so
the forcing bound is neither vacuous nor tight by construction."""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from conftest import golden, load_generator, GOLDEN
from oracle import qg_ref, gen_ref, samplers_ref

S_TOL, QH_TOL = 2e-5, 2e-6


def _gpu_generator(kind):
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    reg = kind.endswith('+reg')
    kind = kind[:-4] if reg else kind
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, f'weights_{kind}.npz'), kind,
                                    regression_npz=os.path.join(GOLDEN, 'weights_gz.npz') if reg else None)
    return qa.Generator(kind, nets, xs, ys)


def _eddy_like_q(rs, B, N):
    m = qg_ref.QGModelRef(nx=N)
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    qh = np.fft.rfftn(q, axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    return np.fft.irfftn(qh, axes=(-2, -1)) * 3.0


def _realisations(seed, member, t, M, N):
    """the M latent fields of one member at key-step t: realisation j on the Philox stream (seed, member, t | (j+1) << 32)"""
    return np.stack([samplers_ref.philox_normal(seed, member, t | (j + 1) << 32, 2 * N * N)[0].reshape(2, N, N)
                     for j in range(M)])


def _oracle_mean(ora, q, M, seed, member_offset, t):
    """-> (raw, de-meaned) forcing of predict_mean_snapshot for every member of q (B,2,N,N), float64"""
    N = q.shape[-1]
    raw = np.stack([ora.predict_mean_snapshot(q[b], M, z=_realisations(seed, member_offset + b, t, M, N))
                    for b in range(q.shape[0])])
    return raw, np.stack([gen_ref.demean(r) for r in raw])


def _s_err(S, ref, scale_of=None):
    sc = np.abs(ref if scale_of is None else scale_of).max(axis=(-2, -1), keepdims=True)
    return (np.abs(S - ref) / sc).max()


_CASES = {}


def _case(kind):
    """inputs and the oracle's answer for one generator kind, computed once and shared (never modified)"""
    if kind not in _CASES:
        reg = kind.endswith('+reg')
        N, B, M = (48, 2, 4) if reg else (48, 3, 5)
        seed, off, t = 31, 7, 3
        q = _eddy_like_q(np.random.RandomState(17), B, N)
        raw, dem = _oracle_mean(load_generator(kind), q, M, seed, off, t)
        for a in (q, raw, dem):
            a.setflags(write=False)
        _CASES[kind] = dict(N=N, B=B, M=M, seed=seed, off=off, t=t, q=q, raw=raw, dem=dem)
    return _CASES[kind]


@pytest.mark.parametrize('kind', ['gan', 'vae'])
def test_forward_mean_matches_oracle_for_every_chunking(kind):
    """B = 3 members, M = 5 realisations, member_offset 7, step 3: chunk 6 (R = 2, with a partial last chunk), chunk 3 (R = 1)
    and the automatic chunk (all five realisations in one launch), de-mean on and off, every member; repeatable bit for bit"""
    c = _case(kind)
    gen = _gpu_generator(kind)
    N, B, M = c['N'], c['B'], c['M']
    qd = torch.as_tensor(c['q']).cuda().contiguous()
    kw = dict(seed=c['seed'], member_offset=c['off'], step=c['t'])
    scale = np.abs(c['dem']).max(axis=(-2, -1), keepdims=True)
    for chunk in (6, 3, 0):
        S = gen.forward_mean(qd, M, demean=True, chunk=chunk, **kw)
        Sraw = gen.forward_mean(qd, M, demean=False, chunk=chunk, **kw)
        again = gen.forward_mean(qd, M, demean=True, chunk=chunk, **kw)
        assert torch.equal(S, again)
        S, Sraw = S.cpu().numpy(), Sraw.cpu().numpy()
        errs = [(_s_err(Sraw[b], c['raw'][b], c['dem'][b]), _s_err(S[b], c['dem'][b])) for b in range(B)]
        print(f'\n{kind} chunk={chunk}: max error / max|S| raw, de-meaned per member {errs}')
        for e_raw, e_dem in errs:
            assert e_raw < S_TOL and e_dem < S_TOL
        assert np.abs(S.mean(axis=(-2, -1))).max() < 1e-14 * scale.max() * N * N
        # de-meaning is not a rounding-level step of this fixture, and neither is the member offset
        assert _s_err(Sraw, c['dem']) > 10 * S_TOL
    other = gen.forward_mean(qd, M, demean=True, seed=c['seed'], member_offset=c['off'] + 1, step=c['t']).cpu().numpy()
    assert _s_err(other, c['dem']) > 10 * S_TOL
    assert gen.range_ok() is None


@pytest.mark.parametrize('kind', ['gan+reg', 'vae+reg'])
def test_forward_mean_with_a_regression_net(kind):
    """regression != 'None' (cgan_regression.py:169-170): the regression net is added ONCE to the mean of the realisations"""
    c = _case(kind)
    gen = _gpu_generator(kind)
    qd = torch.as_tensor(c['q']).cuda().contiguous()
    kw = dict(seed=c['seed'], member_offset=c['off'], step=c['t'])
    for chunk in (0, 4):
        S = gen.forward_mean(qd, c['M'], demean=True, chunk=chunk, **kw).cpu().numpy()
        Sraw = gen.forward_mean(qd, c['M'], demean=False, chunk=chunk, **kw).cpu().numpy()
        for b in range(c['B']):
            assert _s_err(Sraw[b], c['raw'][b], c['dem'][b]) < S_TOL
            assert _s_err(S[b], c['dem'][b]) < S_TOL
    # the regression net is not a rounding-level term of this fixture
    plain = _gpu_generator(kind[:-4]).forward_mean(qd, c['M'], demean=False, **kw).cpu().numpy()
    assert _s_err(plain, c['raw'], c['dem']) > 1e-2


def test_forward_mean_gz_is_the_mean_net_alone():
    """mean_var_model.py:111-115: S = y_std * net_mean(q / x_std), whatever M"""
    N, B = 48, 3
    gen = _gpu_generator('gz')
    ora = load_generator('gz')
    q = _eddy_like_q(np.random.RandomState(19), B, N)
    qd = torch.as_tensor(q).cuda().contiguous()
    ref = np.stack([ora.predict_mean_snapshot(q[b]) for b in range(B)])
    outs = [gen.forward_mean(qd, M, demean=False, seed=5, step=2) for M in (1, 7)]
    assert torch.equal(outs[0], outs[1])
    for b in range(B):
        assert _s_err(outs[0][b].cpu().numpy(), ref[b]) < S_TOL
    S = gen.forward_mean(qd, 7, demean=True).cpu().numpy()
    for b in range(B):
        assert _s_err(S[b], gen_ref.demean(ref[b])) < S_TOL


def test_forward_mean_unet_handle():
    """the DeepInversion U-Net as net 0 (qgx_generator_create_unet), against tests/unet_restatement.py"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    import unet_restatement as U
    N, B, M, seed, off, t = 32, 1, 3, 9, 2, 1
    d = golden('weights_gan.npz')
    xs, ys = np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32) / np.float32(16)
    net = weights.synthetic_unet()
    gen = qa.Generator('gan', [net], xs, ys)
    sd = U.to_torch(net)
    q = _eddy_like_q(np.random.RandomState(23), B, N)
    z = _realisations(seed, off, t, M, N)
    X = (q[0].astype('float32')[None] / xs.reshape(1, 2, 1, 1))
    Y = U.forward(sd, torch.as_tensor(np.concatenate([np.tile(X, (M, 1, 1, 1)), z], axis=1))).numpy().mean(0, keepdims=True)
    ref = (Y * ys.reshape(1, 2, 1, 1)).squeeze().astype('float64')
    qd = torch.as_tensor(q).cuda().contiguous()
    for chunk in (0, 2):
        S = gen.forward_mean(qd, M, demean=False, chunk=chunk, seed=seed, member_offset=off, step=t).cpu().numpy()[0]
        assert _s_err(S, ref) < S_TOL
    one = gen.forward_mean(qd, 1, demean=False, seed=seed, member_offset=off, step=t).cpu().numpy()[0]
    assert _s_err(one, ref) > 10 * S_TOL          # the mean is not one realisation


class _MeanPlugin:
    """test-local deterministic-sampling plugin for QGModelRef: the oracle's predict_mean_snapshot on the realisations the
    device draws, key-step advancing by one per call (parameterization.py:27-28 with the pinned stream)"""

    def __init__(self, ora, M, seed, member, weight):
        self.ora, self.M, self.seed, self.member, self.weight, self.t = ora, M, seed, member, weight, 0

    def __call__(self, m):
        z = _realisations(self.seed, self.member, self.t, self.M, m.nx)
        m.PV_forcing = gen_ref.demean(self.ora.predict_mean_snapshot(m.q, self.M, z=z))
        self.t += 1
        return self.weight * m.PV_forcing


ONLINE = dict(N=48, B=2, M=4, weight=0.5, seed=13, off=5, nsteps=3, dt=14400.)


def _online_engine(q0, **opts):
    import pyqg_generative_amd as qa
    e = qa.EnsembleEngine(nx=ONLINE['N'], n_members=ONLINE['B'], dt=ONLINE['dt'])
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_q(q0)
    return e


def _det_step(e, gen, n, **kw):
    o = ONLINE
    e.step(n, generator=gen, sampling='deterministic', n_mean=kw.pop('n_mean', o['M']), weight=o['weight'], seed=o['seed'],
           member_offset=o['off'], **kw)


@pytest.fixture(scope='module')
def online_q0():
    q0 = _eddy_like_q(np.random.RandomState(29), ONLINE['B'], ONLINE['N'])
    q0.setflags(write=False)
    return q0


def test_deterministic_steps_match_oracle(online_q0):
    """three online steps, gan, 2 members, M = 4, weight 0.5: the forcing of every step and qh at the end against QGModelRef;
    three steps in one call are bit-identical to three calls; the latent noise is untouched; never in halves; another
    chunking stays inside the tolerances"""
    import pyqg_generative_amd._lib as L
    o = ONLINE
    gen = _gpu_generator('gan')
    ora = load_generator('gan')
    refs = []
    for b in range(o['B']):
        m = qg_ref.QGModelRef(nx=o['N'], dt=o['dt'])
        m.sampling_type = 'deterministic'
        m.q_parameterization = _MeanPlugin(ora, o['M'], o['seed'], o['off'] + b, o['weight'])
        m.set_q(online_q0[b])
        refs.append(m)
    e1, e3, e4 = _online_engine(online_q0), _online_engine(online_q0), _online_engine(online_q0, mean_chunk=4, streams=2)
    z_before = e1.get(L.F_Z).clone()
    for s in range(o['nsteps']):
        _det_step(e1, gen, 1)
        _det_step(e4, gen, 1)
        for m in refs:
            m._step_forward()
        S, S4 = e1.get(L.F_S).cpu().numpy(), e4.get(L.F_S).cpu().numpy()
        for b, m in enumerate(refs):
            assert _s_err(S[b], m.PV_forcing) < S_TOL, (s, b)
            assert _s_err(S4[b], m.PV_forcing) < S_TOL, (s, b)
    _det_step(e3, gen, o['nsteps'])
    for f in (L.F_QH, L.F_S, L.F_Q):
        assert torch.equal(e1.get(f), e3.get(f)), f
    qh, qh4 = e1.get(L.F_QH).cpu().numpy(), e4.get(L.F_QH).cpu().numpy()
    for b, m in enumerate(refs):
        assert np.abs(qh[b] - m.qh).max() < QH_TOL * np.abs(m.qh).max(), b
        assert np.abs(qh4[b] - m.qh).max() < QH_TOL * np.abs(m.qh).max(), b
    assert e1.tc == o['nsteps'] and e3.tc == o['nsteps']
    assert torch.equal(e1.get(L.F_Z), z_before)
    # the forcing is not a rounding-level term of these steps
    free = _online_engine(online_q0)
    free.step(o['nsteps'])
    assert np.abs(free.get(L.F_QH).cpu().numpy() - qh).max() > 100 * QH_TOL * np.abs(qh).max()
    # an even ensemble whose AR1 / constant steps go in two halves steps the deterministic mode on one stream
    assert e4.step_streams(gen) == 2 and e4.step_streams(gen, sampling='deterministic') == 1
    assert gen.range_ok() is None
    for e in (e1, e3, e4, free):
        e.close()


def test_run_simulation_deterministic_ensemble(online_q0):
    """run_simulation(..., sampling='deterministic', M=4, n_members=2): the facade routes the mode to the device for the whole
    ensemble; its final q is the engine-level run's"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.simulate import run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    o = ONLINE
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    model = CGANRegression.from_arrays(nets, xs, ys)
    params = EDDY_PARAMS.nx(o['N'])._update({'tmax': o['dt'] * 3, 'log_level': 0})
    calls = []
    model.predict_mean_snapshot = lambda *a, **k: calls.append(1)       # the host plugin path is not taken
    ds = run_simulation(dict(params), parameterization=dict(self=model, sampling='deterministic', nsteps=1, M=o['M']),
                        q_init=np.array(online_q0), sampling_freq=o['dt'] * 3, n_members=o['B'], seed=o['seed'],
                        member_offset=o['off'])
    assert not calls
    q = np.asarray(ds['q'].values)
    assert q.shape[0] == o['B'] and q.shape[-3:] == (2, o['N'], o['N'])
    e = qa.EnsembleEngine(nx=o['N'], n_members=o['B'], dt=o['dt'])
    e.set_q(np.array(online_q0))
    e.step(3, generator=model.device_generator(), sampling='deterministic', n_mean=o['M'], seed=o['seed'], member_offset=o['off'])
    ref = e.get(L.F_Q).cpu().numpy()
    e.close()
    last = q[:, -1]
    # snapshots are stored as float32
    assert np.abs(last - ref.astype('float32')).max() <= 1e-6 * np.abs(ref).max()
    # M reached the device: another M gives another run
    e = qa.EnsembleEngine(nx=o['N'], n_members=o['B'], dt=o['dt'])
    e.set_q(np.array(online_q0))
    e.step(3, generator=model.device_generator(), sampling='deterministic', n_mean=1, seed=o['seed'], member_offset=o['off'])
    assert np.abs(e.get(L.F_Q).cpu().numpy() - ref).max() > 1e-5 * np.abs(ref).max()
    e.close()


def test_stochastic_model_default_n_mean_is_the_references():
    from pyqg_generative_amd.tools.stochastic_pyqg import stochastic_QGModel
    m = stochastic_QGModel(dict(nx=48, dt=14400., log_level=0), 'deterministic')
    assert m.n_mean == 100
    m.close()
    m = stochastic_QGModel(dict(nx=48, dt=14400., log_level=0), 'deterministic', n_mean=7)
    assert m.n_mean == 7
    m.close()


def _snapshot(e):
    import pyqg_generative_amd._lib as L
    return [e.get(f).clone() for f in (L.F_QH, L.F_Q, L.F_S, L.F_Z)] + [torch.as_tensor(e.tc)]


def test_refusals_leave_the_model_where_it_was(online_q0):
    """n_mean = 0, external noise, an OLS generator, a grid the nets do not take (24 x 24), a mean_chunk below the member
    count: refused before anything is launched or changed — state, forcing, latent noise and step count bitwise as they
    were, and the next AR1 step the one a model that never saw the refusals takes (sampler state and noise counter)"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    from pyqg_generative_amd._lib import QgxError
    o = ONLINE
    N, B = o['N'], o['B']
    gen = _gpu_generator('gan')
    d = golden('weights_gz.npz')
    ols = qa.Generator('ols', [weights.net_from_npz(d, 'net0_')], np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32))
    e, twin = _online_engine(online_q0), _online_engine(online_q0)
    for m in (e, twin):
        m.step(2, generator=gen, sampling='AR1', nsteps_decor=3, seed=4)
    before = _snapshot(e)
    z = torch.zeros((B, 2, N, N), dtype=torch.float32, device='cuda')
    with pytest.raises(QgxError, match='n_mean'):
        _det_step(e, gen, 1, n_mean=0)
    with pytest.raises(QgxError, match='z_external'):
        _det_step(e, gen, 1, z_external=z)
    with pytest.raises(QgxError, match='predict_mean_snapshot'):
        _det_step(e, ols, 1)
    e.set_option('mean_chunk', B - 1)
    with pytest.raises(QgxError, match='chunk'):
        _det_step(e, gen, 1)
    e.set_option('mean_chunk', 0)
    with pytest.raises(QgxError, match='predict_mean_snapshot'):
        ols.forward_mean(torch.as_tensor(np.array(online_q0)).cuda(), 3)
    for a, b in zip(before, _snapshot(e)):
        assert torch.equal(a, b)
    for m in (e, twin):
        m.step(1, generator=gen, sampling='AR1', nsteps_decor=3, seed=4)
    for a, b in zip(_snapshot(e), _snapshot(twin)):
        assert torch.equal(a, b)
    e.close()
    twin.close()
    # 24 x 24: a grid qgx_create admits and the AndrewCNN kernels do not take
    N = 24
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=o['dt'])
    e.set_q(_eddy_like_q(np.random.RandomState(3), B, N))
    e.step(1)
    before = _snapshot(e)
    with pytest.raises((QgxError, ValueError), match='24'):
        _det_step(e, gen, 1)
    p = L_param(gen, n_mean=4)
    from pyqg_generative_amd._lib import lib
    assert lib.qgx_step(e._h, 1, p, 1, None) == -1 and b'24' in lib.qgx_last_error()      # the library's own refusal
    with pytest.raises((QgxError, ValueError), match='24'):
        gen.forward_mean(e.get(0), 4)
    for a, b in zip(before, _snapshot(e)):
        assert torch.equal(a, b)
    e.close()


def L_param(gen, n_mean):
    """a qgx_param for a deterministic step, as EnsembleEngine.step fills it (for calls past its Python-side checks)"""
    import ctypes as C
    from pyqg_generative_amd import _lib
    p = _lib.qgx_param()
    p.gen, p.sampling, p.nsteps, p.weight, p.demean, p.n_mean = gen._h, _lib.SAMPLING_DETERMINISTIC, 1, 1.0, 1, n_mean
    return C.byref(p)
