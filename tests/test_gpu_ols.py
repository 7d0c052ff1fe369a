"""GPU: OLSModel, the deterministic CNN parameterization (QGX_GEN_OLS) — forward against the reference's predict_snapshot
(tests/golden/ols.npz), member independence, online steps against the CPU oracle with the test-side restatement
(tests/ols_restatement.py), the noise-free fused step schedules, the facade and the refused inputs."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

HIDDEN = [128, 64, 32, 32, 32, 32, 32]


def _gz_net():
    from pyqg_generative_amd import weights
    return weights.net_from_npz(golden('weights_gz.npz'), 'net0_')


def _scales():
    d = golden('weights_gz.npz')
    return np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32)


def _gpu_ols():
    import pyqg_generative_amd as qa
    xs, ys = _scales()
    return qa.Generator('ols', [_gz_net()], xs, ys)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _eddy_like_q(rs, B, N):
    """band-limited random PV with the amplitude of the training data (q / x_std of unit variance per layer), as
    tests/golden/make_golden_ols.py draws it"""
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N)
    qh = np.fft.rfftn(rs.randn(B, 2, N, N), axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    q = np.fft.irfftn(qh, axes=(-2, -1))
    return q / q.std(axis=(-2, -1), keepdims=True) * _scales()[0].astype('float64').reshape(1, 2, 1, 1)


def _write_folder(path, model_args=True):
    """a reference-layout OLSModel folder (ols_model.py:50-56) holding GZ's net_mean, as make_golden_ols.py wrote it"""
    net = _gz_net()
    sd = {}
    for i in range(8):
        sd[f'conv.{3 * i}.weight'] = torch.as_tensor(net['conv_w'][i])
        sd[f'conv.{3 * i}.bias'] = torch.as_tensor(net['conv_b'][i])
        if i < 7:
            for key, name in (('bn_g', 'weight'), ('bn_b', 'bias'), ('bn_m', 'running_mean'), ('bn_v', 'running_var')):
                sd[f'conv.{3 * i + 2}.{name}'] = torch.as_tensor(net[key][i])
            sd[f'conv.{3 * i + 2}.num_batches_tracked'] = torch.tensor(1)
    torch.save(sd, os.path.join(path, 'net.pt'))
    for name, std in zip(('x_scale.json', 'y_scale.json'), _scales()):
        std = std.reshape(1, 2, 1, 1)
        with open(os.path.join(path, name), 'w') as f:
            json.dump(dict(mean=str((0 * std).tolist()), std=str(std.tolist())), f)
    if model_args:
        with open(os.path.join(path, 'model_args.json'), 'w') as f:
            json.dump(dict(model='OLSModel', div=False, batch_norm=True, bias=True, final_activation='None',
                           hidden_channels=HIDDEN), f)
    return str(path)


@pytest.fixture(scope='module')
def gen():
    return _gpu_ols()


@pytest.mark.parametrize('N', [48, 64, 96])
def test_forward_matches_reference_golden(gen, N):
    """qgx_generator_forward (demean 0) on 1 and 40 members against the reference's predict_snapshot: the generator bound
    (2e-5 of max|y|) on the default kernels, the float32 class on the exact-f32 kernels"""
    d = golden('ols.npz')
    q, S = d[f'q{N}'].astype('float64'), d[f'S{N}'].astype('float64')
    T = q.shape[0]
    for B in (1, 40):
        qd = torch.as_tensor(np.ascontiguousarray(np.resize(q, (B, 2, N, N)))).cuda()
        ref = np.resize(S, (B, 2, N, N))
        out = gen.forward(qd, demean=False).cpu().numpy()
        worst = max(_rel(out[b], ref[b]) for b in range(B))
        print(f'\nOLS N={N} B={B}: max error {worst:.2e} of max|S| (layer 2 kernel {gen.layer2_kernel(B, N)}, {gen.wino_info(N)})')
        assert worst < 2e-5
    gen.set_option('precision', 0)
    try:
        out = gen.forward(torch.as_tensor(q).cuda(), demean=False).cpu().numpy()
    finally:
        gen.set_option('auto', 0)
    errs = [_rel(out[t], S[t]) for t in range(T)]
    print(f'OLS N={N} exact-f32: max error {max(errs):.2e}')
    assert max(errs) < 5e-6
    assert gen.range_ok() is None


def test_member_copies_are_bit_identical_in_an_ensemble(gen):
    """copies of a member spread over a 128-member ensemble (forward and online steps) stay bit-identical"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    N, B = 64, 128
    rs = np.random.RandomState(5)
    q = _eddy_like_q(rs, B, N)
    pos = [0, 37, 64, 101, B - 1]
    q[pos] = q[0]
    S = gen.forward(torch.as_tensor(q).cuda(), demean=True)
    for p in pos[1:]:
        assert torch.equal(S[p], S[0]), p
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    e.set_q(q)
    e.step(5, generator=gen, sampling='AR1', nsteps_decor=1)
    for f in (L.F_QH, L.F_S):
        x = e.get(f)
        for p in pos[1:]:
            assert torch.equal(x[p], x[0]), (f, p)
    e.close()


def _oracle_models(q0, N, sampling, nd, weight, params, members):
    from oracle import qg_ref, gen_ref, samplers_ref
    from ols_restatement import OLSRef
    ora = OLSRef.from_fixture()
    refs = []
    for b in members:
        m = qg_ref.QGModelRef(nx=N, **params)
        m.sampling_type = sampling
        m.noise_sampler = samplers_ref.make_sampler(sampling, nd)
        m.q_parameterization = gen_ref.ParameterizationRef(ora, weight=weight)
        m.set_q(q0[b])
        refs.append(m)
    return refs


@pytest.mark.parametrize('sampling,nd,N,B,weight', [
    ('constant', 1, 64, 4, 1.0),
    ('constant', 3, 64, 4, 1.0),
    ('AR1', 1, 48, 3, 1.0),
    ('AR1', -1, 64, 2, 1.0),
    ('constant', 1, 32, 2, 0.5),
    ('constant', 3, 96, 16, 1.0),
    ('AR1', 1, 128, 2, 1.0),
], ids=['const1-64', 'const3-64', 'ar1-48', 'ar1-frozen-64', 'const1-32-w05', 'const3-96-halves', 'ar1-128'])
def test_online_steps_match_oracle(gen, sampling, nd, N, B, weight):
    """sampler + net + de-mean + spectral step in chunks of several steps (the fused input / output of consecutive steps)
    against QGModelRef + ParameterizationRef + the restatement; bounds of test_gpu_parity.py (forcing 2e-5 of max|S|,
    qh 5e-7).  constant with nsteps = 3 holds the forcing computed from the q of steps 1, 4, 7, ..."""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    params = dict(dt=14400.) if N <= 64 else dict(dt=7200.)
    q0 = _eddy_like_q(np.random.RandomState(31 + N), B, N)
    members = sorted({0, B // 2, B - 1})
    refs = _oracle_models(q0, N, sampling, nd, weight, params, members)
    e = qa.EnsembleEngine(nx=N, n_members=B, **params)
    e.set_q(q0)
    if N == 96:
        assert e.step_streams(gen) == 2          # the two half-ensembles of the automatic choice
    worst_S = worst_q = 0.0
    S_prev, t = None, 0
    for chunk in (1, 2, 4):
        e.step(chunk, generator=gen, sampling=sampling, nsteps_decor=nd, weight=weight, seed=123)
        for m in refs:
            for _ in range(chunk):
                m._step_forward()
        t += chunk
        qh = e.get(L.F_QH).cpu().numpy()
        S = e.get(L.F_S).cpu().numpy()
        for i, (b, m) in enumerate(zip(members, refs)):
            sc = np.abs(m.PV_forcing).max(axis=(1, 2), keepdims=True)
            eS = (np.abs(S[b] - m.PV_forcing) / sc).max()
            eq = _rel(qh[b], m.qh)
            worst_S, worst_q = max(worst_S, eS), max(worst_q, eq)
            assert eS < 2e-5, (t, b)
            assert eq < 5e-7, (t, b)
        if sampling == 'constant' and nd == 3 and t == 3:
            assert torch.equal(torch.as_tensor(S), S_prev)          # steps 2 and 3 hold the forcing of step 1
        if t == 7:
            assert not torch.equal(torch.as_tensor(S), S_prev)      # recomputed (constant, nsteps = 3: on step 7)
        S_prev = torch.as_tensor(S)
    assert gen.range_ok() is None
    print(f'\nOLS {sampling} {nd} N={N} B={B} w={weight}: worst S error {worst_S:.2e}, worst qh error {worst_q:.2e}')
    e.close()


def _lib_diags():
    from pyqg_generative_amd._lib import DIAGS
    return DIAGS


@pytest.mark.parametrize('sampling,nd', [('constant', 3), ('AR1', 1)])
def test_fused_step_changes_nothing(gen, sampling, nd):
    """Layer-split small grids: the output kernel in the step kernel's prologue, the next input float(q)/x_std in its epilogue
    (no Philox, no z), on every step before a recompute — bit-identical to separate kernels (genfuse = 0), to the
    two-workgroup and cross-XCD forms (siblings = 0 / 2), to the two-kernel step (split_adv = 1) and, as two half-ensembles
    (streams = 2), to the halves with separate kernels; state, forcing, diagnostics and the range words"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    N, B = 64, 4
    q0 = _eddy_like_q(np.random.RandomState(7), B, N)
    res = []
    sets = ({}, dict(genfuse=0), dict(siblings=0), dict(siblings=2), dict(split_adv=1), dict(split_adv=1, genfuse=0),
            dict(streams=2), dict(streams=2, genfuse=0))
    for opts in sets:
        e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
        for opt, val in opts.items():
            e.set_option(opt, val)
        e.set_q(q0)
        e.diag_config(0, 4)
        gen.range_read()
        for chunk in (7, 1, 5):
            e.step(chunk, generator=gen, sampling=sampling, nsteps_decor=nd, seed=11, member_offset=3)
        res.append([e.get(f).clone() for f in (L.F_QH, L.F_S, L.F_Q, L.F_U, L.F_PH)] +
                   [e.diag(n).clone() for n in _lib_diags()] +
                   [torch.as_tensor(gen.range_read()[1]), torch.as_tensor(e.diag_count), torch.as_tensor(e.tc)])
        e.close()
    for i, j in ((0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (6, 7)):
        for k, (a, b) in enumerate(zip(res[i], res[j])):
            assert torch.equal(a, b), (sets[j], k)


def test_model_folder_run_simulation_matches_oracle(tmp_path):
    """OLSModel(folder) through run_simulation (sampling 'constant', nsteps 1: the fused device path) against the oracle"""
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.tools.simulate import run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    model = OLSModel(folder=_write_folder(tmp_path))
    assert model.generate_latent_noise(64, 64) == 0
    N, nsteps = 64, 10
    q0 = _eddy_like_q(np.random.RandomState(2), 1, N)[0]
    params = EDDY_PARAMS.nx(N)._update({'tmax': 14400. * nsteps, 'log_level': 0})
    ds = run_simulation(dict(params), parameterization=dict(self=model, sampling='constant', nsteps=1), q_init=q0,
                        sampling_freq=14400. * 5)
    q = np.asarray(ds['q'].values)
    assert q.shape == (3, 2, N, N)
    m = _oracle_models(q0[None], N, 'constant', 1, 1.0, dict(dt=14400.), [0])[0]
    for _ in range(nsteps):
        m._step_forward()
    sc = np.abs(m.q).max(axis=(1, 2), keepdims=True)
    err = (np.abs(q[-1] - m.q) / sc).max()
    print(f'\nrun_simulation OLS, {nsteps} steps: max error {err:.2e}')
    assert err < 2e-5


def test_forecast_with_one_member_and_load_parameterization(tmp_path):
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.qgmodel import WeightedParameterization
    from pyqg_generative_amd.tools.simulate import run_forecast, load_parameterization
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    folder = _write_folder(tmp_path)
    p = load_parameterization(folder, model_weight=0.5)
    assert isinstance(p, WeightedParameterization) and p.weight == 0.5 and isinstance(p.param, OLSModel)
    assert p.param.x_scale.std.reshape(-1).tolist() == _scales()[0].tolist()
    d = golden('ols.npz')

    class _M:
        pass
    m = _M()
    m.q = d['q48'][0].astype('float64')
    S = p.param.predict_snapshot(m, np.ones(3))           # noise is ignored
    assert S.shape == (2, 48, 48) and _rel(S, d['S48'][0].astype('float64')) < 2e-5
    # run_forecasting.py:31,56: OLS is run with n_ens = 1
    N, ndays = 48, 1
    params = EDDY_PARAMS.nx(N)._update({'tmax': 86400. * ndays, 'log_level': 0})
    out = run_forecast(dict(params), dict(self=p, sampling='constant', nsteps=1), m.q, n_ens=1, seed=5)
    q, qm = np.asarray(out['q'].values), np.asarray(out['q_mean'].values)
    assert q.shape == (ndays + 1, 2, N, N) and np.isfinite(q).all()
    np.testing.assert_array_equal(q, qm)
    ref = _oracle_models(m.q[None], N, 'constant', 1, 0.5, dict(dt=14400.), [0])[0]
    for _ in range(6):
        ref._step_forward()
    sc = np.abs(ref.q).max(axis=(1, 2), keepdims=True)
    assert (np.abs(q[-1] - ref.q) / sc).max() < 2e-5


def test_predict_layout_and_deterministic_sampling(tmp_path):
    from pyqg_generative_amd.models import OLSModel
    from pyqg_generative_amd.tools.simulate import dataset_backend, run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    xr = dataset_backend()
    model = OLSModel(folder=_write_folder(tmp_path, model_args=False))
    d = golden('ols.npz')
    q = d['q64'].astype('float64').reshape(1, 2, 2, 64, 64)
    out = model.predict(xr.Dataset({'q': (['run', 'time', 'lev', 'y', 'x'], q)}), M=5)
    for name in ('q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var'):
        assert out[name].dims == ('run', 'time', 'lev', 'y', 'x') and out[name].shape == q.shape
    Y = np.asarray(out['q_forcing_advection'].values)
    np.testing.assert_array_equal(Y, np.asarray(out['q_forcing_advection_mean'].values))
    assert (np.asarray(out['q_forcing_advection_var'].values) == 0).all()
    S = d['S64'].astype('float64')
    for t in range(2):
        assert _rel(Y[0, t], S[t]) < 2e-5
    # the reference defines no predict_mean_snapshot for OLSModel
    params = EDDY_PARAMS.nx(64)._update({'tmax': 14400. * 2, 'log_level': 0})
    with pytest.raises((NotImplementedError, TypeError)):
        run_simulation(dict(params), parameterization=dict(self=model, sampling='deterministic', nsteps=1),
                       q_init=q[0, 0], sampling_freq=14400.)


def test_refused_inputs(gen):
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    from pyqg_generative_amd._lib import QgxError
    xs, ys = _scales()
    with pytest.raises(QgxError):
        qa.Generator('ols', [_gz_net(), _gz_net()], xs, ys)                 # n_nets = 2
    with pytest.raises(QgxError):
        qa.Generator('ols', weights.synthetic('gan', seed=3)[0], xs, ys)    # a 4-channel net
    N, B = 64, 2
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    e.set_q(_eddy_like_q(np.random.RandomState(1), B, N))
    z = torch.zeros((B, 2, N, N), dtype=torch.float32, device='cuda')
    with pytest.raises(QgxError, match='noise'):
        e.step(1, generator=gen, sampling='AR1', nsteps_decor=1, z_external=z)
    assert e.tc == 0
    e.close()
    x = torch.zeros((1, 2, N, N), dtype=torch.float32, device='cuda')
    with pytest.raises(QgxError):
        gen.cnn_forward(x, inet=1)
    with pytest.raises(ValueError):
        gen.forward(torch.zeros((1, 2, N, N), dtype=torch.float64, device='cuda'), z)
    assert gen.noise_dtype is None and gen.n_in == 2
    # the AndrewCNN queries and options work on the OLS handle
    assert gen.info()['precision'] in (0, 3)
    assert gen.wino_info(64)['N'] == 64
    assert gen.layer2_kernel(B, N) in range(5)
