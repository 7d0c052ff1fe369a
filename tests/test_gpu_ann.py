"""GPU: ANNModel, the pointwise stencil-ANN parameterization (qgx_generator_create_ann) — forward against the reference's
predict_snapshot (tests/golden/ann.npz) for three nets and five sizes, the NaN of zero-norm stencils, member independence,
online steps against the CPU oracle with the test-side restatement (tests/ann_restatement.py), the fused and split step
forms, the model folder through load_parameterization / run_simulation / run_forecast, predict / test_offline, and the
refused inputs."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

SIZES = (32, 48, 64, 96, 128)


def _net(tag='a'):
    from ann_restatement import net_from_fixture
    return net_from_fixture(golden('ann.npz'), tag)


def _scales():
    d = golden('ann.npz')
    return float(d['x_scale']), float(d['y_scale'])


def _gpu_ann(tag='a'):
    import pyqg_generative_amd as qa
    xs, ys = _scales()
    return qa.Generator('ann', [_net(tag)], xs, ys)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _eddy_like_q(rs, B, N):
    """band-limited random PV with the amplitude of tests/golden/make_golden_ann.py's fields"""
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N)
    qh = np.fft.rfftn(rs.randn(B, 2, N, N), axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    q = np.fft.irfftn(qh, axes=(-2, -1))
    x_std = np.array([7.784383342368528e-06, 1.0471941322975908e-06]).reshape(1, 2, 1, 1)
    return q / q.std(axis=(-2, -1), keepdims=True) * x_std


def _write_folder(path, tag='a', model_args=True):
    """a reference-layout ANNModel folder (ann_model.py:54-66) holding net `tag` of ann.npz"""
    net = _net(tag)
    sd = {}
    for l in range(len(net['w'])):
        sd[f'layers.{2 * l}.weight'] = torch.as_tensor(net['w'][l])
        sd[f'layers.{2 * l}.bias'] = torch.as_tensor(net['b'][l])
    torch.save(sd, os.path.join(path, 'net.pt'))
    xs, ys = _scales()
    with open(os.path.join(path, 'scale.json'), 'w') as f:
        json.dump({'x_scale': xs, 'y_scale': ys}, f)
    if model_args:
        with open(os.path.join(path, 'model_args.json'), 'w') as f:
            json.dump(dict(model='ANNModel', stencil_size=net['stencil_size'], hidden_channels=net['hidden'],
                           scale_invariant=net['scale_invariant']), f)
    return str(path)


@pytest.fixture(scope='module')
def gen():
    return _gpu_ann('a')


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_forward_matches_reference_golden(tag):
    """qgx_generator_forward (demean 0) on 1 and 5 members against the reference's predict_snapshot: 2e-5 of max|S|"""
    g = _gpu_ann(tag)
    d = golden('ann.npz')
    worst = 0.0
    for N in SIZES:
        q, S = d[f'q{N}'].astype('float64'), d[f'S{tag}{N}'].astype('float64')
        for B in (1, 5):
            qd = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(q, (B, 2, N, N)))).cuda()
            out = g.forward(qd, demean=False).cpu().numpy()
            err = max(_rel(out[b], S) for b in range(B))
            worst = max(worst, err)
            assert err < 2e-5, (N, B)
    print(f'\nANN net {tag}: max error {worst:.2e} of max|S| over N = {SIZES}')
    assert g.range_ok() is None


@pytest.mark.parametrize('tag', ['a', 'c'])
def test_forward_matches_restatement_beyond_the_golden_sizes(tag):
    """the ANN kernel takes every N up to 512; the golden vectors stop at 128.  24, 72, 162 and 512 against the test-side
    restatement (tests/ann_restatement.py, held to the reference's vectors in tests/test_ann_cpu.py): 2e-5 of max|S| as above"""
    from ann_restatement import ANNRef
    g = _gpu_ann(tag)
    ora = ANNRef.from_fixture(tag)
    worst = 0.0
    for N in (24, 72, 162, 512):
        for B in ((1, 3) if N < 512 else (1,)):       # (the restatement holds every stencil feature of a batch in memory)
            q = _eddy_like_q(np.random.RandomState(N + B), B, N)
            out = g.forward(torch.as_tensor(q).cuda(), demean=False).cpu().numpy()
            ref = ora.predict_snapshot(q, 0)
            err = max(_rel(out[b], ref[b]) for b in range(B))
            worst = max(worst, err)
            assert err < 2e-5, (N, B, err)
    print(f'\nANN net {tag}: max error {worst:.2e} of max|S| over N = 24, 72, 162, 512')
    assert g.range_ok() is None


def test_zero_norm_stencils_give_nan_as_the_reference():
    """scale_invariant: a stencil of norm 0 is 0/0 = NaN in torch, and ReLU keeps it NaN: the zero lower layer of
    the reference's initial condition gives a NaN forcing there, the upper layer is finite"""
    g = _gpu_ann('b')
    d = golden('ann.npz')
    q, S = d['qz32'].astype('float64'), d['Sbz32'].astype('float64')
    out = g.forward(torch.as_tensor(q[None]).cuda(), demean=False).cpu().numpy()[0]
    np.testing.assert_array_equal(np.isnan(out), np.isnan(S))
    assert np.isnan(out[1]).all() and np.isfinite(out[0]).all()
    assert _rel(out[0], S[0]) < 2e-5
    flags, _ = g.range_read()
    assert flags >> 31 & 1                   # the non-finite forcing is flagged
    raw = g.cnn_forward(torch.zeros((1, 1, 32, 32), dtype=torch.float32, device='cuda'))
    assert torch.isnan(raw).all()


@pytest.mark.parametrize('tag', ['a', 'c'])
def test_member_bits_independent_of_ensemble_and_stream(tag):
    """a member's forcing is bitwise the same alone, in 3 and in 128 members, and on another stream"""
    g = _gpu_ann(tag)
    N = 64
    q = _eddy_like_q(np.random.RandomState(5), 128, N)
    one = g.forward(torch.as_tensor(q[:1]).cuda(), demean=True)
    three = g.forward(torch.as_tensor(q[:3]).cuda(), demean=True)
    full = g.forward(torch.as_tensor(q).cuda(), demean=True)
    assert torch.equal(one[0], three[0]) and torch.equal(three, full[:3])
    q[[37, 101, 127]] = q[0]
    full = g.forward(torch.as_tensor(q).cuda(), demean=True)
    for p in (37, 101, 127):
        assert torch.equal(full[p], one[0])
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        other = g.forward(torch.as_tensor(q).cuda(), demean=True)
    s.synchronize()
    assert torch.equal(other, full)
    x = (torch.as_tensor(q[:2]).cuda().to(torch.float32) / np.float32(_scales()[0])).reshape(4, 1, N, N).contiguous()
    y = g.cnn_forward(x)
    assert y.shape == (4, 1, N, N)
    raw = (full[:2] + 0).cpu().numpy()
    ys = np.float32(_scales()[1])
    S_direct = (ys * y.cpu().numpy().reshape(2, 2, N, N)).astype('float64')
    S_direct -= S_direct.mean(axis=(-2, -1), keepdims=True)
    assert _rel(S_direct, raw) < 1e-6


def _oracle_models(q0, N, sampling, nd, weight, params, members, tag='a'):
    from oracle import qg_ref, gen_ref, samplers_ref
    from ann_restatement import ANNRef
    ora = ANNRef.from_fixture(tag)
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
    ('AR1', 1, 32, 2, 1.0),
    ('AR1', 1, 48, 3, 0.5),
    ('AR1', -1, 64, 2, 1.0),
    ('constant', 3, 64, 4, 1.0),
    ('constant', 3, 96, 16, 1.0),
    ('AR1', 1, 128, 2, 1.0),
], ids=['ar1-32', 'ar1-48-w05', 'ar1-frozen-64', 'const3-64', 'const3-96-halves', 'ar1-128'])
def test_online_steps_match_oracle(gen, sampling, nd, N, B, weight):
    """net + de-mean + spectral step in chunks of several steps against QGModelRef + ParameterizationRef + the
    restatement; the bounds of test_gpu_ols.py (forcing 2e-5 of max|S|, qh 5e-7).  constant with nsteps = 3 holds the
    forcing computed from the q of steps 1, 4, 7, ..."""
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
        for b, m in zip(members, refs):
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
    print(f'\nANN {sampling} {nd} N={N} B={B} w={weight}: worst S error {worst_S:.2e}, worst qh error {worst_q:.2e}')
    e.close()


@pytest.mark.parametrize('sampling,nd', [('constant', 3), ('AR1', 1)])
def test_fused_split_and_halves_change_nothing(gen, sampling, nd):
    """the output kernel in the step kernel's prologue (genfuse 1) or separate (0), the two-workgroup and cross-XCD forms,
    the two-kernel step (split_adv = 1) and two half-ensembles (streams = 2): bit-identical state, forcing and diagnostics"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    N, B = 64, 4
    q0 = _eddy_like_q(np.random.RandomState(7), B, N)
    res = []
    sets = ({}, dict(genfuse=0), dict(siblings=0), dict(siblings=2), dict(split_adv=1), dict(split_adv=1, genfuse=0),
            dict(streams=2), dict(streams=2, genfuse=0))
    from pyqg_generative_amd._lib import DIAGS
    for opts in sets:
        e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
        for opt, val in opts.items():
            e.set_option(opt, val)
        e.set_q(q0)
        e.diag_config(0, 4)
        for chunk in (7, 1, 5):
            e.step(chunk, generator=gen, sampling=sampling, nsteps_decor=nd, seed=11, member_offset=3)
        res.append([e.get(f).clone() for f in (L.F_QH, L.F_S, L.F_Q, L.F_U, L.F_PH)] +
                   [e.diag(n).clone() for n in DIAGS] + [torch.as_tensor(e.diag_count), torch.as_tensor(e.tc)])
        e.close()
    for j in range(1, len(sets)):
        for k, (a, b) in enumerate(zip(res[0], res[j])):
            assert torch.equal(a, b), (sets[j], k)


def test_model_folder_run_simulation_matches_oracle(tmp_path):
    """an ANNModel folder through load_parameterization + run_simulation (AR1, nsteps 1: the fused device path) against
    the oracle"""
    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.qgmodel import WeightedParameterization
    from pyqg_generative_amd.tools.simulate import run_simulation, load_parameterization
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    p = load_parameterization(_write_folder(tmp_path), model_weight=0.5)
    assert isinstance(p, WeightedParameterization) and p.weight == 0.5 and isinstance(p.param, ANNModel)
    assert (p.param.x_scale, p.param.y_scale) == _scales()
    assert p.param.generate_latent_noise(64, 64) == 0
    N, nsteps = 64, 10
    q0 = _eddy_like_q(np.random.RandomState(2), 1, N)[0]
    params = EDDY_PARAMS.nx(N)._update({'tmax': 14400. * nsteps, 'log_level': 0})
    ds = run_simulation(dict(params), parameterization=dict(self=p, sampling='AR1', nsteps=1), q_init=q0,
                        sampling_freq=14400. * 5)
    q = np.asarray(ds['q'].values)
    assert q.shape == (3, 2, N, N)
    m = _oracle_models(q0[None], N, 'AR1', 1, 0.5, dict(dt=14400.), [0])[0]
    for _ in range(nsteps):
        m._step_forward()
    sc = np.abs(m.q).max(axis=(1, 2), keepdims=True)
    err = (np.abs(q[-1] - m.q) / sc).max()
    print(f'\nrun_simulation ANN, {nsteps} steps: max error {err:.2e}')
    assert err < 2e-5


def test_forecast_and_predict_snapshot(tmp_path):
    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.tools.simulate import run_forecast
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    model = ANNModel(folder=_write_folder(tmp_path, 'c', model_args=False), stencil_size=5, hidden_channels=[32, 16, 8])
    d = golden('ann.npz')

    class _M:
        pass
    m = _M()
    m.q = d['q48'].astype('float64')
    S = model.predict_snapshot(m, np.ones(3))           # noise is ignored
    assert S.shape == (2, 48, 48) and _rel(S, d['Sc48'].astype('float64')) < 2e-5
    N, ndays = 48, 1
    params = EDDY_PARAMS.nx(N)._update({'tmax': 86400. * ndays, 'log_level': 0})
    out = run_forecast(dict(params), dict(self=model, sampling='constant', nsteps=1), m.q, n_ens=1, seed=5)
    q, qm = np.asarray(out['q'].values), np.asarray(out['q_mean'].values)
    assert q.shape == (ndays + 1, 2, N, N) and np.isfinite(q).all()
    np.testing.assert_array_equal(q, qm)
    ref = _oracle_models(m.q[None], N, 'constant', 1, 1.0, dict(dt=14400.), [0], tag='c')[0]
    for _ in range(6):
        ref._step_forward()
    sc = np.abs(ref.q).max(axis=(1, 2), keepdims=True)
    assert (np.abs(q[-1] - ref.q) / sc).max() < 2e-5


def test_predict_layout_test_offline_and_deterministic_sampling(tmp_path):
    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.tools.simulate import dataset_backend, run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    from test_gpu_offline import _dataset, FIELD_VARS, SCORES, GROUPED, SPECTRA, PDFS
    xr = dataset_backend()
    model = ANNModel(folder=_write_folder(tmp_path))
    d = golden('ann.npz')
    q = np.stack([d['q64'], d['q64'][::-1]]).astype('float64').reshape(1, 2, 2, 64, 64)
    model.PREDICT_VALUES = 2 * 64 * 64          # one snapshot per launch: the chunks of predict
    out = model.predict(xr.Dataset({'q': (['run', 'time', 'lev', 'y', 'x'], q)}), M=5)
    for name in ('q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var'):
        assert out[name].dims == ('run', 'time', 'lev', 'y', 'x') and out[name].shape == q.shape
    Y = np.asarray(out['q_forcing_advection'].values)
    np.testing.assert_array_equal(Y, np.asarray(out['q_forcing_advection_mean'].values))
    assert (np.asarray(out['q_forcing_advection_var'].values) == 0).all()
    assert _rel(Y[0, 0], d['Sa64'].astype('float64')) < 2e-5
    del model.PREDICT_VALUES

    ds = _dataset()
    res = model.test_offline(ds, 8)
    names = FIELD_VARS + SCORES + GROUPED + SPECTRA + ['L2_PSD', 'L2_Eflux', 'CSD_res', 'CSD_gen_res'] + list(PDFS)
    assert sorted(res.keys()) == sorted(names)
    gen = np.asarray(model.predict(ds)['q_forcing_advection'].values)
    np.testing.assert_array_equal(res['q_forcing_advection_gen'].values, gen.astype('float32'))
    for k in ('q_forcing_advection_gen_res', 'PSD_gen_res', 'Eflux_gen_res', 'CSD_gen_res'):
        assert (np.asarray(res[k].values) == 0).all(), k
    # the reference defines no predict_mean_snapshot for ANNModel
    params = EDDY_PARAMS.nx(64)._update({'tmax': 14400. * 2, 'log_level': 0})
    with pytest.raises((NotImplementedError, TypeError)):
        run_simulation(dict(params), parameterization=dict(self=model, sampling='deterministic', nsteps=1),
                       q_init=q[0, 0], sampling_freq=14400.)


def test_refused_inputs(gen):
    import pyqg_generative_amd as qa
    from pyqg_generative_amd._lib import QgxError
    N, B = 64, 2
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    e.set_q(_eddy_like_q(np.random.RandomState(1), B, N))
    z = torch.zeros((B, 2, N, N), dtype=torch.float32, device='cuda')
    with pytest.raises(QgxError, match='noise'):
        e.step(1, generator=gen, sampling='AR1', nsteps_decor=1, z_external=z)
    assert e.tc == 0
    e.close()
    with pytest.raises(ValueError):
        gen.forward(torch.zeros((1, 2, N, N), dtype=torch.float64, device='cuda'), z)
    with pytest.raises(QgxError):
        gen.cnn_forward(torch.zeros((1, 1, N, N), dtype=torch.float32, device='cuda'), inet=1)
    assert gen.noise_dtype is None and gen.n_in == 1
    assert gen.info()['precision'] == 0
    gen.set_option('precision', 0)
    for call in (lambda: gen.set_option('wino', 0), lambda: gen.set_option('precision', 3), lambda: gen.wino_info(64),
                 lambda: gen.wino_info(), lambda: gen.layer2_kernel(B, N), lambda: gen.profile(1), gen.profile_read):
        with pytest.raises(QgxError, match='ANN'):
            call()
    with pytest.raises(QgxError, match='N = 1024'):
        gen.forward(torch.zeros((1, 2, 1024, 1024), dtype=torch.float64, device='cuda'), demean=False)
    with pytest.raises(ValueError):
        qa.Generator('ann', [_net('a'), _net('a')], *_scales())
