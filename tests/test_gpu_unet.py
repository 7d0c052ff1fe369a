"""GPU: the DeepInversion U-Net generator (CGANRegression(generator='DeepInversion'), unet.hip) against the reference's
forward (tests/golden/unet.npz), member independence, the online step against the CPU oracle, the fused step schedules,
the model-folder facade and the refused inputs."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

JET = dict(dt=7200., rek=7e-8, delta=0.1, beta=1e-11)      # tools/parameters.py:26-27,37


def _unet():
    from pyqg_generative_amd import weights
    return weights.synthetic_unet()


def _scales():
    """the CGAN fixture's scalers; y_std / 16 (exact) because the recipe U-Net's outputs (max|y| ~ 50) are an order of
    magnitude above a trained generator's, and the qh bound of the online test is set for forcing of that amplitude"""
    d = golden('weights_gan.npz')
    return np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32) / np.float32(16)


def _gpu_unet(regression=False):
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    nets = [_unet()]
    if regression:
        nets.append(weights.net_from_npz(golden('weights_gz.npz'), 'net0_'))
    xs, ys = _scales()
    return qa.Generator('gan', nets, xs, ys)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _eddy_like_q(rs, B, N):
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N)
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    qh = np.fft.rfftn(q, axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    return np.fft.irfftn(qh, axes=(-2, -1)) * 3.0


@pytest.fixture(scope='module')
def gen():
    return _gpu_unet()


@pytest.mark.parametrize('N', [32, 48, 64, 96, 128])
def test_raw_forward_matches_reference(gen, N):
    d = golden('unet.npz')
    x, y = d[f'x{N}'], d[f'y{N}']
    out = gen.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
    err = np.abs(out - y).max() / np.abs(y).max()
    print(f'\nU-Net N={N} B={x.shape[0]}: max error {err:.2e} of max|y| ({np.abs(y).max():.3g})')
    assert err < 2e-5


def test_member_is_bit_identical_in_any_ensemble(gen):
    N = 64
    rs = np.random.RandomState(3)
    member = rs.randn(1, 4, N, N).astype(np.float32)
    outs = []
    for B in (1, 2, 40, 128):
        x = rs.randn(B, 4, N, N).astype(np.float32)
        pos = B // 2
        x[pos] = member[0]
        outs.append(gen.cnn_forward(torch.as_tensor(x).cuda())[pos].cpu().numpy())
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])


class _UNetGeneratorRef:
    """oracle.gen_ref.GeneratorRef whose generator is the test-side U-Net restatement (tests/unet_restatement.py)"""

    @staticmethod
    def make(regression):
        from oracle.gen_ref import GeneratorRef, CNNWeights, cnn_forward
        import unet_restatement as U

        class Ref(GeneratorRef):
            def __init__(self):
                xs, ys = _scales()
                nets = [None] + ([CNNWeights.from_npz_dict(golden('weights_gz.npz'), 'net0_')] if regression else [])
                super().__init__('gan', nets, xs, ys)
                self.sd = U.to_torch(_unet())

            def predict_snapshot(self, q, noise):
                X = self.x_scale.normalize(q.astype('float32'))
                Y = U.forward(self.sd, torch.as_tensor(np.concatenate([X, noise.astype('float32')], axis=1))).numpy()
                if len(self.nets) == 2:
                    Y += cnn_forward(self.nets[1], X)
                return self.y_scale.denormalize(Y).squeeze().astype('float64')
        return Ref()


@pytest.mark.parametrize('sampling,nd,N,B,nsteps,params,regression', [
    ('AR1', 1, 64, 2, 3, dict(dt=14400.), False),
    ('constant', 2, 48, 2, 3, dict(dt=14400.), False),
    ('AR1', 1, 96, 3, 2, JET, False),
    ('AR1', 1, 64, 2, 3, dict(dt=14400.), True),
], ids=['ar1-64', 'const2-48', 'ar1-96-jet', 'ar1-64-reg'])
def test_online_step_matches_oracle_with_external_noise(sampling, nd, N, B, nsteps, params, regression):
    """sampler + U-Net + de-mean + spectral step against QGModelRef + ParameterizationRef, the white noise supplied
    externally (the bounds of test_gpu_parity.py::test_parameterized_steps_match_oracle_with_external_noise)"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from oracle import qg_ref, gen_ref, samplers_ref
    rs = np.random.RandomState(77)
    q0 = _eddy_like_q(rs, B, N)
    g = _gpu_unet(regression)
    ora = _UNetGeneratorRef.make(regression)
    e = qa.EnsembleEngine(nx=N, n_members=B, **params)
    e.set_q(q0)
    xis = [rs.randn(B, 1, 2, N, N).astype('float32') for _ in range(nsteps)]
    refs = []
    for b in range(B):
        it = iter([x[b] for x in xis])

        class _Rng:
            def __init__(self, it):
                self.it = it

            def randn(self, *shape):
                return next(self.it).astype('float64').reshape(shape)
        m = qg_ref.QGModelRef(nx=N, **params)
        m.sampling_type = sampling
        m.noise_sampler = samplers_ref.make_sampler(sampling, nd)
        m.q_parameterization = gen_ref.ParameterizationRef(ora, rng=_Rng(it))
        m.set_q(q0[b])
        refs.append(m)
    draws = 0
    worst_S = worst_q = 0.0
    for s in range(nsteps):
        xi = torch.as_tensor(np.ascontiguousarray(xis[draws].reshape(B, 2, N, N))).cuda()
        if sampling == 'AR1' or s % nd == 0:
            draws += 1
        e.step(1, generator=g, sampling=sampling, nsteps_decor=nd, z_external=xi)
        for m in refs:
            m._step_forward()
        qh = e.get(L.F_QH).cpu().numpy()
        S = e.get(L.F_S).cpu().numpy()
        for b, m in enumerate(refs):
            sc = np.abs(m.PV_forcing).max(axis=(1, 2), keepdims=True)
            eS = (np.abs(S[b] - m.PV_forcing) / sc).max()
            eq = _rel(qh[b], m.qh)
            worst_S, worst_q = max(worst_S, eS), max(worst_q, eq)
            assert eS < 2e-5, (s, b)
            assert eq < 5e-7, (s, b)
    print(f'\nU-Net {sampling} {nd} {N} {B} reg={regression}: worst S error {worst_S:.2e}, worst qh error {worst_q:.2e}')


@pytest.mark.parametrize('N,B', [(64, 128), (96, 32)])
def test_fused_step_equals_stepping_with_the_generator_output(gen, N, B):
    """qgx_step with the U-Net attached in the schedules the step picks by itself (generator output and next input fused
    into the step kernel; two half-ensembles at 96 x 96) against qgx_generator_forward's output passed as the forcing"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    nsteps, seed = 3, 99
    params = dict(dt=14400.) if N == 64 else JET
    q0 = _eddy_like_q(np.random.RandomState(11), B, N)
    e1 = qa.EnsembleEngine(nx=N, n_members=B, **params)
    e1.set_q(q0)
    e1.step(nsteps, generator=gen, sampling='AR1', nsteps_decor=1, seed=seed)
    e2 = qa.EnsembleEngine(nx=N, n_members=B, **params)
    e2.set_q(q0)
    z = torch.empty((B, 2, N, N), dtype=torch.float32, device='cuda')
    for s in range(nsteps):
        # AR1 with nsteps_decor = 1: z = xi, Philox (seed, member, draw s)
        check(lib.qgx_noise_normal(_ptr(z), 0, B, 2 * N * N, seed, 0, s, 0.0, 1.0, _stream()))
        q = e2.get(L.F_Q)
        S = gen.forward(q, z, demean=True)
        e2.step(1, forcing=S, demean=False)
    for f in (L.F_QH, L.F_Q):
        np.testing.assert_array_equal(e1.get(f).cpu().numpy(), e2.get(f).cpu().numpy())
    e1.close()
    e2.close()


def _state_dict_folder(tmp_path):
    sd = {k: torch.as_tensor(v) for k, v in _unet().items()}
    for p, _, _, bn in __import__('pyqg_generative_amd.weights', fromlist=['x']).UNET_UNITS:
        if bn:
            sd[f'{p}.bn.num_batches_tracked'] = torch.tensor(0)
            sd[f'{p}.conv.2.num_batches_tracked'] = torch.tensor(0)
    torch.save(sd, tmp_path / 'G.pt')
    xs, ys = _scales()
    for name, v in (('x_scale.json', xs), ('y_scale.json', ys)):
        with open(tmp_path / name, 'w') as f:
            json.dump({'mean': str([[[0.0]], [[0.0]]]), 'std': str([[[float(v[0])]], [[float(v[1])]]])}, f)
    with open(tmp_path / 'model_args.json', 'w') as f:
        json.dump({'model': 'CGANRegression', 'regression': 'None', 'nx': 48, 'generator': 'DeepInversion'}, f)
    return str(tmp_path)


def test_model_folder_and_forecast(tmp_path):
    from pyqg_generative_amd.models.cgan_regression import CGANRegression
    from pyqg_generative_amd.tools.simulate import run_forecast
    folder = _state_dict_folder(tmp_path)
    args = json.load(open(os.path.join(folder, 'model_args.json')))
    model = CGANRegression(folder=folder, generator=args['generator'], regression=args['regression'])
    d = golden('unet.npz')
    x, y = d['x64'], d['y64']
    out = model._gen.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
    assert np.abs(out - y).max() / np.abs(y).max() < 2e-5
    # predict_snapshot: S = y_std * U-Net([q / x_std, z])
    rs = np.random.RandomState(4)
    q = _eddy_like_q(rs, 1, 48)[0]
    z = rs.randn(1, 2, 48, 48).astype(np.float32)

    class _M:
        pass
    m = _M()
    m.q = q
    S = model.predict_snapshot(m, z)
    ref = _UNetGeneratorRef.make(False).predict_snapshot(q, z)
    assert _rel(S, ref) < 2e-5
    # a short forecast: AR1, 4 members, 48 x 48
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    params = EDDY_PARAMS.nx(48)._update({'tmax': 86400., 'log_level': 0})
    out = run_forecast(dict(params), dict(self=model, sampling='AR1', nsteps=1), q, n_ens=4, seed=5)
    q_end, qm = np.asarray(out['q'].values), np.asarray(out['q_mean'].values)
    assert q_end.shape == (2, 2, 48, 48) and np.isfinite(q_end).all() and np.isfinite(qm).all()
    assert np.abs(qm[-1] - q_end[-1]).max() > 0                        # members diverged through the noise


def test_refused_inputs(gen):
    x = torch.zeros((1, 4, 40, 40), dtype=torch.float32, device='cuda')
    with pytest.raises(ValueError):
        gen.cnn_forward(x)
    from pyqg_generative_amd._lib import QgxError
    with pytest.raises(QgxError):
        gen.set_option('precision', 3)
    with pytest.raises(QgxError):
        gen.wino_info()
    assert gen.info()['precision'] == 0
