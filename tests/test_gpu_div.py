"""GPU: flux-form nets, AndrewCNN(div=True) — a four-channel last layer and y = 10000 * divergence(fluxes) behind it, float32,
one LDS-resident FFT kernel (csrc/fluxdiv.hip).  Forward against the reference's own AndrewCNN(div=True) (tests/golden/
generator_div.npz), the divergence kernel alone against the float64 divergence of the device's own fluxes, zero mean, member
independence, every model kind that takes such a net, online steps against the CPU oracle with the test-side restatement
(tests/div_restatement.py), the Winograd admission on the post-divergence output, and the CGANRegression(div=True) facade."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

import div_restatement as R

pytestmark = pytest.mark.gpu

GEN_TOL = 2e-5          # the project's generator bound, of max|y|


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _generator(kind, nets):
    import pyqg_generative_amd as qa
    xs, ys = R.scales()
    return qa.Generator(kind, nets, xs, ys)


@pytest.fixture(scope='module')
def gan():
    return _generator('gan', [R.flux_net_dict('gan')])


@pytest.fixture(scope='module')
def reg():
    """regression != 'None', both nets flux-form"""
    return _generator('gan', [R.flux_net_dict('gan'), R.flux_net_dict('ols')])


@pytest.fixture(scope='module')
def ols():
    return _generator('ols', [R.flux_net_dict('ols')])


def _members(kind, N, B):
    """B members from the fixture's snapshots -> (x, y32, y64, q).  Where the fixture holds ONE snapshot (96, 128) the odd members are
    circular shifts of it: the convolutions are circular and the divergence is spectral, so the forward commutes with shifts
    exactly in exact arithmetic — the shifted y64 is the float64 forward of the shifted input to 1e-15, the shifted y32 a
    float32 evaluation of it within the reference's own float32 error (3 % of the 2e-5 it is used with)"""
    x, a, b = R.inputs(kind, N), R.y32(kind, N), R.y64(kind, N).astype('float64')
    q0 = R.fixture()[f'q{N}'].astype('float64')          # float32(q) / x_std is the fixture's input bit for bit
    T = x.shape[0]
    xs, ya, yb, qs = [], [], [], []
    for m in range(B):
        t, shift = m % T, ((5 * (m // T)) % N, (3 * (m // T)) % N)
        xs.append(np.roll(x[t], shift, axis=(-2, -1)))
        ya.append(np.roll(a[t], shift, axis=(-2, -1)))
        yb.append(np.roll(b[t], shift, axis=(-2, -1)))
        qs.append(np.roll(q0[t], shift, axis=(-2, -1)))
    return np.ascontiguousarray(np.stack(xs)), np.stack(ya), np.stack(yb), np.ascontiguousarray(np.stack(qs))


@pytest.mark.parametrize('N,B', [(16, 1), (16, 3), (48, 2), (64, 1), (64, 40), (96, 2), (128, 2)])
def test_cnn_forward_and_generator_forward_match_the_reference(gan, N, B):
    """qgx_cnn_forward and qgx_generator_forward (demean 0) against the reference's float32 forward: the generator bound on the
    default kernels; on the exact-f32 kernels the error against the reference's FLOAT64 forward within 4 x its own float32 error
    (the existing float32 class sits at 1-2e-6 where the reference's float32 sits near 5e-7).  Every layer's mean is zero
    before any de-mean."""
    x, y32, y64, q = _members('gan', N, B)
    m = np.abs(y64).max()
    xd = torch.as_tensor(x).cuda()
    xs, ys = R.scales()
    qd = torch.as_tensor(q).cuda()
    zd = torch.as_tensor(np.ascontiguousarray(x[:, 2:])).cuda()
    y = gan.cnn_forward(xd).cpu().numpy()
    assert y.shape == (B, 2, N, N)
    e_def = np.abs(y - y32).max() / m
    S = gan.forward(qd, zd, demean=False).cpu().numpy()
    ysd = ys.astype('float64').reshape(1, 2, 1, 1)
    e_gen = (np.abs(S / ysd - y32) / m).max()
    mean = np.abs(y.astype('float64').mean(axis=(-2, -1))).max() / m
    gan.set_option('precision', 0)
    try:
        y0 = gan.cnn_forward(xd).cpu().numpy()
    finally:
        gan.set_option('auto', 0)
    e_exact = np.abs(y0 - y64).max() / m
    mean0 = np.abs(y0.astype('float64').mean(axis=(-2, -1))).max() / m
    print(f'\nflux GAN N={N} B={B}: default kernels {e_def:.2e} (generator_forward {e_gen:.2e}), exact-f32 vs float64 {e_exact:.2e} '
          f'(reference float32 {R.e_ref("gan", N):.2e}), |mean|/max {mean:.1e} / {mean0:.1e}; layer 2 kernel {gan.layer2_kernel(B, N)}')
    assert e_def < GEN_TOL
    assert e_gen < GEN_TOL
    assert e_exact < 4 * R.e_ref('gan', N)
    assert mean < 1e-6 and mean0 < 1e-6
    assert gan.range_ok() is None


def test_divergence_kernel_alone():
    """N = 16, 48, 128: the device output against the float64 divergence of the device's OWN fluxes (read back from the
    workspace): the float32 FFT's rounding alone.  Bound: 4 x the error of a host float32 rfftn divergence (pocketfft through
    torch.fft, the reference's own arithmetic) on the same fluxes."""
    import subprocess
    import sys
    # the read-back lives in the A/B library, which must be the one loaded: a child process with QGX_LIB set
    code = f'''
import sys, os, ctypes as C
sys.path.insert(0, {ROOT!r}); sys.path.insert(0, os.path.join({ROOT!r}, "tests"))
import numpy as np, torch
import pyqg_generative_amd as qa
from pyqg_generative_amd._lib import lib, check
import div_restatement as R
xs, ys = R.scales()
gen = qa.Generator("gan", [R.flux_net_dict("gan")], xs, ys)
gen.set_option("precision", 0)
lib.qgx_debug_read_act.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
for N in (16, 48, 128):
    x = R.inputs("gan", N)
    B = x.shape[0]
    y = gen.cnn_forward(torch.as_tensor(x).cuda())
    F = torch.empty((B, 4, N, N), dtype=torch.float32, device="cuda")
    check(lib.qgx_debug_read_act(gen._h, 2, C.c_void_p(F.data_ptr()), F.numel() * 4, None))
    torch.cuda.synchronize()
    F, y = F.cpu().numpy(), y.cpu().numpy()
    exact = 10000. * R.divergence_rfftn(F, "float64")
    host32 = 10000. * R.divergence_rfftn(F, "float32")
    m = np.abs(exact).max()
    print("RESULT", N, np.abs(y - exact).max() / m, np.abs(host32 - exact).max() / m)
'''
    env = dict(os.environ, QGX_LIB=os.path.join(ROOT, 'pyqg_generative_amd', 'libqgx_ab.so'))
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines() if l.startswith('RESULT')]
    assert [r[1] for r in rows] == ['16', '48', '128']
    for _, N, dev, host in rows:
        dev, host = float(dev), float(host)
        print(f'\nfluxdiv alone N={N}: device {dev:.2e}, host float32 rfftn {host:.2e} of max|y|')
        assert dev <= 4 * host, N


def test_member_copies_are_bit_identical_in_an_ensemble(gan):
    N, B = 64, 128
    x, _, _, _ = _members('gan', N, 2)
    rs = np.random.RandomState(5)
    big = rs.randn(B, 4, N, N).astype(np.float32)
    pos = [0, 37, 64, 101, B - 1]
    big[pos] = x[0]
    y = gan.cnn_forward(torch.as_tensor(big).cuda())
    for p in pos[1:]:
        assert torch.equal(y[p], y[0]), p
    assert not torch.equal(y[1], y[0])


@pytest.mark.parametrize('N', [16, 64])
def test_regression_both_nets_flux_form(reg, N):
    """FIN_SUM: S = y_std (G([x, z]) + net_mean(x)), both in flux form, against the reference's CGANRegression(regression=
    'full_loss', div=True).predict_snapshot"""
    d = R.fixture()
    S_ref = d[f'S_{N}'].astype('float64')
    T = S_ref.shape[0]
    q = d[f'q{N}'][:T].astype('float64')
    z = R.latent_noise(N, d[f'q{N}'].shape[0])[:T]
    S = reg.forward(torch.as_tensor(q).cuda(), torch.as_tensor(z).cuda(), demean=False).cpu().numpy()
    errs = [(np.abs(S[t] - S_ref[t]) / np.abs(S_ref[t]).max(axis=(1, 2), keepdims=True)).max() for t in range(T)]
    print(f'\nflux regression N={N}: {errs}')
    assert max(errs) < GEN_TOL
    # net 1 alone is the OLS-kind fixture
    y1 = reg.cnn_forward(torch.as_tensor(R.inputs('ols', N)).cuda(), inet=1).cpu().numpy()
    assert _rel(y1, R.y32('ols', N)) < GEN_TOL
    # the regression net is not a rounding-level term
    plain = R.y32('gan', N)[:T] * R.scales()[1].reshape(1, 2, 1, 1)
    assert _rel(plain, S_ref) > 1e-2


def test_unet_with_a_flux_form_net_mean():
    """cgan_regression.py:50-60 with generator='DeepInversion', div=True: the U-Net is not flux-form, its net_mean is"""
    from pyqg_generative_amd import weights
    N = 64
    unet = weights.synthetic_unet()
    gen = _generator('gan', [unet, R.flux_net_dict('ols')])
    x = R.inputs('gan', N)[:1]
    y1 = gen.cnn_forward(torch.as_tensor(np.ascontiguousarray(x[:, :2])).cuda(), inet=1).cpu().numpy()
    m = np.abs(R.y64('ols', N)).max()
    assert np.abs(y1 - R.y64('ols', N)[:1]).max() < 4 * R.e_ref('ols', N) * m          # exact f32 on such a handle
    xs, ys = R.scales()
    q = x[:, :2].astype('float64') * xs.astype('float64').reshape(1, 2, 1, 1)
    S = gen.forward(torch.as_tensor(q).cuda(), torch.as_tensor(np.ascontiguousarray(x[:, 2:])).cuda(), demean=False).cpu().numpy()
    y0 = gen.cnn_forward(torch.as_tensor(x).cuda(), inet=0).cpu().numpy()
    ref = (y0 + y1) * ys.reshape(1, 2, 1, 1)
    assert _rel(S, ref.astype('float64')) < 2e-6


@pytest.mark.parametrize('N', [16, 64])
def test_ols_and_vae_kinds(ols, N):
    x, y32, y64 = R.inputs('ols', N), R.y32('ols', N), R.y64('ols', N)
    m = np.abs(y64).max()
    xs, ys = R.scales()
    y = ols.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
    assert np.abs(y - y32).max() < GEN_TOL * m
    q = R.fixture()[f'q{N}'][:x.shape[0]].astype('float64')
    S = ols.forward(torch.as_tensor(q).cuda(), demean=False).cpu().numpy()
    assert (np.abs(S / ys.astype('float64').reshape(1, 2, 1, 1) - y32) / m).max() < GEN_TOL
    ols.set_option('precision', 0)
    try:
        y0 = ols.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
    finally:
        ols.set_option('auto', 0)
    print(f'\nflux OLS N={N}: default {np.abs(y - y32).max() / m:.2e}, exact-f32 vs float64 {np.abs(y0 - y64).max() / m:.2e} '
          f'(reference float32 {R.e_ref("ols", N):.2e})')
    assert np.abs(y0 - y64).max() < 4 * R.e_ref('ols', N) * m
    # the VAE kind runs the same dataflow with the decoder: the GAN fixture's net as a decoder
    vae = _generator('vae', [R.flux_net_dict('gan')])
    xg = R.inputs('gan', N)
    yv = vae.cnn_forward(torch.as_tensor(xg).cuda()).cpu().numpy()
    assert np.abs(yv - R.y32('gan', N)).max() < GEN_TOL * np.abs(R.y32('gan', N)).max()
    vae.close()


# ---- online ---------------------------------------------------------------------------------------------------------------
def _eddy_like_q(rs, B, N):
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N)
    qh = np.fft.rfftn(rs.randn(B, 2, N, N), axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    q = np.fft.irfftn(qh, axes=(-2, -1))
    return q / q.std(axis=(-2, -1), keepdims=True) * R.scales()[0].astype('float64').reshape(1, 2, 1, 1)


def _flux_oracle():
    xs, ys = R.scales()
    return R.FluxGeneratorRef('gan', [R.flux_net_ref('gan')], xs, ys)


@pytest.mark.parametrize('sampling,nd,N,B', [('AR1', 1, 64, 4), ('constant', 2, 48, 2)], ids=['ar1-64', 'const2-48'])
def test_online_steps_match_oracle(gan, sampling, nd, N, B):
    """sampler + flux-form generator + de-mean + spectral step against QGModelRef + ParameterizationRef + the restatement, the
    white noise supplied externally; bounds of test_gpu_ols.py::test_online_steps_match_oracle (forcing 2e-5 of max|S|, qh 5e-7)"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from oracle import qg_ref, gen_ref, samplers_ref
    nsteps = 4
    rs = np.random.RandomState(77 + N)
    q0 = _eddy_like_q(rs, B, N)
    xis = [rs.randn(B, 1, 2, N, N).astype('float32') for _ in range(nsteps)]
    ora = _flux_oracle()
    refs = []
    for b in range(B):
        class _Rng:
            def __init__(self, it):
                self.it = it

            def randn(self, *shape):
                return next(self.it).astype('float64').reshape(shape)
        m = qg_ref.QGModelRef(nx=N, dt=14400.)
        m.sampling_type = sampling
        m.noise_sampler = samplers_ref.make_sampler(sampling, nd)
        m.q_parameterization = gen_ref.ParameterizationRef(ora, rng=_Rng(iter([x[b] for x in xis])))
        m.set_q(q0[b])
        refs.append(m)
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    e.set_q(q0)
    draws = 0
    worst_S = worst_q = 0.0
    for s in range(nsteps):
        xi = torch.as_tensor(np.ascontiguousarray(xis[draws].reshape(B, 2, N, N))).cuda()
        if sampling == 'AR1' or s % nd == 0:
            draws += 1
        e.step(1, generator=gan, sampling=sampling, nsteps_decor=nd, z_external=xi)
        for m in refs:
            m._step_forward()
        qh, S = e.get(L.F_QH).cpu().numpy(), e.get(L.F_S).cpu().numpy()
        for b, m in enumerate(refs):
            sc = np.abs(m.PV_forcing).max(axis=(1, 2), keepdims=True)
            eS, eq = (np.abs(S[b] - m.PV_forcing) / sc).max(), _rel(qh[b], m.qh)
            worst_S, worst_q = max(worst_S, eS), max(worst_q, eq)
            assert eS < 2e-5, (s, b)
            assert eq < 5e-7, (s, b)
    print(f'\nflux GAN online {sampling} {nd} N={N} B={B}: worst S error {worst_S:.2e}, worst qh error {worst_q:.2e}')
    assert gan.range_ok() is None
    e.close()


@pytest.mark.parametrize('sampling,nd', [('constant', 3), ('AR1', 1)])
def test_fused_step_prologue_is_bit_identical(gan, sampling, nd):
    """the deferred finish in the step kernel's prologue reads the post-divergence output (GenFuse::y stays Y0): bit-identical to
    separate kernels (genfuse = 0)"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    N, B = 64, 4
    q0 = _eddy_like_q(np.random.RandomState(7), B, N)
    res = []
    for opts in ({}, dict(genfuse=0)):
        e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
        for opt, val in opts.items():
            e.set_option(opt, val)
        e.set_q(q0)
        for chunk in (4, 1, 3):
            e.step(chunk, generator=gan, sampling=sampling, nsteps_decor=nd, seed=11, member_offset=3)
        res.append([e.get(f).clone() for f in (L.F_QH, L.F_S, L.F_Q)])
        e.close()
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), k
    assert res[0][1].abs().max() > 0


def test_deterministic_sampling(gan):
    """sampling='deterministic', M = 8: forward_mean against the restatement's predict_mean_snapshot on the pinned Philox draws,
    and one online step of it"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from oracle import samplers_ref, gen_ref
    N, B, M, seed, off, t = 48, 2, 8, 31, 7, 0
    q = _eddy_like_q(np.random.RandomState(17), B, N)
    ora = _flux_oracle()
    raw = []
    for b in range(B):
        z = np.stack([samplers_ref.philox_normal(seed, off + b, t | (j + 1) << 32, 2 * N * N)[0].reshape(2, N, N) for j in range(M)])
        raw.append(ora.predict_mean_snapshot(q[b], M, z=z.astype('float32')))
    dem = np.stack([gen_ref.demean(r) for r in raw])
    qd = torch.as_tensor(q).cuda().contiguous()
    S = gan.forward_mean(qd, M, demean=True, seed=seed, member_offset=off, step=t).cpu().numpy()
    sc = np.abs(dem).max(axis=(-2, -1), keepdims=True)
    err = (np.abs(S - dem) / sc).max()
    print(f'\nflux GAN deterministic M={M}: {err:.2e}')
    assert err < 2e-5
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    e.set_q(q)
    e.step(1, generator=gan, sampling='deterministic', seed=seed, member_offset=off, n_mean=M)
    S1 = e.get(L.F_S).cpu().numpy()
    e.close()
    assert (np.abs(S1 - dem) / sc).max() < 2e-5


# ---- Winograd admission ---------------------------------------------------------------------------------------------------
def test_wino_admission_is_measured_after_the_divergence():
    """qgx_generator_wino_info_n: the calibration compares the nets' OUTPUT — for a flux-form net that is the divergence, which
    roughly doubles relative conv error — so the same layers 1-7 report a different error with the flux head than with the
    plain one, and whichever way a size is decided the forward stays inside the generator bound without error"""
    from pyqg_generative_amd import weights
    plain_net = weights.net_from_npz(golden('weights_gan.npz'), 'net0_')
    flux = _generator('gan', [R.flux_net_dict('gan')])
    plain = _generator('gan', [plain_net])
    assert flux.info()['precision'] == 3
    for N in (48, 64, 96, 128):
        a, b = flux.wino_info(N), plain.wino_info(N)
        print(f'\nN={N}: flux head {a}, plain head {b}')
        assert np.isfinite(a['calibration_error']) and a['calibration_error'] > 0
        assert a['calibration_error'] != b['calibration_error']
        assert a['chosen_by_calibration'] == (a['calibration_error'] <= 1e-5)
        assert a['enabled'] == a['chosen_by_calibration']
    # a size the calibration refused runs the 25-tap kernels (no error), one it admitted the Winograd kernel
    for N, B in ((64, 40), (96, 2)):
        x, y32, _, _ = _members('gan', N, B)
        k = flux.layer2_kernel(B, N)
        y = flux.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
        assert np.abs(y - y32).max() < GEN_TOL * np.abs(y32).max()
        flux.set_option('wino', 0)
        y_off = flux.cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
        flux.set_option('auto', 0)
        assert flux.layer2_kernel(B, N) == k
        assert np.abs(y_off - y32).max() < GEN_TOL * np.abs(y32).max()
    flux.close()
    plain.close()


def test_net_admitted_with_the_plain_head_but_not_with_the_flux_head_falls_back():
    """weights.synthetic('gan', seed=5): the same layers 1-7; with the two-channel head the Winograd layer is admitted at 64 x 64
    (measured 9.2e-6), with a flux head it is not (2.0e-5: the divergence amplifies the layer's error) — the flux-form handle then
    runs the 25-tap kernel where the plain one runs the Winograd kernel, without error and inside the generator bound"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    N, B = 64, 40
    gens = {}
    for div in (False, True):
        nets, xs, ys = weights.synthetic('gan', seed=5, div=div)
        gens[div] = qa.Generator('gan', nets, xs, ys)
    a, b = gens[False].wino_info(N), gens[True].wino_info(N)
    print(f'\nseed 5, N={N}: plain head {a}, flux head {b}')
    assert a['chosen_by_calibration'] and a['calibration_error'] <= 1e-5
    assert not b['chosen_by_calibration'] and not b['enabled'] and b['calibration_error'] > 1e-5
    assert gens[False].layer2_kernel(B, N) in (3, 4) and gens[True].layer2_kernel(B, N) == 1
    x = torch.as_tensor(np.random.RandomState(3).randn(B, 4, N, N).astype(np.float32)).cuda()
    y = gens[True].cnn_forward(x).cpu().numpy()
    gens[True].set_option('precision', 0)
    y0 = gens[True].cnn_forward(x).cpu().numpy()
    assert y.shape == (B, 2, N, N) and np.abs(y - y0).max() < GEN_TOL * np.abs(y0).max()
    assert gens[True].range_ok() is None
    for g in gens.values():
        g.close()


# ---- facade ---------------------------------------------------------------------------------------------------------------
def test_cgan_regression_div_from_a_folder(tmp_path, reg):
    """CGANRegression(div=True) from a reference-layout folder, through load_parameterization: predict_snapshot,
    predict_mean_snapshot(seed=...) and run_simulation agree with the Generator-level results"""
    from test_div_cpu import write_cgan_folder
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    from pyqg_generative_amd.qgmodel import WeightedParameterization
    folder = write_cgan_folder(tmp_path, R.flux_net_dict('gan'), R.flux_net_dict('ols'))
    p = load_parameterization(folder, model_weight=1.0)
    assert isinstance(p, WeightedParameterization) and isinstance(p.param, CGANRegression)
    model = p.param
    assert model.div is True and model.regression == 'full_loss'
    N = 64
    d = R.fixture()

    class _M:
        pass
    m = _M()
    m.q = d[f'q{N}'][0].astype('float64')
    z = R.latent_noise(N, d[f'q{N}'].shape[0])[:1]
    S = model.predict_snapshot(m, z)
    S_ref = d[f'S_{N}'][0].astype('float64')
    assert S.shape == (2, N, N)
    assert (np.abs(S - S_ref) / np.abs(S_ref).max(axis=(1, 2), keepdims=True)).max() < GEN_TOL
    # the bound nets apply the head: G and net_mean return (B, 2, N, N) divergences
    x = torch.as_tensor(R.inputs('gan', N)[:1]).cuda()
    assert _rel(model.G(x).cpu().numpy(), R.y32('gan', N)[:1]) < GEN_TOL
    assert _rel(model.net_mean(x[:, :2].contiguous()).cpu().numpy(), R.y32('ols', N)[:1]) < GEN_TOL
    # predict_mean_snapshot(seed): realisation j on the Philox stream (seed, counter j) — the Generator-level pieces
    M = 4
    Sm = model.predict_mean_snapshot(m, M=M, seed=9)
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    X = (d[f'q{N}'][:1] / R.scales()[0].reshape(1, 2, 1, 1))
    zz = torch.empty((M, 2, N, N), dtype=torch.float32, device='cuda')
    check(lib.qgx_noise_normal(_ptr(zz), 0, M, 2 * N * N, 9, 0, 0, 0.0, 1.0, _stream()))
    xx = torch.cat([torch.as_tensor(np.tile(X, (M, 1, 1, 1))).cuda(), zz], dim=1).contiguous()
    Y = reg.cnn_forward(xx).to(torch.float64).mean(0, keepdim=True).cpu().numpy().astype('float32')
    Y = Y + reg.cnn_forward(torch.as_tensor(np.ascontiguousarray(X)).cuda(), inet=1).cpu().numpy()
    ref = (Y * R.scales()[1].reshape(1, 2, 1, 1)).squeeze().astype('float64')
    assert _rel(Sm, ref) < 1e-6
    assert np.abs(Sm.mean(axis=(-2, -1))).max() < 1e-6 * np.abs(Sm).max()
    # offline: predict's layout, and every Monte-Carlo field integrates to zero
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    qv = d[f'q{N}'][:1].astype('float64').reshape(1, 1, 2, N, N)
    out = model.predict(xr.Dataset({'q': (['run', 'time', 'lev', 'y', 'x'], qv)}), M=3)
    for name in ('q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var'):
        assert out[name].shape == qv.shape
    for name in ('q_forcing_advection', 'q_forcing_advection_mean'):
        v = np.asarray(out[name].values)
        assert np.abs(v.mean(axis=(-2, -1))).max() < 1e-6 * np.abs(v).max()
    # online: the fused device path
    nsteps = 4
    q0 = _eddy_like_q(np.random.RandomState(2), 1, N)[0]
    params = EDDY_PARAMS.nx(N)._update({'tmax': 14400. * nsteps, 'log_level': 0})
    ds = run_simulation(dict(params), parameterization=dict(self=model, sampling='AR1', nsteps=1), q_init=q0,
                        sampling_freq=14400. * nsteps)
    q = np.asarray(ds['q'].values)
    assert q.shape[-3:] == (2, N, N) and np.isfinite(q).all()
    assert np.abs(q[-1] - q0).max() > 0
