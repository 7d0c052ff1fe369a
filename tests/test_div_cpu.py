"""CPU: flux-form nets, AndrewCNN(div=True) — the fixture against the restatement, the two forms of the divergence, the fixture's
sensitivity to the Nyquist rule, the loaders and what the C ABI refuses before any device work (no GPU needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden

import div_restatement as R

GAN_SIZES = (16, 48, 64, 96, 128)
OLS_SIZES = (16, 64)
CASES = [('gan', N) for N in GAN_SIZES] + [('ols', N) for N in OLS_SIZES]


@pytest.fixture(scope='module')
def fluxes64():
    """the float64 fluxes of every fixture case, computed once"""
    from oracle.gen_ref import cnn_forward
    torch.set_num_threads(4)
    return {(kind, N): cnn_forward(R.flux_net_ref(kind), R.inputs(kind, N), dtype='float64') for kind, N in CASES}


def test_fixture_is_small_and_complete():
    path = os.path.join(R.GOLDEN, 'generator_div.npz')
    assert os.path.getsize(path) < 1 << 20
    d = R.fixture()
    for kind, N in CASES:
        T = d[f'{kind}_y32_{N}'].shape[0]
        assert d[f'{kind}_y32_{N}'].shape == (T, 2, N, N) and d[f'{kind}_y32_{N}'].dtype == np.float32
        assert d[f'{kind}_d16_{N}'].shape == (T, 2, N, N)
        assert R.inputs(kind, N).shape == (T, 4 if kind == 'gan' else 2, N, N)
        # the reference's own float32 error against its float64 forward, as recorded: the float32 class
        e = np.abs(R.y32(kind, N) - R.y64(kind, N)).max() / np.abs(R.y64(kind, N)).max()
        assert abs(e - R.e_ref(kind, N)) < 1e-9 and 1e-7 < e < 4e-6, (kind, N, e)
    assert d['gan_last_w'].shape == (4, 32, 3, 3) and d['ols_last_w'].shape == (4, 32, 3, 3)


@pytest.mark.parametrize('kind,N', CASES)
def test_two_forms_of_the_divergence_agree(fluxes64, kind, N):
    """irfftn(ik rfftn(fx) + il rfftn(fy)) = ifft2(Hx fft2(fx1 + i fx2) + Hy fft2(fy1 + i fy2)) with the Hermitian multipliers
    of the restatement, to 1e-12 in float64; and both are the fixture's y64"""
    F = fluxes64[kind, N]
    a, b = 10000. * R.divergence_rfftn(F, 'float64'), 10000. * R.divergence_plane(F)
    m = np.abs(a).max()
    assert np.abs(a - b).max() <= 1e-12 * m
    # y64 is stored as y32 + a float16-coded difference: 2^-11 of 1e-6
    assert np.abs(a - R.y64(kind, N)).max() <= 2e-9 * m
    # the flux form's point: the output integrates to zero without any de-mean
    assert np.abs(a.mean(axis=(-2, -1))).max() <= 1e-15 * m


@pytest.mark.parametrize('kind,N', CASES)
def test_fixture_sees_the_nyquist_rule(fluxes64, kind, N):
    """CNN output is not band-limited: the two plausible wrong rules for the Nyquist row are off by more than 1e-2"""
    F, y64 = fluxes64[kind, N], R.y64(kind, N)
    m = np.abs(y64).max()
    for rule in ('naive_row', 'zero_row'):
        assert np.abs(10000. * R.divergence_plane(F, rule) - y64).max() > 1e-2 * m, rule


@pytest.mark.parametrize('kind,N', CASES)
def test_restatement_matches_the_reference(kind, N):
    """torch float32 restatement (circular conv2d, eval BatchNorm, rfftn divergence) against the reference's y32: float32 class
    (the summation order of another torch build may differ; the bound is the one test_ols_cpu.py holds its restatement to)"""
    y = R.flux_forward(R.flux_net_ref(kind), R.inputs(kind, N))
    assert y.dtype == np.float32
    assert np.abs(y - R.y32(kind, N)).max() <= 2e-6 * np.abs(R.y32(kind, N)).max()


def test_predict_snapshot_restatement():
    """CGANRegression(regression='full_loss', div=True).predict_snapshot: both nets flux-form, summed in float32"""
    xs, ys = R.scales()
    ref = R.FluxGeneratorRef('gan', [R.flux_net_ref('gan'), R.flux_net_ref('ols')], xs, ys)
    for N in OLS_SIZES:
        S = R.fixture()[f'S_{N}'].astype('float64')
        z = R.latent_noise(N, R.fixture()[f'q{N}'].shape[0])
        for t in range(S.shape[0]):
            out = ref.predict_snapshot(R.fixture()[f'q{N}'][t].astype('float64'), z[t:t + 1])
            sc = np.abs(S[t]).max(axis=(1, 2), keepdims=True)
            assert (np.abs(out - S[t]) / sc).max() <= 2e-6, (N, t)


# ---- loaders and facade ----------------------------------------------------------------------------------------------------
def _state_dict(net):
    sd = {}
    for i in range(8):
        sd[f'conv.{3 * i}.weight'] = torch.as_tensor(net['conv_w'][i])
        sd[f'conv.{3 * i}.bias'] = torch.as_tensor(net['conv_b'][i])
        if i < 7:
            for key, name in (('bn_g', 'weight'), ('bn_b', 'bias'), ('bn_m', 'running_mean'), ('bn_v', 'running_var')):
                sd[f'conv.{3 * i + 2}.{name}'] = torch.as_tensor(net[key][i])
            sd[f'conv.{3 * i + 2}.num_batches_tracked'] = torch.tensor(3)
    return sd


def write_cgan_folder(path, G, net_mean=None, **args):
    """a reference-layout CGANRegression folder (cgan_regression.py:98-107)"""
    torch.save(_state_dict(G), os.path.join(path, 'G.pt'))
    if net_mean is not None:
        torch.save(_state_dict(net_mean), os.path.join(path, 'net_mean.pt'))
    xs, ys = R.scales()
    for name, std in (('x_scale.json', xs), ('y_scale.json', ys)):
        std = std.reshape(1, 2, 1, 1)
        with open(os.path.join(path, name), 'w') as f:
            json.dump(dict(mean=str((0 * std).tolist()), std=str(std.tolist())), f)
    full = dict(model='CGANRegression', regression='None' if net_mean is None else 'full_loss', nx=64, generator='Andrew',
                div=True, hidden_channels=[128, 64, 32, 32, 32, 32, 32])
    full.update(args)
    with open(os.path.join(path, 'model_args.json'), 'w') as f:
        json.dump(full, f)
    return str(path)


def _plain_gan():
    from pyqg_generative_amd import weights
    return weights.net_from_npz(golden('weights_gan.npz'), 'net0_')


def test_load_folder_checks_the_last_layer_against_the_flag(tmp_path):
    from pyqg_generative_amd import weights
    a, b = tmp_path / 'flux', tmp_path / 'plain'
    a.mkdir(); b.mkdir()
    write_cgan_folder(a, R.flux_net_dict('gan'), R.flux_net_dict('ols'))
    write_cgan_folder(b, _plain_gan(), div=False)
    nets, xs, ys = weights.load_folder(str(a), 'gan', regression=True, div=True)
    assert [n['conv_w'][7].shape for n in nets] == [(4, 32, 3, 3)] * 2 and all(weights.is_flux_form(n) for n in nets)
    np.testing.assert_array_equal(xs, R.scales()[0])
    with pytest.raises(ValueError, match='div=False'):
        weights.load_folder(str(a), 'gan', regression=True)
    with pytest.raises(ValueError, match='div=True'):
        weights.load_folder(str(b), 'gan', div=True)
    assert not weights.is_flux_form(weights.load_folder(str(b), 'gan')[0][0])


def test_synthetic_flux_form():
    from pyqg_generative_amd import weights
    nets, _, _ = weights.synthetic('gan', seed=3, regression=True, div=True)
    assert [n['conv_w'][7].shape for n in nets] == [(4, 32, 3, 3)] * 2 and nets[0]['conv_b'][7].shape == (4,)
    plain, _, _ = weights.synthetic('gan', seed=3)
    flux, _, _ = weights.synthetic('gan', seed=3, div=True)
    for i in range(7):
        np.testing.assert_array_equal(plain[0]['conv_w'][i], flux[0]['conv_w'][i])
    assert weights.synthetic('ols', div=True)[0][0]['conv_w'][7].shape == (4, 32, 3, 3)
    with pytest.raises(ValueError):
        weights.synthetic('gz', div=True)


def test_cgan_folder_with_div_reaches_the_device(tmp_path):
    """load_parameterization on a CGANRegression folder whose model_args.json says div=True: no NotImplementedError any more —
    the class is built; without a GPU the first device call is what fails (QgxError), with one the model loads"""
    from pyqg_generative_amd.tools.simulate import load_parameterization
    from pyqg_generative_amd._lib import QgxError
    folder = write_cgan_folder(tmp_path, R.flux_net_dict('gan'))
    try:
        p = load_parameterization(folder)
    except QgxError as e:
        assert 'hip' in str(e).lower() or 'device' in str(e).lower(), e
    else:
        assert p is not None


def test_cgan_folder_whose_last_layer_contradicts_the_flag_is_refused(tmp_path):
    from pyqg_generative_amd.tools.simulate import load_parameterization
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir(); b.mkdir()
    with pytest.raises(ValueError, match='div=True'):          # flag set, two-channel G
        load_parameterization(write_cgan_folder(a, _plain_gan()))
    with pytest.raises(ValueError, match='div=False'):         # flux-form G, flag not set
        load_parameterization(write_cgan_folder(b, R.flux_net_dict('gan'), div=False))


# ---- C ABI, before any device work ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n_nets,n_out', [('GEN_GAN', 1, [3]), ('GEN_GAN', 2, [4, 3]), ('GEN_OLS', 1, [1]), ('GEN_VAE', 1, [6]),
                                              ('GEN_GZ', 2, [4, 2]), ('GEN_GZ', 2, [2, 4]), ('GEN_GZ', 2, [4, 4])])
def test_abi_refuses_other_channel_counts_before_any_allocation(kind, n_nets, n_out):
    """n_out is 2, or 4 for a flux-form net of a GAN / VAE / OLS handle (each net on its own); GZ takes 2 only.  Refused with
    QGX_ERR_INVALID before the device is touched (so this runs without one)"""
    from pyqg_generative_amd import _lib
    k = getattr(_lib, kind)
    nets = (_lib.qgx_cnn_weights * 2)()
    for n, w in enumerate(nets):
        w.n_in = 2 if (k in (_lib.GEN_GZ, _lib.GEN_OLS) or n == 1) else 4
        w.n_out = n_out[n] if n < len(n_out) else 2
    xs = (C.c_float * 2)(1.0, 1.0)
    h = C.c_void_p(0)
    rc = _lib.lib.qgx_generator_create(k, nets, n_nets, xs, xs, 0, C.byref(h))
    assert rc == -1 and not h.value
    assert b'n_out' in _lib.lib.qgx_last_error()


def test_abi_unet_handle_refuses_a_three_channel_net_mean():
    from pyqg_generative_amd import _lib
    u, mean = _lib.qgx_unet_weights(), _lib.qgx_cnn_weights()
    mean.n_in, mean.n_out = 2, 3
    xs = (C.c_float * 2)(1.0, 1.0)
    h = C.c_void_p(0)
    rc = _lib.lib.qgx_generator_create_unet(C.byref(u), C.byref(mean), xs, xs, 0, C.byref(h))
    assert rc == -1 and not h.value and b'net_mean' in _lib.lib.qgx_last_error()
