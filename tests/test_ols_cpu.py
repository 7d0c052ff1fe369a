"""CPU: OLSModel, the deterministic CNN parameterization — fixture, restatement, folder loader, model_args.json dispatch,
the C ABI's kind and what is refused before any device work (no GPU needed)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

HIDDEN = [128, 64, 32, 32, 32, 32, 32]


def _gz_net():
    from pyqg_generative_amd import weights
    return weights.net_from_npz(golden('weights_gz.npz'), 'net0_')


def _write_folder(path, args=None):
    """a reference-layout OLSModel folder (ols_model.py:50-56): net.pt, x_scale.json, y_scale.json, model_args.json"""
    net = _gz_net()
    sd = {}
    for i in range(8):
        sd[f'conv.{3 * i}.weight'] = torch.as_tensor(net['conv_w'][i])
        sd[f'conv.{3 * i}.bias'] = torch.as_tensor(net['conv_b'][i])
        if i < 7:
            for key, name in (('bn_g', 'weight'), ('bn_b', 'bias'), ('bn_m', 'running_mean'), ('bn_v', 'running_var')):
                sd[f'conv.{3 * i + 2}.{name}'] = torch.as_tensor(net[key][i])
            sd[f'conv.{3 * i + 2}.num_batches_tracked'] = torch.tensor(3)
    torch.save(sd, os.path.join(path, 'net.pt'))
    d = golden('weights_gz.npz')
    for name, key in (('x_scale.json', 'x_std'), ('y_scale.json', 'y_std')):
        std = np.asarray(d[key], np.float32).reshape(1, 2, 1, 1)
        with open(os.path.join(path, name), 'w') as f:
            json.dump(dict(mean=str((0 * std).tolist()), std=str(std.tolist())), f)
    args = args if args is not None else dict(model='OLSModel', div=False, batch_norm=True, bias=True,
                                              final_activation='None', hidden_channels=HIDDEN)
    with open(os.path.join(path, 'model_args.json'), 'w') as f:
        json.dump(args, f)
    return str(path)


def test_fixture_matches_restatement_and_checksum():
    from pyqg_generative_amd import weights
    from ols_restatement import OLSRef
    d = golden('ols.npz')
    assert str(d['weights_checksum']) == weights.net_checksum(_gz_net())
    ref = OLSRef.from_fixture()
    np.testing.assert_array_equal(ref.x_scale.std.reshape(-1), d['x_std'])
    np.testing.assert_array_equal(ref.y_scale.std.reshape(-1), d['y_std'])
    for N in (48, 64, 96):
        q, S = d[f'q{N}'].astype('float64'), d[f'S{N}'].astype('float64')
        assert q.shape[1:] == (2, N, N) and q.shape[0] >= 2
        for t in range(q.shape[0]):
            out = ref.predict_snapshot(q[t], 0)
            assert out.shape == (2, N, N) and out.dtype == np.float64
            assert np.abs(out - S[t]).max() <= 2e-6 * np.abs(S[t]).max(), (N, t)
        assert ref.generate_latent_noise(N, N) == 0


def test_load_folder_reads_the_reference_layout(tmp_path):
    from pyqg_generative_amd import weights
    nets, xs, ys = weights.load_folder(_write_folder(tmp_path), 'ols')
    assert len(nets) == 1 and nets[0]['conv_w'][0].shape == (128, 2, 5, 5) and nets[0]['conv_w'][7].shape == (2, 32, 3, 3)
    assert weights.net_checksum(nets[0]) == str(golden('ols.npz')['weights_checksum'])
    d = golden('weights_gz.npz')
    np.testing.assert_array_equal(xs, d['x_std'])
    np.testing.assert_array_equal(ys, d['y_std'])
    syn, sxs, sys_ = weights.synthetic('ols', seed=1)
    assert len(syn) == 1 and syn[0]['conv_w'][0].shape == (128, 2, 5, 5)


def test_model_args_dispatch(tmp_path):
    """simulate.py:238-242: the class named in model_args.json is built with the remaining arguments; the dispatch reaches
    the class (its configuration checks run before any device work), names without a device path are refused"""
    from pyqg_generative_amd.tools.simulate import load_parameterization
    for i, (args, exc, text) in enumerate([
            (dict(model='OLSModel', div=True), NotImplementedError, 'div=False'),
            (dict(model='OLSModel', hidden_channels=[64, 32]), NotImplementedError, 'div=False'),
            (dict(model='MeanVarModel', hidden_channels=[64, 32]), NotImplementedError, 'channel'),
            (dict(model='CGANRegression', generator='Other'), NotImplementedError, 'generator'),
            (dict(model='CVAERegression', div=True), NotImplementedError, 'div=False'),
            (dict(model='ANNModel'), NotImplementedError, 'ANNModel'),
            (dict(model='BackscatterBiharmonic'), NotImplementedError, 'BackscatterBiharmonic')]):
        folder = tmp_path / str(i)
        folder.mkdir()
        _write_folder(folder, args)
        with pytest.raises(exc, match=text):
            load_parameterization(str(folder), model_weight=0.5)


@pytest.mark.parametrize('kw', [dict(div=True), dict(batch_norm=False), dict(bias=False), dict(final_activation='softplus'),
                                dict(hidden_channels=[128, 64, 32, 32, 32, 32])])
def test_unsupported_configurations_are_refused_before_device_work(tmp_path, kw):
    from pyqg_generative_amd.models import OLSModel
    with pytest.raises(NotImplementedError):
        OLSModel(folder=_write_folder(tmp_path), **kw)


def test_folder_without_a_trained_net_is_refused(tmp_path):
    from pyqg_generative_amd.models import OLSModel
    with pytest.raises(FileNotFoundError, match='net.pt'):
        OLSModel(folder=str(tmp_path))


def test_gen_kind_matches_header():
    from pyqg_generative_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    enum = re.search(r'enum\s+qgx_gen_kind\s*\{([^}]*)\}', text).group(1)
    kinds = {k: int(v) for k, v in re.findall(r'(QGX_GEN_\w+)\s*=\s*(\d+)', enum)}
    assert kinds == {'QGX_GEN_GAN': _lib.GEN_GAN, 'QGX_GEN_VAE': _lib.GEN_VAE, 'QGX_GEN_GZ': _lib.GEN_GZ,
                     'QGX_GEN_OLS': _lib.GEN_OLS}
    assert _lib.GEN_OLS == 3
    from pyqg_generative_amd.engine import Generator
    assert Generator.KINDS['ols'] == _lib.GEN_OLS


@pytest.mark.parametrize('n_nets,n_in', [(2, 2), (1, 4), (0, 2)])
def test_abi_refuses_other_shapes_before_any_allocation(n_nets, n_in):
    """qgx_generator_create(QGX_GEN_OLS, ...) takes exactly one AndrewCNN(2, 2); the shapes are checked before the device is
    touched (so this runs without one)"""
    from pyqg_generative_amd import _lib
    nets = (_lib.qgx_cnn_weights * 2)()
    for w in nets:
        w.n_in, w.n_out = n_in, 2
    xs = (C.c_float * 2)(1.0, 1.0)
    h = C.c_void_p(0)
    rc = _lib.lib.qgx_generator_create(_lib.GEN_OLS, nets, n_nets, xs, xs, 0, C.byref(h))
    assert rc == -1 and not h.value          # QGX_ERR_INVALID, no handle
    assert b'net' in _lib.lib.qgx_last_error()
