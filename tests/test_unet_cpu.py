"""CPU: the DeepInversion U-Net generator's weight recipe, loader and C ABI (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden


@pytest.fixture(scope='module')
def net():
    from pyqg_generative_amd import weights
    return weights.synthetic_unet()


def test_recipe_reproduces_the_golden_checksum(net):
    from pyqg_generative_amd import weights
    assert weights.unet_checksum(net) == str(golden('unet.npz')['weights_checksum'])
    assert sum(v.size for k, v in net.items() if 'running' not in k) == 13129954     # parameters of DeepInversionGenerator(4, 2)


def test_restatement_matches_reference_forward(net):
    import unet_restatement as U
    d = golden('unet.npz')
    sd = U.to_torch(net)
    for N in (32, 48, 64, 96, 128):
        keep = {}
        y = U.forward(sd, torch.as_tensor(d[f'x{N}']), keep).numpy()
        ref = d[f'y{N}']
        assert np.abs(y - ref).max() <= 2e-6 * np.abs(ref).max(), N
        if N == 64:
            b = keep['bottleneck'].numpy()
            assert np.abs(b - d['bottleneck64']).max() <= 2e-6 * np.abs(d['bottleneck64']).max()


def test_restatement_needs_the_in_place_rule(net):
    """the skip of the bn='None' units sees LeakyReLU(x): with the raw x the output moves by O(1) of max|y|"""
    import unet_restatement as U
    import torch.nn.functional as F
    d = golden('unet.npz')
    sd = U.to_torch(net)
    orig = U._res

    def raw_skip(x, sd_, p, bn):
        if bn:
            return orig(x, sd_, p, bn)
        a = U._conv3(F.leaky_relu(x, 0.2), sd_[p + '.conv.1.weight'], sd_[p + '.conv.1.bias'])
        a = U._conv3(F.leaky_relu(a, 0.2), sd_[p + '.conv.4.weight'], sd_[p + '.conv.4.bias'])
        return a + F.conv2d(x, sd_[p + '.conv1.weight'], sd_[p + '.conv1.bias'])
    U._res = raw_skip
    try:
        y = U.forward(sd, torch.as_tensor(d['x32'])).numpy()
    finally:
        U._res = orig
    assert np.abs(y - d['y32']).max() > 1e-2 * np.abs(d['y32']).max()


def test_state_dict_loader(net):
    from pyqg_generative_amd import weights
    sd = {k: torch.as_tensor(v) for k, v in net.items()}
    sd['down64.conv.1.bn.num_batches_tracked'] = torch.tensor(5)        # ignored
    out = weights.unet_from_state_dict(sd)
    assert weights.is_unet(out) and set(out) == set(net)
    for k in net:
        np.testing.assert_array_equal(out[k], net[k])
    missing = dict(sd)
    del missing['res512.conv.2.running_var']
    with pytest.raises(KeyError):
        weights.unet_from_state_dict(missing)
    extra = dict(sd)
    extra['res512.conv.5.weight'] = torch.zeros(1)
    with pytest.raises(KeyError):
        weights.unet_from_state_dict(extra)


def test_header_declares_and_library_exports_create_unet():
    from pyqg_generative_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'qgx.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+qgx_generator_create_unet\s*\(', text)
    assert 'qgx_generator_create_unet' in {name for name, _, _ in _lib.SYMBOLS}
    assert ctypes.CDLL(_lib.LIB_PATH).qgx_generator_create_unet is not None


def test_unet_struct_sizes_match_header():
    from pyqg_generative_amd import _lib
    assert ctypes.sizeof(_lib.qgx_unet_res) == 14 * 8
    # conv32 (2 pointers), 11 units, up_w / up_b (8), conv_end (2), bn_eps + padding
    assert ctypes.sizeof(_lib.qgx_unet_weights) == 2 * 8 + 11 * 14 * 8 + 8 * 8 + 2 * 8 + 8
