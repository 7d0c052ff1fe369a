"""CPU: ANNModel, the pointwise stencil-ANN parameterization — fixture and restatement, state-dict mapping, the folder
layout (net.pt, scale.json, model_args.json), load_parameterization's dispatch, and what the C ABI refuses before any
device work (no GPU needed)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden


def _state_dict(net):
    sd = {}
    for l in range(len(net['w'])):
        sd[f'layers.{2 * l}.weight'] = torch.as_tensor(net['w'][l])
        sd[f'layers.{2 * l}.bias'] = torch.as_tensor(net['b'][l])
    return sd


def _write_folder(path, tag='a', args=None, scale=True):
    """a reference-layout ANNModel folder (ann_model.py:54-66): net.pt, scale.json, model_args.json"""
    from ann_restatement import net_from_fixture
    d = golden('ann.npz')
    net = net_from_fixture(d, tag)
    torch.save(_state_dict(net), os.path.join(path, 'net.pt'))
    if scale:
        with open(os.path.join(path, 'scale.json'), 'w') as f:
            json.dump({'x_scale': float(d['x_scale']), 'y_scale': float(d['y_scale'])}, f)
    if args is None:
        args = dict(model='ANNModel', stencil_size=net['stencil_size'], hidden_channels=net['hidden'],
                    scale_invariant=net['scale_invariant'])
    with open(os.path.join(path, 'model_args.json'), 'w') as f:
        json.dump(args, f)
    return str(path)


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_restatement_matches_reference_golden(tag):
    from ann_restatement import ANNRef
    d = golden('ann.npz')
    ref = ANNRef.from_fixture(tag)
    assert ref.generate_latent_noise(32, 32) == 0
    fields = [(f'q{N}', f'S{tag}{N}') for N in (32, 48, 64, 96, 128)]
    if tag == 'b':
        fields.append(('qz32', 'Sbz32'))
    for qk, sk in fields:
        q, S = d[qk].astype('float64'), d[sk].astype('float64')
        out = ref.predict_snapshot(q, 0)
        assert out.shape == q.shape and out.dtype == np.float64
        np.testing.assert_array_equal(np.isnan(out), np.isnan(S))
        fin = ~np.isnan(S)
        assert np.abs(out[fin] - S[fin]).max() <= 2e-6 * np.abs(S[fin]).max(), (tag, sk)
    if tag == 'b':          # the zero lower layer: every stencil there has norm 0, torch gives 0/0 = NaN
        S = d['Sbz32']
        assert np.isnan(S[1]).all() and np.isfinite(S[0]).all()


def test_state_dict_mapping_and_shape_refusals():
    from pyqg_generative_amd import weights
    from ann_restatement import net_from_fixture
    net = net_from_fixture(golden('ann.npz'), 'c')
    sd = _state_dict(net)
    m = weights.ann_from_state_dict(sd, 5, [32, 16, 8], False)
    assert m['stencil_size'] == 5 and m['hidden'] == [32, 16, 8] and not m['scale_invariant']
    assert [w.shape for w in m['w']] == [(32, 25), (16, 32), (8, 16), (1, 8)]
    for a, b in zip(m['w'] + m['b'], net['w'] + net['b']):
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
    for args in [(3, [32, 16, 8]), (5, [32, 16]), (5, [32, 16, 9]), (7, [32, 16, 8])]:
        with pytest.raises(ValueError):
            weights.ann_from_state_dict(sd, *args)
    bad = dict(sd)
    bad['layers.0.weight'] = torch.zeros(32, 24)
    with pytest.raises(ValueError, match='shape'):
        weights.ann_from_state_dict(bad, 5, [32, 16, 8])
    assert weights.is_ann_state_dict(sd) and not weights.is_ann_state_dict({'conv.0.weight': 0})
    syn = weights.synthetic_ann(7, [128, 64, 32, 1], True, seed=3)
    assert [w.shape for w in syn['w']] == [(128, 49), (64, 128), (32, 64), (1, 32), (1, 1)]


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_folder_round_trip(tmp_path, tag):
    """scale.json and model_args.json as the reference writes them (ann_model.py:61-66) come back through load_folder"""
    from pyqg_generative_amd import weights
    from ann_restatement import net_from_fixture
    d = golden('ann.npz')
    folder = _write_folder(tmp_path, tag)
    nets, xs, ys = weights.load_folder(folder, 'ann')
    assert (xs, ys) == (float(d['x_scale']), float(d['y_scale']))
    assert isinstance(xs, float) and isinstance(ys, float)
    want = net_from_fixture(d, tag)
    assert len(nets) == 1
    for k in ('stencil_size', 'hidden', 'scale_invariant'):
        assert nets[0][k] == want[k]
    for a, b in zip(nets[0]['w'] + nets[0]['b'], want['w'] + want['b']):
        np.testing.assert_array_equal(a, b)
    with open(os.path.join(folder, 'model_args.json')) as f:
        args = json.load(f)
    assert args['model'] == 'ANNModel' and args['stencil_size'] == want['stencil_size']


def test_model_class_refusals_before_device_work(tmp_path):
    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.tools.simulate import load_parameterization
    with pytest.raises(FileNotFoundError, match='net.pt'):
        ANNModel(folder=str(tmp_path))
    with pytest.raises(NotImplementedError, match='read=False'):
        ANNModel(folder=str(tmp_path), read=False)
    with pytest.raises(NotImplementedError, match='training'):
        ANNModel.__new__(ANNModel).fit(None, None)
    folder = tmp_path / 'c'
    folder.mkdir()
    _write_folder(folder, 'c')
    with pytest.raises(ValueError, match='ANN'):          # the folder's net is not what the arguments describe
        ANNModel(folder=str(folder))
    folder = tmp_path / 'args'
    folder.mkdir()
    _write_folder(folder, 'c', args=dict(model='ANNModel', stencil_size=3, hidden_channels=[32, 16, 8]))
    with pytest.raises(ValueError, match='ANN'):
        load_parameterization(str(folder), model_weight=0.5)


def test_gen_kind_ann_matches_header():
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.engine import Generator
    text = open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    enum = re.search(r'enum\s+qgx_gen_kind_ann\s*\{([^}]*)\}', text).group(1)
    assert dict(re.findall(r'(QGX_GEN_\w+)\s*=\s*(\d+)', enum)) == {'QGX_GEN_ANN': '4'}
    assert _lib.GEN_ANN == 4 and Generator.KINDS['ann'] == 4
    assert C.sizeof(_lib.qgx_ann_weights) == 7 * 4 + 4 + 10 * 8
    assert 'qgx_generator_create_ann' in {name for name, _, _ in _lib.SYMBOLS}


def _weights_struct(s=3, hidden=(24, 24), keep=None):
    from pyqg_generative_amd import _lib
    a = _lib.qgx_ann_weights()
    a.stencil_size, a.n_hidden = s, len(hidden)
    widths = [s * s] + list(hidden) + [1]
    for l, h in enumerate(hidden[:4]):
        a.hidden[l] = h
    for l in range(min(len(widths) - 1, 5)):
        w = np.zeros((max(widths[l + 1], 1), max(widths[l], 1)), np.float32)
        b = np.zeros(max(widths[l + 1], 1), np.float32)
        keep += [w, b]
        a.w[l], a.b[l] = w.ctypes.data, b.ctypes.data
    return a


@pytest.mark.parametrize('s,hidden,what', [(2, (24, 24), b'stencil_size'), (9, (24, 24), b'stencil_size'),
                                           (-1, (24, 24), b'stencil_size'), (3, (), b'hidden layers'),
                                           (3, (8, 8, 8, 8, 8), b'hidden layers'), (3, (24, 129), b'width'),
                                           (3, (0, 24), b'width')])
def test_abi_refuses_bad_shapes_before_any_device_call(s, hidden, what):
    """qgx_generator_create_ann checks stencil, depth and widths before the device is touched (so this runs without one);
    qgx_generator_create keeps refusing the ANN kind"""
    from pyqg_generative_amd import _lib
    keep = []
    a = _weights_struct(s, hidden, keep)
    if len(hidden) > 4:
        a.n_hidden = len(hidden)
    h = C.c_void_p(0)
    rc = _lib.lib.qgx_generator_create_ann(C.byref(a), 1.0, 1.0, 0, C.byref(h))
    assert rc == -1 and not h.value          # QGX_ERR_INVALID, no handle
    assert what in _lib.lib.qgx_last_error()
    nets = (_lib.qgx_cnn_weights * 1)()
    xs = (C.c_float * 2)(1.0, 1.0)
    assert _lib.lib.qgx_generator_create(_lib.GEN_ANN, nets, 1, xs, xs, 0, C.byref(h)) == -1 and not h.value
    assert b'kind' in _lib.lib.qgx_last_error()
