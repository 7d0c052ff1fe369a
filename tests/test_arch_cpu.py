"""CPU: AndrewCNN nets of any hidden_channels — the fixture against the float64 restatement, the architecture-aware weight
reader, model folders with model_args.json, and what qgx_generator_create_arch refuses before any device call (no GPU needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import arch_restatement as AR

SHIPPED = [128, 64, 32, 32, 32, 32, 32]


@pytest.mark.parametrize('name,N', [(n, N) for n, c in AR.CASES.items() for N in c['sizes']])
def test_fixture_matches_the_float64_restatement(name, N):
    """the reference's float64 forward against plain numpy in float64 on the regenerated weights and noise; the fixture carries the
    reference's FLOAT32 forward exactly and the float64 one through a float16 difference, so the bound is set by the float32
    evaluation: max(4 e_ref, 2e-6) of max|y|"""
    from pyqg_generative_amd import weights
    net = AR.case_net(name)
    assert weights.net_checksum(net) == str(AR.fixture()[f'{name}_checksum'])
    x, want = AR.inputs(name, N), AR.y64(name, N)
    assert x.shape == (AR.CASES[name]['sizes'][N], AR.CASES[name]['n_in'], N, N)
    got = AR.forward(net, x)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f'\ncase {name} N={N}: restatement vs fixture float64 {err:.2e} (e_ref {AR.e_ref(name, N):.2e})')
    assert got.shape == want.shape == (x.shape[0], 2, N, N)
    assert err <= max(4 * AR.e_ref(name, N), 2e-6)
    if AR.CASES[name]['div']:
        assert np.abs(got.mean(axis=(-2, -1))).max() < 1e-9 * np.abs(got).max()


@pytest.mark.parametrize('name,N', [(n, N) for n, c in AR.EDGE_CASES.items() for N in c['sizes']])
def test_edge_truth_is_the_references_float64_forward(name, N):
    """the truth of the generic engine's edge cases (AR.edge_truth: plain numpy in float64 on seeded weights and inputs) against the
    reference's own AndrewCNN in float64 at 256 seeded positions of its output (generator_arch_edges.npz): two float64 evaluations
    of sums of at most 6400 terms, 1e-12 of max|y|"""
    from pyqg_generative_amd import weights
    d = AR.edge_fixture()
    net = AR.edge_net(name)
    assert weights.net_checksum(net) == str(d[f'{name}_checksum'])
    assert [w.shape[-1] for w in net['conv_w']] == AR.edge_kernels(name)
    got, want, ymax = AR.edge_truth(name, N), d[f'{name}_y_{N}'], float(d[f'{name}_ymax_{N}'])
    assert got.shape == (AR.EDGE_T, 2, N, N) and got.dtype == np.float64 and want.shape == (AR.EDGE_SAMPLES,)
    pos = AR.edge_positions(name, N)
    assert len(np.unique(pos // (N * N))) == 2 * AR.EDGE_T          # both members, both channels
    err = np.abs(got.reshape(-1)[pos] - want).max() / ymax
    print(f'\nedge case {name} N={N}: restatement vs the reference in float64 {err:.2e} (max|y| {ymax:.3g})')
    assert err < 1e-12
    assert abs(np.abs(got).max() / ymax - 1) < 1e-12
    if AR.EDGE_CASES[name]['div']:
        assert np.abs(got.mean(axis=(-2, -1))).max() < 1e-9 * ymax


# csrc/conv_generic.hip at the commit that retired the A/B-only conv kernels, restated: tiles_per_wg (l. 293), rows_generic
# (l. 299-309), launch_convg's choice of the instantiation (l. 331-341) and cnn_pack_net_arch's padding (l. 255-256)
def _tiles_per_wg(ntf):
    return 2 if ntf % 2 == 0 else 1


def _rows_generic(B, N, ny):
    cap = 256 if 256 % N == 0 else 384
    best = 0
    for R in range(1, N + 1):
        if N % R or (R * N) % 32:
            continue
        if R * N > cap:
            break
        best = R
    while best > 1 and best % 2 == 0 and ((best // 2) * N) % 32 == 0 and B * (N // best) * ny < 256:
        best //= 2
    return best


def _launches(name, N, B):
    """(N, R, M-tiles per wave, NT, ny, chunks of input channels as (full, rest)) of every convolution of the case"""
    from pyqg_generative_amd import weights
    c = AR.EDGE_CASES[name] if name in AR.EDGE_CASES else AR.CASES[name]
    ch = [c['n_in']] + list(c['hidden_channels']) + [4 if c['div'] else 2]
    ks = AR.edge_kernels(name) if name in AR.EDGE_CASES else weights.arch_kernels(c['hidden_channels'])
    out = []
    for l in range(len(ch) - 1):
        cinp = 8 if l == 0 else -(-ch[l] // 8) * 8
        ntf = -(-ch[l + 1] // 32)
        nt = _tiles_per_wg(ntf)
        R = _rows_generic(B, N, ntf // nt)
        out.append((N, R, 3 if R * N // 32 > 8 else 2, nt, ntf // nt, (cinp // 32, cinp % 32), ks[l]))
    return out


ALL_TILE_SHAPES = {16: [16, 8, 4, 2], 32: [8, 4, 2, 1], 48: [8, 4, 2], 64: [4, 2, 1], 96: [4, 2, 1], 128: [2, 1]}


def test_edge_cases_reach_every_launch_shape_of_the_generic_engine():
    """what tests/test_gpu_arch.py launches (AR.launch_table) against what the rule can give: all 19 (N, R) tile shapes, both M-tile
    counts per wave with both NT, every (NT, ny) of 1 ... 8 output tiles, the chunk counts, and a 5x5 layer over 256 channels"""
    # the rule's own range: every member count at every size gives one of the 19 shapes, and each is given by some count
    for N, Rs in ALL_TILE_SHAPES.items():
        assert {_rows_generic(B, N, 1) for B in range(1, 600)} == set(Rs), N
        for ny in (2, 3, 4, 5, 7):
            assert {_rows_generic(B, N, ny) for B in range(1, 600)} <= set(Rs), (N, ny)
    runs = [s for name, N, B in AR.launch_table() for s in _launches(name, N, B)]
    assert {(N, R) for N, R, *_ in runs} == {(N, R) for N, Rs in ALL_TILE_SHAPES.items() for R in Rs}
    assert len({(N, R) for N, R, *_ in runs}) == 19
    assert {(mt, nt) for _, _, mt, nt, *_ in runs} == {(2, 1), (2, 2), (3, 1), (3, 2)}
    assert {(nt, ny) for _, _, _, nt, ny, *_ in runs} == {(1, 1), (2, 1), (1, 3), (2, 2), (1, 5), (2, 3), (1, 7), (2, 4)}
    chunks = {ck for *_, ck, _ in runs}
    assert {(3, 0), (6, 0), (7, 0), (8, 0), (1, 8), (0, 8), (0, 16), (0, 24), (2, 0), (4, 0)} <= chunks
    assert (8, 0, 5) in {(ck[0], ck[1], ks) for *_, ck, ks in runs}          # 25 taps x 256 channels: K = 6400
    # the ladder of each (case, N) walks every R of that size, and the two below-threshold counts take the smaller tile
    for (name, N), Bs in AR.LADDER.items():
        if name != 'E':
            assert {_launches(name, N, B)[0][1] for B in Bs} == set(ALL_TILE_SHAPES[N]), (name, N)
            assert all(len({s[1] for s in _launches(name, N, B)}) == 1 for B in Bs)          # ny = 1 throughout: one R per launch
    assert _launches('I', 32, 63)[0][1] == 4 and _launches('I', 32, 64)[0][1] == 8
    assert _launches('I', 96, 10)[0][1] == 2 and _launches('I', 96, 11)[0][1] == 4
    # E at 16 x 16: its wide layers (ny = 4) and its last layer (ny = 1) change shape at different counts
    assert [tuple(s[1] for s in _launches('E', 16, B)) for B in AR.LADDER[('E', 16)]] == \
        [(2, 2, 2), (2, 2, 2), (4, 4, 2), (8, 8, 2), (16, 16, 4)]


def test_state_dict_key_layout_follows_the_flags():
    from pyqg_generative_amd import weights
    s = weights.arch_shapes(2, [24, 40, 12, 20], batch_norm=False, bias=False)
    assert list(s) == ['conv.0.weight', 'conv.2.weight', 'conv.4.weight', 'conv.6.weight', 'conv.8.weight']
    assert s['conv.0.weight'] == (24, 2, 5, 5) and s['conv.2.weight'] == (40, 24, 5, 5) and s['conv.4.weight'] == (12, 40, 3, 3)
    assert s['conv.8.weight'] == (2, 20, 3, 3)
    s = weights.arch_shapes(4, [48, 8, 8], div=True)
    assert s['conv.9.weight'] == (4, 8, 3, 3) and s['conv.9.bias'] == (4,) and s['conv.5.running_var'] == (8,)
    assert 'conv.11.weight' not in s and 'conv.2.weight' in s and s['conv.3.weight'] == (8, 48, 5, 5)
    s = weights.arch_shapes(2, [136], bias=False)
    assert set(s) == {'conv.0.weight', 'conv.3.weight'} | {f'conv.2.{k}' for k in ('weight', 'bias', 'running_mean', 'running_var')}
    assert s['conv.3.weight'] == (2, 136, 3, 3)
    # the default arguments are the layout net_from_state_dict reads
    s = weights.arch_shapes(2, SHIPPED)
    assert s['conv.21.weight'] == (2, 32, 3, 3) and s['conv.20.running_mean'] == (32,) and len(s) == 8 * 2 + 7 * 4


@pytest.mark.parametrize('name', list(AR.CASES))
def test_reader_round_trip_and_checksum(name):
    from pyqg_generative_amd import weights
    c = AR.CASES[name]
    net = AR.case_net(name)
    sd = {k: torch.as_tensor(v) for k, v in weights.state_dict_from_net(net).items()}
    if c['batch_norm']:
        sd['conv.2.num_batches_tracked'] = torch.tensor(3)          # ignored, as by the existing reader
    back = weights.net_from_state_dict_arch(sd, **{k: c[k] for k in AR.ARCH_KEYS})
    assert weights.net_checksum(back) == weights.net_checksum(net)
    assert len(back['conv_w']) == len(c['hidden_channels']) + 1
    assert (len(back['conv_b']) > 0) == c['bias'] and (len(back['bn_g']) > 0) == c['batch_norm']
    assert weights.is_flux_form(back) == c['div'] and not weights.is_shipped_arch(back)
    assert weights.net_arch(back) == {k: c[k] for k in AR.ARCH_KEYS}


def test_reader_refuses_what_the_constructor_arguments_do_not_describe():
    from pyqg_generative_amd import weights
    a = AR.CASES['A']
    sd = weights.state_dict_from_net(AR.case_net('A'))
    kw = {k: a[k] for k in AR.ARCH_KEYS}
    with pytest.raises(ValueError, match=r'conv\.3\.weight'):                      # other widths
        weights.net_from_state_dict_arch(sd, **dict(kw, hidden_channels=[64, 48, 16, 16, 16, 16, 16]))
    with pytest.raises(ValueError, match=r'conv\.\d+\.'):                          # fewer layers
        weights.net_from_state_dict_arch(sd, **dict(kw, hidden_channels=[64, 32, 16]))
    with pytest.raises(ValueError, match=r"unexpected key 'conv\.\d+\.bias'"):     # trained with bias
        weights.net_from_state_dict_arch(sd, **dict(kw, bias=False))
    with pytest.raises(ValueError, match='conv'):                                  # trained with BatchNorm
        weights.net_from_state_dict_arch(sd, **dict(kw, batch_norm=False))
    with pytest.raises(ValueError, match=r'conv\.21\.weight'):                     # two-channel last layer, div=True
        weights.net_from_state_dict_arch(sd, **dict(kw, div=True))
    d = AR.CASES['D']
    sdd = weights.state_dict_from_net(AR.case_net('D'))
    with pytest.raises(ValueError, match=r'conv\.9\.weight'):                      # flux-form last layer without div
        weights.net_from_state_dict_arch(sdd, **dict({k: d[k] for k in AR.ARCH_KEYS}, div=False))
    with pytest.raises(ValueError, match=r'conv\.0\.weight'):                      # n_in
        weights.net_from_state_dict_arch(sdd, **dict({k: d[k] for k in AR.ARCH_KEYS}, n_in=2))
    # the shipped state dict does not load under other widths, nor the other way round
    shipped = weights.state_dict_from_net(weights.synthetic('ols')[0][0])
    with pytest.raises(ValueError):
        weights.net_from_state_dict_arch(shipped, 2, [64, 32])
    for bad in ([], [8] * 8, [0, 8], [300], [16.5]):
        with pytest.raises(ValueError, match='hidden_channels'):
            weights.check_hidden_channels(bad)


def test_synthetic_arch_is_seeded_and_scaled():
    from pyqg_generative_amd import weights
    a, b = weights.synthetic_arch(2, [24, 40], seed=4), weights.synthetic_arch(2, [24, 40], seed=4)
    assert weights.net_checksum(a) == weights.net_checksum(b) != weights.net_checksum(weights.synthetic_arch(2, [24, 40], seed=5))
    assert [w.shape for w in a['conv_w']] == [(24, 2, 5, 5), (40, 24, 5, 5), (2, 40, 3, 3)]
    assert abs(a['conv_w'][1].std() / np.sqrt(2.0 / (24 * 25)) - 1) < 0.05          # He scale
    # the shipped widths draw the stream `synthetic` draws
    s = weights.synthetic_arch(2, SHIPPED, seed=0)
    assert weights.net_checksum(s) == weights.net_checksum(weights.synthetic('ols', seed=0)[0][0])
    assert weights.is_shipped_arch(s) and not weights.is_shipped_arch(weights.synthetic_arch(2, SHIPPED, bias=False))


def test_load_folder_takes_the_architecture_arguments(tmp_path):
    from pyqg_generative_amd import weights
    b, a = AR.CASES['B'], AR.CASES['A']
    fb, fa, fz = tmp_path / 'ols', tmp_path / 'vae', tmp_path / 'gz'
    for f in (fb, fa, fz):
        f.mkdir()
    AR.write_folder(fb, 'ols', [AR.case_net('B')])
    nets, xs, ys = weights.load_folder(str(fb), 'ols', hidden_channels=b['hidden_channels'], batch_norm=False, bias=False)
    assert weights.net_checksum(nets[0]) == str(AR.fixture()['B_checksum'])
    np.testing.assert_array_equal(xs, AR.scales()[0])
    with pytest.raises((ValueError, KeyError), match='conv'):      # the default arguments do not describe this folder (the
        weights.load_folder(str(fb), 'ols')                        # existing reader of the default architecture: a KeyError)
    with pytest.raises(ValueError, match='conv'):
        weights.load_folder(str(fb), 'ols', hidden_channels=b['hidden_channels'])
    # a VAE with a regression net: hidden_channels reaches the decoder alone, net_mean has the default widths
    mean = weights.synthetic('ols', seed=2)[0][0]
    AR.write_folder(fa, 'vae', [AR.case_net('A'), mean])
    nets, _, _ = weights.load_folder(str(fa), 'vae', regression=True, hidden_channels=a['hidden_channels'])
    assert weights.net_checksum(nets[0]) == str(AR.fixture()['A_checksum']) and weights.net_checksum(nets[1]) == weights.net_checksum(mean)
    assert not weights.is_shipped_arch(nets[0]) and weights.is_shipped_arch(nets[1])
    # GZ: both nets
    gz = [weights.synthetic_arch(2, [32, 16, 16], seed=s) for s in (1, 2)]
    AR.write_folder(fz, 'gz', gz)
    nets, _, _ = weights.load_folder(str(fz), 'gz', hidden_channels=[32, 16, 16])
    assert [weights.net_checksum(n) for n in nets] == [weights.net_checksum(n) for n in gz]


class _Recorder:
    """stands in for engine.Generator: records what the model class hands to the device"""
    made = []

    def __init__(self, kind, nets, x_std, y_std, device=0, **kw):
        self.kind, self.nets, self.device, self.n_nets = kind, nets, device, len(nets)
        _Recorder.made.append(self)


@pytest.fixture
def recorder(monkeypatch):
    from pyqg_generative_amd.models import parameterization
    _Recorder.made = []
    monkeypatch.setattr(parameterization, 'Generator', _Recorder)
    return _Recorder


def test_load_parameterization_passes_model_args_through(tmp_path, recorder):
    """model_args.json as save_model_args writes it (cnn_tools.py:21-25) for the four classes; the handle creation is replaced"""
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.simulate import load_parameterization
    from pyqg_generative_amd.models import OLSModel, CVAERegression, CGANRegression, MeanVarModel
    a, b, d = AR.CASES['A'], AR.CASES['B'], AR.CASES['D']
    mean = weights.synthetic('ols', seed=2)[0][0]
    gz = [weights.synthetic_arch(2, [32, 16, 16], seed=s) for s in (1, 2)]
    jobs = [
        ('ols', [AR.case_net('B')], dict(model='OLSModel', div=False, batch_norm=False, bias=False, final_activation='None',
                                         hidden_channels=b['hidden_channels']), OLSModel, ['B']),
        ('vae', [AR.case_net('A'), mean], dict(model='CVAERegression', regression='full_loss', decoder_var='adaptive', div=False,
                                               hidden_channels=a['hidden_channels']), CVAERegression, ['A', None]),
        ('gan', [AR.case_net('D')], dict(model='CGANRegression', regression='None', nx=64, generator='Andrew', div=True,
                                         hidden_channels=d['hidden_channels']), CGANRegression, ['D']),
        ('gz', gz, dict(model='MeanVarModel', hidden_channels=[32, 16, 16]), MeanVarModel, [None, None]),
    ]
    for i, (kind, nets, args, cls, cases) in enumerate(jobs):
        folder = tmp_path / str(i)
        folder.mkdir()
        p = load_parameterization(AR.write_folder(folder, kind, nets, args), model_weight=0.5, device=0)
        assert isinstance(p.param, cls) and p.param.hidden_channels == args['hidden_channels']
        g = recorder.made[-1]
        assert g.kind == kind and [weights.net_checksum(n) for n in g.nets] == [weights.net_checksum(n) for n in nets]
        for n, case in zip(g.nets, cases):
            if case is not None:
                assert weights.net_arch(n) == {k: AR.CASES[case][k] for k in AR.ARCH_KEYS}
    # shipped widths with div=True are no refusals any more (OLSModel, CVAERegression): the loader checks the form instead
    for kind, cls_name in (('ols', 'OLSModel'), ('vae', 'CVAERegression')):
        folder = tmp_path / f'div_{kind}'
        folder.mkdir()
        n_in = 2 if kind == 'ols' else 4
        flux = weights.synthetic_arch(n_in, SHIPPED, div=True, seed=6)
        p = load_parameterization(AR.write_folder(folder, kind, [flux], dict(model=cls_name, div=True)))
        assert p.param.div is True and weights.is_flux_form(recorder.made[-1].nets[0])


def test_a_folder_that_does_not_match_the_arguments_is_refused_either_way(tmp_path):
    """the model classes used to refuse every architecture argument with NotImplementedError; now the arguments reach the loader,
    which holds the folder's state dicts to them.  A mismatch is an ArchitectureMismatch — a ValueError (what the loaders raise) AND
    a NotImplementedError (what the classes raise for a configuration that does not run) — naming the key; a folder without the
    class's trained files is an UntrainedFolder (NotImplementedError: there is no training on the device)"""
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import OLSModel, MeanVarModel, CVAERegression
    folder = AR.write_folder(tmp_path, 'ols', [AR.case_net('B')])
    for exc in (ValueError, NotImplementedError, weights.ArchitectureMismatch):
        with pytest.raises(exc, match=r'conv\.\d+\.'):
            OLSModel(folder=folder, hidden_channels=[24, 40, 12, 20])          # trained without BatchNorm and bias
    with pytest.raises(weights.ArchitectureMismatch, match=r'conv\.8\.weight.*div=True'):
        OLSModel(folder=folder, hidden_channels=[24, 40, 12, 20], batch_norm=False, bias=False, div=True)
    for cls, name in ((MeanVarModel, 'net_mean.pt'), (CVAERegression, 'decoder.pt')):
        with pytest.raises(weights.UntrainedFolder, match=name):
            cls(folder=folder, hidden_channels=[24, 40])
    assert not issubclass(weights.UntrainedFolder, ValueError)


def test_from_arrays_takes_nets_of_any_architecture(recorder):
    from pyqg_generative_amd.models import OLSModel, CGANRegression
    xs, ys = AR.scales()
    m = OLSModel.from_arrays([AR.case_net('B')], xs, ys)
    assert recorder.made[-1].nets[0]['arch']['hidden_channels'] == AR.CASES['B']['hidden_channels'] and m.folder is None
    CGANRegression.from_arrays([AR.case_net('A')], xs, ys)
    assert recorder.made[-1].kind == 'gan'


def test_final_activation_is_refused_naming_the_argument(tmp_path):
    from pyqg_generative_amd.models import OLSModel
    with pytest.raises(NotImplementedError, match='final_activation'):
        OLSModel(final_activation='torch.tanh', folder=str(tmp_path))
    with pytest.raises(NotImplementedError, match=r'eval\(\)'):              # ... and why: the reference evaluates the string
        OLSModel(final_activation='torch.tanh', hidden_channels=[16, 16], folder=str(tmp_path))


# ---- C ABI, before any device work -------------------------------------------------------------------------------------------
def _descriptor(hidden=(24, 40, 12, 20), n_in=2, n_out=2, batch_norm=1, bias=1):
    """a complete qgx_cnn_arch on dummy host arrays -> (struct, keep-alive list)"""
    from pyqg_generative_amd import _lib
    a = _lib.qgx_cnn_arch()
    ch = [n_in] + list(hidden) + [n_out]
    a.n_layers = len(ch) - 1
    keep = []
    for l, c in enumerate(ch):
        a.channels[l] = c
    for l in range(a.n_layers):
        a.ksize[l] = 5 if l < 2 and l < a.n_layers - 1 else 3
        buf = np.zeros(max(1, abs(ch[l + 1])) * max(1, abs(ch[l])) * 25, np.float32)
        keep.append(buf)
        a.conv_w[l] = buf.ctypes.data
        a.conv_b[l] = buf.ctypes.data
        if l < a.n_layers - 1:
            for f in ('bn_gamma', 'bn_beta', 'bn_mean', 'bn_var'):
                getattr(a, f)[l] = buf.ctypes.data
    a.batch_norm, a.bias, a.bn_eps = batch_norm, bias, 1e-5
    return a, keep


def _create(kind, descs):
    from pyqg_generative_amd import _lib
    arr = (_lib.qgx_cnn_arch * 2)()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(d))
    xs = (C.c_float * 2)(1.0, 1.0)
    h = C.c_void_p(0)
    rc = _lib.lib.qgx_generator_create_arch(kind, arr, len(descs), xs, xs, 0, C.byref(h))
    return rc, h, _lib.lib.qgx_last_error().decode()


def _set(field, index, value):
    def edit(a):
        if index is None:
            setattr(a, field, value)
        else:
            getattr(a, field)[index] = value
    return edit


@pytest.mark.parametrize('edit,text', [
    (_set('n_layers', None, 1), 'n_layers'), (_set('n_layers', None, 9), 'n_layers'), (_set('n_layers', None, 0), 'n_layers'),
    (_set('channels', 2, 0), r'channels\[2\]'), (_set('channels', 1, 257), r'channels\[1\]'), (_set('channels', 3, -4), r'channels\[3\]'),
    (_set('channels', 0, 3), r'channels\[0\]'), (_set('channels', 5, 3), r'channels\[5\]'),
    (_set('ksize', 1, 4), r'ksize\[1\]'), (_set('ksize', 4, 7), r'ksize\[4\]'), (_set('ksize', 0, 0), r'ksize\[0\]'),
    (_set('batch_norm', None, 2), 'batch_norm'), (_set('bias', None, -1), 'bias'),
    (_set('conv_w', 3, None), r'conv_w\[3\]'), (_set('conv_b', 4, None), r'conv_b\[4\]'),
    (_set('bn_gamma', 0, None), r'bn_gamma\[0\]'), (_set('bn_beta', 1, None), r'bn_beta\[1\]'),
    (_set('bn_mean', 2, None), r'bn_mean\[2\]'), (_set('bn_var', 3, None), r'bn_var\[3\]'),
], ids=lambda v: v if isinstance(v, str) else None)
def test_abi_refuses_every_bad_field_before_any_device_call(edit, text):
    """QGX_ERR_INVALID with the field named, on a machine without a GPU: the refusal precedes every allocation and device call"""
    import re
    from pyqg_generative_amd import _lib
    a, keep = _descriptor()
    edit(a)
    rc, h, msg = _create(_lib.GEN_OLS, [a])
    assert rc == -1 and not h.value, msg
    assert re.search(text, msg), msg


def test_abi_null_pointers_are_fine_where_the_flags_do_not_require_them():
    """batch_norm = 0 / bias = 0: the matching pointers may be NULL — the descriptor passes the checks, and what fails on a machine
    without a GPU is the first device call (QGX_ERR_HIP), on one with a GPU nothing"""
    from pyqg_generative_amd import _lib
    a, keep = _descriptor(batch_norm=0, bias=0)
    for l in range(8):
        a.conv_b[l] = None
    for l in range(7):
        for f in ('bn_gamma', 'bn_beta', 'bn_mean', 'bn_var'):
            getattr(a, f)[l] = None
    rc, h, msg = _create(_lib.GEN_OLS, [a])
    assert rc != -1, msg
    if h.value:
        _lib.lib.qgx_generator_destroy(h)


def test_abi_kind_rules_are_those_of_qgx_generator_create():
    from pyqg_generative_amd import _lib
    ols, _k1 = _descriptor()
    gen, _k2 = _descriptor(n_in=4)
    flux, _k3 = _descriptor(n_out=4)
    for kind, descs, text in ((_lib.GEN_OLS, [ols, ols], 'nets'), (_lib.GEN_GZ, [ols], 'nets'), (_lib.GEN_OLS, [gen], 'n_in'),
                              (_lib.GEN_GAN, [ols], 'n_in'), (_lib.GEN_GAN, [gen, gen], 'n_in'), (_lib.GEN_GZ, [ols, flux], 'n_out'),
                              (7, [ols], 'kind')):
        rc, h, msg = _create(kind, descs)
        assert rc == -1 and not h.value and text in msg, (kind, msg)
    from pyqg_generative_amd import _lib as L
    xs = (C.c_float * 2)(1.0, 1.0)
    h = C.c_void_p(0)
    assert L.lib.qgx_generator_create_arch(L.GEN_OLS, None, 1, xs, xs, 0, C.byref(h)) == -1


def test_struct_and_symbols_match_the_header():
    """include/qgx_arch.h (included by qgx.h) declares what _lib.ARCH_SYMBOLS binds, and the library exports it"""
    import re
    from conftest import ROOT
    from pyqg_generative_amd import _lib
    assert '#include "qgx_arch.h"' in open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    text = open(os.path.join(ROOT, 'include', 'qgx_arch.h')).read()
    assert 'int qgx_generator_create_arch(int kind, const qgx_cnn_arch *nets, int n_nets' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(qgx_[a-z_0-9]+)\s*\(', code)))
    assert declared == sorted(name for name, _, _ in _lib.ARCH_SYMBOLS) == ['qgx_generator_create_arch']
    raw = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert getattr(raw, name) is not None
    assert C.sizeof(_lib.qgx_cnn_arch) == 4 * (1 + 9 + 8 + 3) + 4 + 8 * (8 + 8 + 4 * 7) + 8
    assert 'qgx_generator_create_arch' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
