"""Test-side restatement of AndrewCNN nets of any architecture (pyqg_generative/tools/cnn_tools.py:79-98, 125-176):
len(hidden_channels) + 1 circular-padded convolutions with kernels 5, 5, 3, 3, ... (the last one 3), each hidden one followed by
ReLU and — batch_norm — eval-mode BatchNorm2d; bias optional; div=True: a four-channel last layer and 10000 * divergence behind it.
Plain numpy in float64 (np.roll + einsum per tap), on the dicts of pyqg_generative_amd.weights.synthetic_arch.

The cases of tests/golden/generator_arch.npz (make_golden_arch.py ran them through the reference's own AndrewCNN) are described here
once, for the fixture's generator and every test: weights and latent noise are regenerated from seeds, not stored.  EDGE_CASES, a
second table, holds nets at the ends of what the device engine admits (one of them with other kernel sizes: `forward` takes them
from the weights' shapes); their truth is `forward` itself, pinned to the reference by tests/golden/generator_arch_edges.npz."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
Z_SEED = 7300

# name -> constructor arguments, weight seed, {N: snapshots}
CASES = {
    'A': dict(n_in=4, hidden_channels=[64, 32, 16, 16, 16, 16, 16], batch_norm=True, bias=True, div=False, seed=9101, sizes={16: 2, 64: 1}),
    'B': dict(n_in=2, hidden_channels=[24, 40, 12, 20], batch_norm=False, bias=False, div=False, seed=9102, sizes={16: 2, 48: 1}),
    'C': dict(n_in=2, hidden_channels=[136], batch_norm=True, bias=True, div=False, seed=9103, sizes={16: 2}),
    'D': dict(n_in=4, hidden_channels=[48, 8, 8], batch_norm=True, bias=True, div=True, seed=9104, sizes={16: 2, 64: 1}),
}
ARCH_KEYS = ('n_in', 'hidden_channels', 'batch_norm', 'bias', 'div')


def case_net(name):
    """the weights-module dict of a fixture case (weights.synthetic_arch with the case's seed)"""
    from pyqg_generative_amd import weights
    c = CASES[name]
    return weights.synthetic_arch(**{k: c[k] for k in ARCH_KEYS}, seed=c['seed'])


def scales():
    """x_std, y_std of the shipped models (weights.synthetic's constants)"""
    from pyqg_generative_amd import weights
    _, xs, ys = weights.synthetic('ols')
    return xs, ys


def conv_circular(x, w, b=None):
    """Conv2d(padding='same', padding_mode='circular'): x (B, C, N, N), w (O, C, k, k) -> (B, O, N, N), in x's dtype"""
    k = w.shape[-1]
    p = k // 2
    y = np.zeros((x.shape[0], w.shape[0]) + x.shape[2:], x.dtype)
    for ky in range(k):
        for kx in range(k):
            y += np.einsum('oc,bcyx->boyx', w[:, :, ky, kx].astype(x.dtype), np.roll(x, (p - ky, p - kx), axis=(2, 3)))
    return y if b is None else y + np.asarray(b, x.dtype).reshape(1, -1, 1, 1)


def forward(net, x, dtype='float64', eps=1e-5):
    """AndrewCNN.forward in eval mode, in `dtype` throughout"""
    from div_restatement import divergence_rfftn
    a = np.asarray(x, dtype)
    n = len(net['conv_w'])
    has_b, has_bn = len(net['conv_b']) > 0, len(net['bn_g']) > 0
    for l in range(n):
        a = conv_circular(a, net['conv_w'][l], net['conv_b'][l] if has_b else None)
        if l < n - 1:
            a = np.maximum(a, 0)
            if has_bn:
                g, be, m, v = (np.asarray(net[k][l], dtype).reshape(1, -1, 1, 1) for k in ('bn_g', 'bn_b', 'bn_m', 'bn_v'))
                a = (a - m) / np.sqrt(v + np.asarray(eps, dtype)) * g + be
    if a.shape[1] == 4:
        a = 10000. * divergence_rfftn(a, dtype)
    return np.asarray(a, dtype)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, 'generator_arch.npz'), allow_pickle=False)


def latent_noise(N, T):
    return np.random.RandomState(Z_SEED + N).randn(T, 2, N, N).astype(np.float32)


def inputs(name, N):
    """the case's network input (T, n_in, N, N) float32: the fixture's q / x_std, and for n_in = 4 the white latent noise"""
    T = CASES[name]['sizes'][N]
    X = fixture()[f'q{N}'][:T] / scales()[0].reshape(1, 2, 1, 1)
    assert X.dtype == np.float32
    return np.concatenate([X, latent_noise(N, T)], axis=1) if CASES[name]['n_in'] == 4 else X


def y32(name, N):
    return fixture()[f'{name}_y32_{N}']


def y64(name, N):
    d = fixture()
    return d[f'{name}_y32_{N}'].astype('float64') + d[f'{name}_d16_{N}'].astype('float64') * float(d[f'{name}_dscale_{N}'])


def e_ref(name, N):
    return float(fixture()[f'{name}_eref_{N}'])


# ---- edge cases of the generic engine ----------------------------------------------------------------------------------------
# Nets at the ends of what include/qgx_arch.h admits, chosen for the launch shapes of csrc/conv_generic.hip they reach (output tiles
# of 32 channels ntf = ceil(cout / 32), input chunks of 32 channels):
#   E  ntf 8 (NT = 2, ny = 4); 8 full chunks; a 5x5 layer over 256 channels (K = 6400)
#   F  width 1 (one real channel in a tile of 32, K padded 1 -> 8), and 9 = 8 + 1
#   G  ntf 3 and 7 (NT = 1, blockIdx.y up to 6); 3 and 7 full chunks; 33 = one full chunk + 8; bias without BatchNorm; flux form
#   H  ntf 4 and 6 (NT = 2, ny = 2 and 3); 4 and 6 full chunks; BatchNorm without bias; eight convolutions
#   I  thin: cheap at every grid size and member count (the tile-shape ladder, the online tests)
#   J  NT = 2 at 96 x 96 and 128 x 128 (three M-tiles per wave at 96), flux form: four planar output channels at the largest grids
#   K  kernel sizes [3, 5, 5], an order AndrewCNN builds only through its `kernels=` argument; neither BatchNorm nor bias
# Weights by seed (weights.synthetic_arch; K: the same stream with its own kernel sizes), inputs by seed: nothing is stored but
# tests/golden/generator_arch_edges.npz, the reference's own AndrewCNN in float64 at EDGE_SAMPLES positions of every (case, N).
EDGE_CASES = {
    'E': dict(n_in=4, hidden_channels=[256, 256], batch_norm=True, bias=True, div=False, seed=9201, sizes=(16, 32)),
    'F': dict(n_in=2, hidden_channels=[1, 9, 1], batch_norm=True, bias=True, div=False, seed=9202, sizes=(16, 128)),
    'G': dict(n_in=4, hidden_channels=[96, 224, 33], batch_norm=False, bias=True, div=True, seed=9203, sizes=(16, 32)),
    'H': dict(n_in=2, hidden_channels=[128, 192, 8, 8, 8, 8, 8], batch_norm=True, bias=False, div=False, seed=9204, sizes=(16, 48)),
    'I': dict(n_in=4, hidden_channels=[16, 8], batch_norm=True, bias=True, div=False, seed=9205, sizes=(16, 32, 48, 64, 96, 128)),
    'J': dict(n_in=4, hidden_channels=[64, 24], batch_norm=True, bias=True, div=True, seed=9206, sizes=(96, 128)),
    'K': dict(n_in=2, hidden_channels=[20, 12], batch_norm=False, bias=False, div=False, seed=9207, sizes=(16, 64), kernels=[3, 5, 5]),
}
EDGE_T = 2              # members evaluated in float64; further members are circular shifts of them
EDGE_X_SEED = 7500
EDGE_SAMPLES = 256
EDGE_KIND = {name: 'gan' if c['n_in'] == 4 else 'ols' for name, c in EDGE_CASES.items()}


def edge_kernels(name):
    from pyqg_generative_amd import weights
    c = EDGE_CASES[name]
    return list(c.get('kernels') or weights.arch_kernels(c['hidden_channels']))


def edge_net(name):
    """the weights-module dict of an edge case; K (kernel sizes synthetic_arch does not build) is assembled here from the stream
    synthetic_arch draws: per convolution the He-scaled weight and nothing else (no bias, no BatchNorm)"""
    from pyqg_generative_amd import weights
    c = EDGE_CASES[name]
    if 'kernels' not in c:
        return weights.synthetic_arch(**{k: c[k] for k in ARCH_KEYS}, seed=c['seed'])
    assert not c['batch_norm'] and not c['bias'] and not c['div']
    rs = np.random.RandomState(c['seed'])
    ch = [c['n_in']] + list(c['hidden_channels']) + [2]
    net = dict(conv_w=[], conv_b=[], bn_g=[], bn_b=[], bn_m=[], bn_v=[], arch={k: c[k] for k in ARCH_KEYS})
    for l, k in enumerate(c['kernels']):
        net['conv_w'].append((rs.randn(ch[l + 1], ch[l], k, k) * np.sqrt(2.0 / (ch[l] * k * k))).astype('float32'))
    return net


def edge_inputs(name, N):
    """(EDGE_T, n_in, N, N) float32: white noise, the PV channels 1.5 times wider (q / x_std is O(1) with a heavier tail than z)"""
    c = EDGE_CASES[name]
    x = np.random.RandomState(EDGE_X_SEED + 1000 * c['n_in'] + N).randn(EDGE_T, c['n_in'], N, N).astype(np.float32)
    x[:, :2] *= np.float32(1.5)
    return x


@functools.lru_cache(maxsize=None)
def edge_truth(name, N):
    """the float64 restatement on the case's inputs (EDGE_T, 2, N, N): computed once, read-only"""
    y = forward(edge_net(name), edge_inputs(name, N))
    y.setflags(write=False)
    return y


def edge_positions(name, N):
    """EDGE_SAMPLES flat indices into (EDGE_T, 2, N, N) at which the fixture holds the reference's float64 output"""
    return np.random.RandomState(EDGE_CASES[name]['seed'] + N).randint(0, EDGE_T * 2 * N * N, EDGE_SAMPLES)


@functools.lru_cache(maxsize=None)
def edge_fixture():
    return np.load(os.path.join(GOLDEN, 'generator_arch_edges.npz'), allow_pickle=False)


def edge_members(name, N, B):
    """B members and their float64 truth: member m is input m % EDGE_T shifted circularly by (5, 3) * (m // EDGE_T) pixels (the
    convolutions are circular and the divergence is spectral, so the forward commutes with shifts: see _members of
    tests/test_gpu_arch.py)"""
    x, y = edge_inputs(name, N), edge_truth(name, N)
    xs, ys = np.empty((B,) + x.shape[1:], np.float32), np.empty((B, 2, N, N))
    for m in range(B):
        t, shift = m % EDGE_T, ((5 * (m // EDGE_T)) % N, (3 * (m // EDGE_T)) % N)
        xs[m], ys[m] = np.roll(x[t], shift, axis=(-2, -1)), np.roll(y[t], shift, axis=(-2, -1))
    return xs, ys


# The member counts of the tile-shape ladder: (case, N) -> B list.  rows_generic (csrc/conv_generic.hip) halves the rows per
# workgroup R while B * (N / R) * ny < 256; with ny = 1 (cases I: every layer one output tile; J: two tiles on NT = 2) these counts
# select every R the rule can give at that N, and 63 at 32 x 32 / 10 at 96 x 96 sit one below a threshold.  E (ny = 4 on its
# 256-wide layers, 1 on its last) changes the shapes of the two kinds of layer at different counts: R = 2, 2, 4, 8, 16 on the wide
# layers (the patch of R + 4 rows taller than the image at the end) beside 2, 2, 2, 2, 4 on the last.
LADDER = {
    ('I', 16): [1, 64, 128, 256], ('I', 32): [1, 16, 32, 63, 64], ('I', 48): [1, 22, 43], ('I', 64): [1, 8, 16],
    ('I', 96): [1, 6, 10, 11], ('I', 128): [1, 4],
    ('J', 96): [1, 6, 11], ('J', 128): [1, 4],
    ('E', 16): [1, 8, 16, 32, 64],
}

# the launches of the first table that tests/test_gpu_arch.py::test_cnn_forward_matches_the_reference compares with the fixture
SHAPES = [(n, 16, B) for n in CASES for B in (1, 3, 40)] + [('A', 64, 1), ('A', 64, 16), ('B', 48, 1), ('B', 48, 22), ('B', 48, 44),
                                                            ('D', 64, 1), ('D', 64, 16)]


def launch_table():
    """every (case, N, B) whose qgx_cnn_forward the GPU tests compare with a truth: SHAPES, the edge cases' two members and the
    ladder"""
    return sorted(set(SHAPES) | {(name, N, EDGE_T) for name, c in EDGE_CASES.items() for N in c['sizes']}
                  | {(name, N, B) for (name, N), Bs in LADDER.items() for B in Bs})


def write_folder(path, kind, nets, args=None):
    """a reference-layout model folder: the state dicts of `nets` under the kind's file names, the scalers, model_args.json"""
    import json
    import torch
    from pyqg_generative_amd import weights
    files = {'gan': ['G.pt', 'net_mean.pt'], 'vae': ['decoder.pt', 'net_mean.pt'], 'gz': ['net_mean.pt', 'net_var.pt'], 'ols': ['net.pt']}[kind]
    for f, net in zip(files, nets):
        torch.save({k: torch.as_tensor(v) for k, v in weights.state_dict_from_net(net).items()}, os.path.join(path, f))
    for name, std in zip(('x_scale.json', 'y_scale.json'), scales()):
        std = np.asarray(std, np.float32).reshape(1, 2, 1, 1)
        with open(os.path.join(path, name), 'w') as f:
            json.dump(dict(mean=str((0 * std).tolist()), std=str(std.tolist())), f)
    if args is not None:
        with open(os.path.join(path, 'model_args.json'), 'w') as f:
            json.dump(args, f)
    return str(path)
