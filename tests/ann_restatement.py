"""Test-side restatement of ANNModel's inference (pyqg_generative/models/ann_model.py:79-93, net tools/cnn_tools.py:184-210,
stencils :321-339) in numpy float32: generate_latent_noise returns 0 and predict_snapshot(q, noise) =
float64(float32(y_scale * ANN(stencil(float32(q)) / x_scale))), noise ignored, both layers through the same net.  It has
the interface oracle.gen_ref.ParameterizationRef calls, so it plugs into that and into oracle.qg_ref.QGModelRef unchanged.

The nets are the seeded ANNs tests/golden/make_golden_ann.py ran through the reference's ANNModel (tests/golden/ann.npz).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TAGS = ('a', 'b', 'c')


def net_from_fixture(d, tag):
    """the net `tag` of ann.npz as a weights.ann_from_state_dict dict"""
    hidden = [int(h) for h in d[f'{tag}_hidden']]
    n = len(hidden) + 1
    return dict(stencil_size=int(d[f'{tag}_s']), hidden=hidden, scale_invariant=bool(d[f'{tag}_si']),
                w=[np.asarray(d[f'{tag}_w{l}'], np.float32) for l in range(n)],
                b=[np.asarray(d[f'{tag}_b{l}'], np.float32) for l in range(n)])


def ann_forward(net, x):
    """the raw net on normalised float32 images x (..., N, N) -> (..., N, N) float32; features dy * s + dx of the wrapped
    stencil; ReLU lets NaN through (torch's relu does; np.maximum would too, written out here)"""
    s = net['stencil_size']
    h = s // 2
    N = x.shape[-1]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(h, h), (h, h)], mode='wrap')
    a = np.stack([xp[..., dy:dy + N, dx:dx + N] for dy in range(s) for dx in range(s)], axis=-1).astype(np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        if net['scale_invariant']:
            norm = np.sqrt((a * a).sum(axis=-1, keepdims=True, dtype=np.float32))
            a = a / norm
        n = len(net['w'])
        for l in range(n):
            a = (a @ net['w'][l].T + net['b'][l]).astype(np.float32)
            if l + 1 < n:
                a = np.where(a < 0, np.float32(0), a)
        y = a[..., 0]
        if net['scale_invariant']:
            y = (norm[..., 0] * norm[..., 0]) * y
    return y.astype(np.float32)


class ANNRef:
    def __init__(self, net, x_scale, y_scale):
        self.net = net
        self.x_scale, self.y_scale = float(x_scale), float(y_scale)

    @classmethod
    def from_fixture(cls, tag='a'):
        d = np.load(os.path.join(GOLDEN, 'ann.npz'), allow_pickle=False)
        return cls(net_from_fixture(d, tag), d['x_scale'], d['y_scale'])

    def generate_latent_noise(self, ny, nx, rng=None):
        return 0                                                          # ann_model.py:79-80

    def predict_snapshot(self, q, noise):
        """q: (2, N, N) or (T, 2, N, N) float64 -> S of the same shape, float64 (not de-meaned)"""
        x = np.asarray(q).astype(np.float32) / np.float32(self.x_scale)    # ann_model.py:87-89
        return (np.float32(self.y_scale) * ann_forward(self.net, x)).astype(np.float32).astype(np.float64)
