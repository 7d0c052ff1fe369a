"""Test-side restatement of the U-Net's training convolution of include/qgx_uconv_train.h, in float64 numpy and in the ABI's
layout: activations (B, N, N, C8) with zero pad channels, weights (cout, cin, k, k), k 1 or 3, circular padding k // 2, any grid
N >= 2 (np.roll wraps as torch's circular padding does: at N = 2 the taps 0 and 2 reach the same row).

  forward(x, w, b)                     y[b, co, y, x] = sum x[b, ci, y + ky - P, x + kx - P] w[co, ci, ky, kx] + b[co]
  backward_data(dy, w)                 dx[b, ci, y, x] = sum dy[b, co, y - ky + P, x - kx + P] w[co, ci, ky, kx]
  backward_weight(x, dy, cin, cout, k) dw[co, ci, ky, kx] = sum dy[b, co, y, x] x[b, ci, y + ky - P, x + kx - P], db = sum dy

and of the weight gradient's host-side plan (uwgrad_plan, workspace_bytes), a function of the shape alone, the regimes of the GPU
cases declared as data, the U-Net's layer shapes, and a torch twin of DeepInversionGenerator(4, 2) written from the architecture
description (tests/unet_restatement.py) that a state dict is loaded into with strict=True.  A plain helper module.
"""
import numpy as np

from conv_train_restatement import c8, to_layout, from_layout


def forward(x, w, b=None):
    w = np.asarray(w, np.float64)
    cout, cin, k = w.shape[:3]
    p = k // 2
    xs = from_layout(np.asarray(x, np.float64), cin)
    y = np.zeros((xs.shape[0], cout) + xs.shape[2:])
    for ky in range(k):
        for kx in range(k):
            y += np.einsum('oc,bcyx->boyx', w[:, :, ky, kx], np.roll(xs, (p - ky, p - kx), axis=(2, 3)), optimize=True)
    if b is not None:
        y += np.asarray(b, np.float64).reshape(1, -1, 1, 1)
    return to_layout(y)


def backward_data(dy, w):
    w = np.asarray(w, np.float64)
    cout, cin, k = w.shape[:3]
    p = k // 2
    g = from_layout(np.asarray(dy, np.float64), cout)
    dx = np.zeros((g.shape[0], cin) + g.shape[2:])
    for ky in range(k):
        for kx in range(k):
            dx += np.einsum('oc,boyx->bcyx', w[:, :, ky, kx], np.roll(g, (ky - p, kx - p), axis=(2, 3)), optimize=True)
    return to_layout(dx)


def backward_weight(x, dy, cin, cout, k):
    p = k // 2
    xs, g = from_layout(np.asarray(x, np.float64), cin), from_layout(np.asarray(dy, np.float64), cout)
    dw = np.zeros((cout, cin, k, k))
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = np.einsum('boyx,bcyx->oc', g, np.roll(xs, (p - ky, p - kx), axis=(2, 3)), optimize=True)
    return dw, g.sum(axis=(0, 2, 3))


def case_data(cin, cout, k, B, N, seed, integer):
    """x, w, bias, dy of one case in the ABI's layout (float32, zero pad channels); integer: drawn from -3 ... 3"""
    rs = np.random.RandomState(seed)
    if integer:
        draw = lambda *s: rs.randint(-3, 4, size=s).astype(np.float32)
    else:
        draw = lambda *s: rs.randn(*s).astype(np.float32)
    x, dy = to_layout(draw(B, cin, N, N)), to_layout(draw(B, cout, N, N))
    return x, draw(cout, cin, k, k), draw(cout), dy


# ---- the weight gradient's plan ------------------------------------------------------------------------------------------------
TILE, UNIT, WORKGROUPS = 64, 32, 512


def cdiv(a, b):
    return (a + b - 1) // b


def up(v, m):
    return cdiv(v, m) * m


def uwgrad_plan(B, N, cin, cout, k):
    """units of 32 pixels, S shares of `ups` consecutive units, tiles of 64 output channels x 64 (tap, channel) pairs"""
    P = B * N * N
    U = cdiv(P, UNIT)
    cot_n, nt_n = cdiv(cout, TILE), cdiv(k * k * cin, TILE)
    tiles = cot_n * nt_n
    want = min(cdiv(WORKGROUPS, tiles), U)
    ups = cdiv(U, want)
    S = cdiv(U, ups)
    return dict(P=P, U=U, ups=ups, S=S, last_units=U - (S - 1) * ups, last_pixels=P - (U - 1) * UNIT, cot_n=cot_n, nt_n=nt_n,
                tiles=tiles, direct=S == 1)


def workspace_bytes(B, N, cin, cout, k):
    """floats, every part rounded up to 64: the packed weights (of the forward, cout x k^2 cin8, or of the data gradient,
    cin x k^2 cout8, whichever is larger) | with more than one share, the shares' slices [S][tiles][64][64] | and their db
    sums [S][cot_n 64]"""
    p = uwgrad_plan(B, N, cin, cout, k)
    n = up(max(cout * k * k * c8(cin), cin * k * k * c8(cout)), 64)
    if p['S'] > 1:
        n += up(p['S'] * p['tiles'] * TILE * TILE, 64) + up(p['S'] * p['cot_n'] * TILE, 64)
    return 4 * n


# the GPU cases (cin, cout, k, B, N) that are there for a regime of the weight gradient, and the regime as data
UCONV_REGIMES = {
    (4, 8, 3, 500, 6): dict(tiles=1, U=563, ups=2, S=282, last_units=1, last_pixels=16, direct=False),      # several units, ragged
    (8, 72, 3, 500, 6): dict(cot_n=2, nt_n=2, U=563, ups=5, S=113, last_units=3, direct=False),             # ragged last share
    (3, 5, 1, 600, 16): dict(tiles=1, U=4800, ups=10, S=480, last_units=10, direct=False),                  # k = 1, full shares
    (512, 456, 3, 3, 4): dict(tiles=576, U=2, ups=2, S=1, last_pixels=16, direct=True),                     # S = 1 over two units
    (7, 33, 3, 3, 6): dict(tiles=1, U=4, ups=1, S=4, last_pixels=12, direct=False),                         # units cross images
}


def unet_layers(N):
    """every convolution of DeepInversionGenerator(4, 2) at an N x N input as (cin, cout, k, grid): conv32, the eleven residual
    units (conv.1, conv.4, conv1), the four ConvTranspose2d as 1 x 1 products with 4 C / 2 outputs, conv_end"""
    unit = lambda ci, co, n: [(ci, co, 3, n), (co, co, 3, n), (ci, co, 1, n)]
    L = [(4, 32, 3, N)] + unit(32, 32, N)
    for i, (ci, co) in enumerate(((32, 64), (64, 128), (128, 256), (256, 512))):
        L += unit(ci, co, N >> (i + 1))
    L += unit(512, 512, N // 16)
    for i, c in enumerate((512, 256, 128, 64)):
        L += [(c, 2 * c, 1, N >> (4 - i))] + unit(c, c // 2, N >> (3 - i))
    return L + unit(32, 32, N) + [(32, 2, 1, N)]


# ---- a torch twin of the U-Net ---------------------------------------------------------------------------------------------------
def torch_twin():
    """DeepInversionGenerator(4, 2) as plain torch modules with the reference's state-dict keys; forward is the eval-mode
    restatement of tests/unet_restatement.py on its own state dict"""
    import torch
    from torch import nn
    import unet_restatement as ur

    def unit(ci, co, bn):
        m = nn.Module()
        m.bn = nn.BatchNorm2d(ci) if bn else nn.Identity()
        m.conv = nn.Sequential(nn.LeakyReLU(0.2), nn.Conv2d(ci, co, 3, padding=1, padding_mode='circular'),
                               nn.BatchNorm2d(co) if bn else nn.Identity(), nn.LeakyReLU(0.2),
                               nn.Conv2d(co, co, 3, padding=1, padding_mode='circular'))
        m.conv1 = nn.Conv2d(ci, co, 1)
        return m

    class Twin(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv32 = nn.Conv2d(4, 32, 3, padding=1, padding_mode='circular')
            self.res32_start = unit(32, 32, False)
            for ci, co in ((32, 64), (64, 128), (128, 256), (256, 512)):
                d = nn.Module()
                d.conv = nn.Sequential(nn.AvgPool2d(2, 2), unit(ci, co, True))
                setattr(self, f'down{co}', d)
            self.res512 = unit(512, 512, True)
            for c in (512, 256, 128, 64):
                u = nn.Module()
                u.upsampling = nn.ConvTranspose2d(c, c // 2, 2, stride=2)
                u.conv = unit(c, c // 2, True)
                setattr(self, f'up{c}', u)
            self.res32_end = unit(32, 32, False)
            self.conv_end = nn.Conv2d(32, 2, 1)

        def forward(self, x):
            return ur.forward({k: v for k, v in self.state_dict().items()}, x)

    with torch.random.fork_rng(devices=[]):
        return Twin()
