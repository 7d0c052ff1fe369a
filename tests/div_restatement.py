"""Test-side restatement of flux-form nets, AndrewCNN(div=True) (pyqg_generative/tools/cnn_tools.py:100-123, 139-142, 170-175):
the last convolution writes 2 n_out channels [fx of both layers, fy of both layers], and forward returns
10000 * divergence(fluxes), float32, spectral, with the ik / il grid lines of pyqg.QGModel(nx=N) at pyqg's default L = 1e6 cast to
complex64.

Two forms of the divergence:
  divergence_rfftn   the reference's own: irfftn(ik rfftn(fx) + il rfftn(fy))
  divergence_plane   the equivalent Hermitian multipliers on the full (l, k) plane that a complex transform packing two real
                     fields needs (csrc/fluxdiv.hip): the c2r transform drops the imaginary part of the self-conjugate bins, and
                     pyqg's l at the Nyquist row is -N/2 dk while k at the Nyquist column is +N/2 dk, so
                       Hx(l,k) = i dk k, 0 on the column k = +-N/2;
                       Hy(l,k) = i dk l (l != N/2); on the row l = N/2: i dk (-N/2) sign(k), 0 at k = 0 and k = N/2.
                     rule='naive_row' (i dk (-N/2) on the whole Nyquist row) and rule='zero_row' are the two plausible wrong
                     rules the fixture is shown to be sensitive to.

The nets are the shipped layers 1-7 (weights_gan.npz; weights_gz.npz's net_mean as the 2-input net) with the seeded four-channel
last layers of tests/golden/generator_div.npz (make_golden_div.py ran them through the reference's own AndrewCNN(div=True)).
"""
import functools
import os

import numpy as np
import torch

from oracle.gen_ref import CNNWeights, GeneratorRef, ScalerRef, cnn_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
L_PYQG = 1e6


def grid_lines(N):
    """float64 kk (N/2 + 1), ll (N) of pyqg.QGModel(nx=N)"""
    dk = 2 * np.pi / L_PYQG
    return dk * np.arange(0., N / 2 + 1), dk * np.append(np.arange(0., N / 2), np.arange(-N / 2, 0.))


def divergence_rfftn(F, dtype='float32'):
    """cnn_tools.divergence: F (B, 4, N, N) -> (B, 2, N, N); the wavenumbers are float32 in either precision (complex64 there)"""
    N = F.shape[-1]
    kk, ll = grid_lines(N)
    td = torch.float64 if dtype == 'float64' else torch.float32
    ik = torch.as_tensor((1j * kk[None, :] + 0 * ll[:, None]).astype('complex64'))
    il = torch.as_tensor((1j * ll[:, None] + 0 * kk[None, :]).astype('complex64'))
    x = torch.as_tensor(np.ascontiguousarray(F)).to(td)
    ix = torch.fft.rfftn(x, dim=(-2, -1))
    div = torch.fft.irfftn(ix[:, :2] * ik + ix[:, 2:] * il, dim=(-2, -1))
    assert div.dtype == td
    return div.numpy()


def plane_multipliers(N, rule='exact'):
    """Hx, Hy (N, N) complex128 on the full plane, float32-rounded wavenumbers"""
    kk, ll = grid_lines(N)
    f32 = lambda a: a.astype('float32').astype('float64')
    k = f32(np.append(kk[:N // 2], -kk[N // 2:0:-1]))          # fftfreq order: 0 .. N/2-1, -N/2 .. -1
    l = f32(ll)
    Hx = 1j * np.broadcast_to(k[None, :], (N, N)).copy()
    Hy = 1j * np.broadcast_to(l[:, None], (N, N)).copy()
    Hx[:, N // 2] = 0
    if rule == 'exact':
        sign = np.sign(np.fft.fftfreq(N))
        sign[N // 2] = 0
        Hy[N // 2, :] = 1j * l[N // 2] * sign
    elif rule == 'zero_row':
        Hy[N // 2, :] = 0
    else:
        assert rule == 'naive_row'
    return Hx, Hy


def divergence_plane(F, rule='exact'):
    """float64: ifft2(Hx fft2(fx1 + i fx2) + Hy fft2(fy1 + i fy2)) -> the two output layers as real and imaginary part"""
    F = np.asarray(F, 'float64')
    Hx, Hy = plane_multipliers(F.shape[-1], rule)
    z = np.fft.ifft2(Hx * np.fft.fft2(F[:, 0] + 1j * F[:, 1]) + Hy * np.fft.fft2(F[:, 2] + 1j * F[:, 3]))
    return np.stack([z.real, z.imag], axis=1)


def flux_forward(net, x, dtype='float32', rule=None):
    """AndrewCNN(div=True).forward in eval mode: conv stack (oracle.gen_ref.cnn_forward) then 10000 * divergence.  rule: the
    full-plane form with that multiplier rule (float64 divergence of the dtype's fluxes) instead of the rfftn form"""
    Fx = cnn_forward(net, x, dtype=dtype)
    assert Fx.shape[1] == 4
    if rule is not None:
        return 10000. * divergence_plane(Fx, rule)
    return (10000. * torch.as_tensor(divergence_rfftn(Fx, dtype))).numpy()


def net_forward(net, x, dtype='float32'):
    return flux_forward(net, x, dtype) if net.n_out == 4 else cnn_forward(net, x, dtype=dtype)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, 'generator_div.npz'), allow_pickle=False)


def _shipped(kind):
    d = np.load(os.path.join(GOLDEN, 'weights_gan.npz' if kind == 'gan' else 'weights_gz.npz'), allow_pickle=False)
    return d


def flux_net_dict(kind):
    """weights-module dict (conv_w, conv_b, bn_*) of the fixture's flux-form net: 'gan' AndrewCNN(4, 2, div=True),
    'ols' AndrewCNN(2, 2, div=True)"""
    from pyqg_generative_amd import weights
    net = weights.net_from_npz(_shipped(kind), 'net0_')
    assert weights.net_checksum(net) == str(fixture()[f'{kind}_checksum'])
    net['conv_w'][7] = np.asarray(fixture()[f'{kind}_last_w'], np.float32)
    net['conv_b'][7] = np.asarray(fixture()[f'{kind}_last_b'], np.float32)
    return net


def flux_net_ref(kind):
    n = flux_net_dict(kind)
    return CNNWeights(n['conv_w'], n['conv_b'], n['bn_g'], n['bn_b'], n['bn_m'], n['bn_v'])


def scales():
    d = fixture()
    return np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32)


def latent_noise(N, T):
    return np.random.RandomState(int(fixture()['z_seed']) + N).randn(T, 2, N, N).astype(np.float32)


def inputs(kind, N):
    """the fixture's network input x (T, n_in, N, N) float32: q / x_std, and for 'gan' the white latent noise behind it"""
    d = fixture()
    T = d[f'{kind}_y32_{N}'].shape[0]
    X = d[f'q{N}'][:T] / scales()[0].reshape(1, 2, 1, 1)
    assert X.dtype == np.float32
    return np.concatenate([X, latent_noise(N, d[f'q{N}'].shape[0])[:T]], axis=1) if kind == 'gan' else X


def y32(kind, N):
    return fixture()[f'{kind}_y32_{N}']


def y64(kind, N):
    d = fixture()
    return d[f'{kind}_y32_{N}'].astype('float64') + d[f'{kind}_d16_{N}'].astype('float64') * float(d[f'{kind}_dscale_{N}'])


def e_ref(kind, N):
    return float(fixture()[f'{kind}_eref_{N}'])


class FluxGeneratorRef(GeneratorRef):
    """GeneratorRef whose nets may be flux-form (either, independently); kind 'ols': one net, no latent noise
    (ols_model.py:65-75)"""

    def __init__(self, kind, nets, x_std, y_std):
        self.kind, self.nets = kind, nets
        self.x_scale, self.y_scale = ScalerRef(x_std), ScalerRef(y_std)
        self.n_latent = 2

    def generate_latent_noise(self, ny, nx, rng=None):
        return 0 if self.kind == 'ols' else super().generate_latent_noise(ny, nx, rng)

    def predict_snapshot(self, q, noise):
        X = self.x_scale.normalize(np.asarray(q).astype('float32'))
        if self.kind == 'ols':
            Y = net_forward(self.nets[0], X)
        else:
            Y = net_forward(self.nets[0], np.concatenate([X, np.asarray(noise).astype('float32')], axis=1))
            if len(self.nets) == 2:
                Y = Y + net_forward(self.nets[1], X)
        return self.y_scale.denormalize(Y).squeeze().astype('float64')

    def predict_mean_snapshot(self, q, M=100, rng=None, z=None):
        X = self.x_scale.normalize(np.asarray(q).astype('float32'))
        if z is None:
            z = (rng if rng is not None else np.random).randn(M, self.n_latent, X.shape[2], X.shape[3]).astype('float32')
        Y = net_forward(self.nets[0], np.concatenate([np.tile(X, (M, 1, 1, 1)), z], axis=1)).mean(0, keepdims=True)
        if len(self.nets) == 2:
            Y = Y + net_forward(self.nets[1], X)
        return self.y_scale.denormalize(Y).squeeze().astype('float64')
