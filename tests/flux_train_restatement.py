"""Test-side restatement of the training of flux-form nets, AndrewCNN(div=True): the adjoint of the spectral divergence of
tests/div_restatement.py in float64 numpy, the divergence as a differentiable torch expression (the reference's own rfftn form,
cnn_tools.py:100-123) in float32 or float64, and the reference's div=True net on torch CPU modules.

The forward is D F = ifft2(Hx fft2(fx) + Hy fft2(fy)) per layer with the Hermitian multipliers of div_restatement.plane_multipliers.
The adjoint of ifft2 H fft2 on real fields is ifft2 conj(H) fft2, and the operator is real, so it acts on the real and the
imaginary part of g1 + i g2 separately:
    dfx1 + i dfx2 = ifft2(conj(Hx) fft2(g1 + i g2)),   dfy1 + i dfy2 = ifft2(conj(Hy) fft2(g1 + i g2)).
Neither function here carries the net's factor 10000: the callers state it.
"""
import numpy as np
import torch

import conv_train_restatement as cr
import div_restatement as dr

GRIDS = (16, 32, 48, 64, 96, 128)          # what include/qgx_flux_train.h admits
SCALE = 10000.


def divergence_adjoint(g, rule='exact'):
    """float64: g (B, 2, N, N) -> D^T g (B, 4, N, N) = [dfx1, dfx2, dfy1, dfy2]"""
    g = np.asarray(g, 'float64')
    Hx, Hy = dr.plane_multipliers(g.shape[-1], rule)
    G = np.fft.fft2(g[:, 0] + 1j * g[:, 1])
    zx, zy = np.fft.ifft2(np.conj(Hx) * G), np.fft.ifft2(np.conj(Hy) * G)
    return np.stack([zx.real, zx.imag, zy.real, zy.imag], axis=1)


def divergence_adjoint_per_layer(g, rule='exact'):
    """the same, one real field at a time: dfx_c = real(ifft2(conj(Hx) fft2(g_c))) (the form the identities are derived in)"""
    g = np.asarray(g, 'float64')
    Hx, Hy = dr.plane_multipliers(g.shape[-1], rule)
    G = np.fft.fft2(g)                                        # (B, 2, N, N), over the last two axes
    return np.concatenate([np.fft.ifft2(np.conj(Hx) * G).real, np.fft.ifft2(np.conj(Hy) * G).real], axis=1)


def divergence_torch(F):
    """div_restatement.divergence_rfftn as a differentiable torch expression in F's dtype: (B, 4, N, N) -> (B, 2, N, N); the
    wavenumbers are complex64 in either precision, as the reference's are"""
    N = F.shape[-1]
    kk, ll = dr.grid_lines(N)
    ik = torch.as_tensor((1j * kk[None, :] + 0 * ll[:, None]).astype('complex64'))
    il = torch.as_tensor((1j * ll[:, None] + 0 * kk[None, :]).astype('complex64'))
    ix = torch.fft.rfftn(F, dim=(-2, -1))
    div = torch.fft.irfftn(ix[:, :2] * ik + ix[:, 2:] * il, dim=(-2, -1))
    assert div.dtype == F.dtype
    return div


def autograd_pair(F, g, dtype):
    """(D F, D^T g) by torch CPU in `dtype`: the forward of the rfftn form and its autograd gradient for the cotangent g"""
    Ft = torch.tensor(np.asarray(F), dtype=dtype, requires_grad=True)
    y = divergence_torch(Ft)
    y.backward(torch.tensor(np.asarray(g), dtype=dtype))
    return y.detach().numpy(), Ft.grad.numpy()


def white(B, C, N, seed):
    """white Gaussian float32 fields (B, C, N, N): every wavenumber carries weight, the Nyquist row and column included"""
    return np.random.RandomState(seed).randn(B, C, N, N).astype(np.float32)


def flux_torch_net(n_in, hidden, batch_norm, bias, dtype, state_dict=None):
    """the reference's AndrewCNN(n_in, 2, div=True): conv_train_restatement.torch_net with 4 outputs, then 10000 * divergence"""
    net = cr.torch_net(n_in, 4, hidden, batch_norm, bias, dtype, state_dict)

    class FluxNet(type(net)):
        def forward(self, x):
            return SCALE * divergence_torch(self.conv(x))
    net.__class__ = FluxNet
    return net
