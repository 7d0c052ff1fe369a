#!/usr/bin/env python
"""Golden vectors of flux-form nets, AndrewCNN(div=True): imports the reference's own AndrewCNN and CGANRegression
(pyqg_generative/tools/cnn_tools.py:100-176, models/cgan_regression.py) with the inert stubs of make_golden.py.  cnn_tools.divergence
builds pyqg.QGModel(nx=N) for its ik / il grid lines only; pyqg is not installed, so the stub's QGModel holds exactly those lines as
pyqg 0.7.2 defines them (dk = 2 pi / L, kk = dk arange(N/2 + 1), ll = dk [0 .. N/2 - 1, -N/2 .. -1], L = 1e6, k, l = meshgrid(kk, ll),
ik = 1j k, il = 1j l) — no other arithmetic of pyqg is involved.

Nets: layers 1-7 of the shipped GAN generator (weights_gan.npz) and of GZ's net_mean (weights_gz.npz, the AndrewCNN(2, 2) used as the
OLS-kind and as the regression net) with SEEDED four-channel last layers.  Only the last layers and the checksums of the shipped nets
are stored.  Inputs: band-limited PV of the training amplitude (stored in physical units as float32, normalised by x_std as
predict_snapshot does) and white latent noise, which is NOT stored: z = RandomState(z_seed + N).randn(T, 2, N, N).astype(float32)
(the legacy stream is frozen across numpy versions).

Per N (GAN kind: 16, 48, 64, 96, 128; OLS kind and CGANRegression(regression='full_loss') predict_snapshot: 16, 64):
  q{N}            (T, 2, N, N) float32 PV
  gan_y32_{N}     float32 forward of AndrewCNN(4, 2, div=True) on [q / x_std, z]
  gan_d16_{N}, gan_dscale_{N}   the float64 forward as y64 = y32 + d16 * dscale (d16 float16: 2^-11 of a difference that is itself
                  5e-7 of max|y| — 2000 x below the reference's own float32 error; halves the fixture)
  gan_eref_{N}    max|y32 - y64| / max|y64|
  ols_*           the same for AndrewCNN(2, 2, div=True) on q / x_std (first T_ols snapshots)
  S_{N}           CGANRegression(regression='full_loss', div=True).predict_snapshot, float32 without loss

Run:  python tests/golden/make_golden_div.py      (build machine, with the reference checked out)
"""
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import install_inert_stubs, REF  # noqa: E402
from make_golden_ols import eddy_like_q  # noqa: E402

GAN_SIZES = {16: 2, 48: 2, 64: 2, 96: 1, 128: 1}
OLS_SIZES = {16: 2, 64: 1}
Z_SEED = 7100
LAST_SEED = {'gan': 501, 'ols': 502}


def install_grid_stub():
    import pyqg

    class QGModel:
        def __init__(self, nx=64, L=1e6, **kw):
            dk = 2 * np.pi / L
            kk = dk * np.arange(0., nx / 2 + 1)
            ll = dk * np.append(np.arange(0., nx / 2), np.arange(-nx / 2, 0.))
            self.k, self.l = np.meshgrid(kk, ll)
            self.ik, self.il = 1j * self.k, 1j * self.l
    pyqg.QGModel = QGModel


def last_layer(kind):
    """seeded (4, 32, 3, 3) last layer: fluxes of order one"""
    rs = np.random.RandomState(LAST_SEED[kind])
    return (rs.randn(4, 32, 3, 3) / np.sqrt(32 * 9)).astype(np.float32), (0.1 * rs.randn(4)).astype(np.float32)


def latent_noise(N, T):
    return np.random.RandomState(Z_SEED + N).randn(T, 2, N, N).astype(np.float32)


def state_dict(net, last):
    import torch
    sd = {}
    for i in range(8):
        sd[f'conv.{3 * i}.weight'] = torch.as_tensor(net['conv_w'][i] if i < 7 else last[0])
        sd[f'conv.{3 * i}.bias'] = torch.as_tensor(net['conv_b'][i] if i < 7 else last[1])
        if i < 7:
            for key, name in (('bn_g', 'weight'), ('bn_b', 'bias'), ('bn_m', 'running_mean'), ('bn_v', 'running_var')):
                sd[f'conv.{3 * i + 2}.{name}'] = torch.as_tensor(net[key][i])
    return sd


def main():
    install_inert_stubs()
    install_grid_stub()
    sys.path.insert(0, REF)
    import copy
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.cnn_tools import AndrewCNN, ChannelwiseScaler
    from pyqg_generative.models.cgan_regression import CGANRegression
    from pyqg_generative_amd import weights as W

    dg, dz = np.load(os.path.join(HERE, 'weights_gan.npz')), np.load(os.path.join(HERE, 'weights_gz.npz'))
    shipped = {'gan': W.net_from_npz(dg, 'net0_'), 'ols': W.net_from_npz(dz, 'net0_')}
    x_std, y_std = np.asarray(dg['x_std'], np.float32), np.asarray(dg['y_std'], np.float32)
    out = {'x_std': x_std, 'y_std': y_std, 'z_seed': np.array(Z_SEED)}
    nets = {}
    for kind, n_in in (('gan', 4), ('ols', 2)):
        last = last_layer(kind)
        out[f'{kind}_last_w'], out[f'{kind}_last_b'] = last
        out[f'{kind}_checksum'] = np.array(W.net_checksum(shipped[kind]))
        net = AndrewCNN(n_in, 2, div=True)
        net.load_state_dict(state_dict(shipped[kind], last))
        nets[kind] = net.eval()

    rs = np.random.RandomState(4343)
    xs = x_std.reshape(1, 2, 1, 1)

    def record(kind, N, x):
        with torch.no_grad():
            y32 = nets[kind](torch.as_tensor(x)).numpy()
            y64 = copy.deepcopy(nets[kind]).double()(torch.as_tensor(x).double()).numpy()
        assert y32.dtype == np.float32 and y64.dtype == np.float64
        d = y64 - y32.astype(np.float64)
        scale = np.abs(d).max() / 1024.0
        d16 = (d / scale).astype(np.float16)
        rec = y32.astype(np.float64) + d16.astype(np.float64) * scale
        assert np.abs(rec - y64).max() <= 1e-9 * np.abs(y64).max()
        eref = np.abs(y32 - y64).max() / np.abs(y64).max()
        out[f'{kind}_y32_{N}'], out[f'{kind}_d16_{N}'] = y32, d16
        out[f'{kind}_dscale_{N}'], out[f'{kind}_eref_{N}'] = np.array(scale), np.array(eref)
        mean = np.abs(y64.mean(axis=(-2, -1))).max() / np.abs(y64).max()
        print(f'{kind} N={N}: max|y| {np.abs(y64).max():.3g}, e_ref {eref:.2e}, |mean|/max {mean:.1e}')

    q_all = {}
    for N, T in GAN_SIZES.items():
        q = eddy_like_q(rs, T, N, x_std).astype(np.float32)
        q_all[N] = q
        out[f'q{N}'] = q
        X = q / xs                                     # ChannelwiseScaler.normalize on float32
        record('gan', N, np.concatenate([X, latent_noise(N, T)], axis=1))
        if N in OLS_SIZES:
            record('ols', N, X[:OLS_SIZES[N]])

    # CGANRegression(regression='full_loss', div=True): both nets flux-form, from a reference-layout folder
    with tempfile.TemporaryDirectory() as folder:
        torch.save(nets['ols'].state_dict(), os.path.join(folder, 'net_mean.pt'))
        for name, std in (('x_scale.json', x_std), ('y_scale.json', y_std)):
            sc = ChannelwiseScaler()
            sc.std = std.reshape(1, 2, 1, 1)
            sc.mean = np.zeros((1, 2, 1, 1), np.float32)
            sc.write(name, folder=folder)
        model = CGANRegression(regression='full_loss', div=True, folder=folder)      # reads net_mean.pt and the scalers
        model.G.load_state_dict(nets['gan'].state_dict())     # (no G.pt in the folder: load_GAN would ask for the training-only D.pt)
        assert model.G.div and model.net_mean.div

    class _M:
        pass
    for N, T in OLS_SIZES.items():
        z = latent_noise(N, GAN_SIZES[N])
        S = np.empty((T, 2, N, N))
        for t in range(T):
            m = _M()
            m.q = q_all[N][t].astype(np.float64)
            S[t] = model.predict_snapshot(m, z[t:t + 1])
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        out[f'S_{N}'] = S.astype(np.float32)
    path = os.path.join(HERE, 'generator_div.npz')
    np.savez(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
