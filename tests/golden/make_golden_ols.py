#!/usr/bin/env python
"""Golden vectors of OLSModel, the deterministic CNN parameterization: imports the reference's own OLSModel
(pyqg_generative/models/ols_model.py) with the inert stubs of make_golden.py, builds it from a reference-layout model folder
written in a temporary directory, and records predict_snapshot(m, 0).

The folder holds GZ's trained net_mean (weights_gz.npz, the same AndrewCNN(2, 2) architecture) as net.pt, GZ's scalers as
x_scale.json / y_scale.json written by the reference's ChannelwiseScaler, and model_args.json from save_model_args.  The
weights are not stored again: ols.npz holds their checksum (pyqg_generative_amd.weights.net_checksum).

Writes ols.npz: q{N} (T, 2, N, N) seeded eddy-like PV and S{N} (T, 2, N, N) forcing for N = 48, 64, 96 (two snapshots each),
x_std, y_std and weights_checksum.  Both are stored as float32 without loss: predict_snapshot reads q as float32 (q here is
rounded to float32 before it is used) and its forcing is a float32 product cast to float64.

Run:  python tests/golden/make_golden_ols.py      (build machine, with the reference checked out)
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

SIZES = {48: 2, 64: 2, 96: 2}


def eddy_like_q(rs, T, N, x_std):
    """band-limited random PV (wavenumbers below 2/3 of the largest) with the amplitude of the training data: every layer of
    every snapshot scaled to the standard deviation x_std of that layer (q / x_std has unit variance, as x_scale defines it)"""
    q = rs.randn(T, 2, N, N)
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    q = np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1))
    return q / q.std(axis=(-2, -1), keepdims=True) * np.asarray(x_std, np.float64).reshape(1, 2, 1, 1)


def main():
    install_inert_stubs()
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.cnn_tools import AndrewCNN, ChannelwiseScaler, save_model_args
    from pyqg_generative.models.ols_model import OLSModel
    from pyqg_generative_amd import weights as W

    d = np.load(os.path.join(HERE, 'weights_gz.npz'))
    net = W.net_from_npz(d, 'net0_')
    x_std, y_std = np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32)
    with tempfile.TemporaryDirectory() as folder:
        sd = AndrewCNN(2, 2).state_dict()
        for i in range(8):
            sd[f'conv.{3 * i}.weight'] = torch.as_tensor(net['conv_w'][i])
            sd[f'conv.{3 * i}.bias'] = torch.as_tensor(net['conv_b'][i])
            if i < 7:
                for key, name in (('bn_g', 'weight'), ('bn_b', 'bias'), ('bn_m', 'running_mean'), ('bn_v', 'running_var')):
                    sd[f'conv.{3 * i + 2}.{name}'] = torch.as_tensor(net[key][i])
        torch.save(sd, os.path.join(folder, 'net.pt'))
        for name, std in (('x_scale.json', x_std), ('y_scale.json', y_std)):
            sc = ChannelwiseScaler()
            sc.std = std.reshape(1, 2, 1, 1)
            sc.mean = np.zeros((1, 2, 1, 1), np.float32)
            sc.write(name, folder=folder)
        save_model_args('OLSModel', folder=folder, div=False, batch_norm=True, bias=True, final_activation='None',
                        hidden_channels=[128, 64, 32, 32, 32, 32, 32])
        model = OLSModel(folder=folder)

    class _M:
        pass
    out = {'x_std': x_std, 'y_std': y_std, 'weights_checksum': np.array(W.net_checksum(net))}
    rs = np.random.RandomState(4242)
    for N, T in SIZES.items():
        q = eddy_like_q(rs, T, N, x_std).astype(np.float32).astype(np.float64)
        S = np.empty_like(q)
        for t in range(T):
            m = _M()
            m.q = q[t]
            S[t] = model.predict_snapshot(m, 0)
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        out[f'q{N}'], out[f'S{N}'] = q.astype(np.float32), S.astype(np.float32)
        print(f'N={N}: {T} snapshots, max|S| {np.abs(S).max():.3g}')
    np.savez(os.path.join(HERE, 'ols.npz'), **out)


if __name__ == '__main__':
    main()
