#!/usr/bin/env python
"""Golden vectors of AndrewCNN nets of other architectures than the shipped one: imports the reference's own AndrewCNN, CVAERegression
and OLSModel (pyqg_generative/tools/cnn_tools.py:125-176, models/cvae_regression.py, models/ols_model.py) with the inert stubs of
make_golden.py and the grid-line stub of make_golden_div.py, and runs them with torch on the CPU.

The cases (tests/arch_restatement.py::CASES) take their weights from pyqg_generative_amd.weights.synthetic_arch — seeded, NOT stored;
the fixture holds weights.net_checksum of each.  Inputs as in make_golden_div.py: band-limited PV of the training amplitude (stored as
float32, normalised by x_std), white latent noise regenerated from RandomState(z_seed + N).

  q{N}                       (T, 2, N, N) float32 PV, N = 16, 48, 64
  {case}_checksum            weights.net_checksum of the case's net
  {case}_y32_{N}             float32 forward of AndrewCNN(n_in, 2, batch_norm=, bias=, div=, hidden_channels=)
  {case}_d16_{N}, {case}_dscale_{N}   the float64 forward as y64 = y32 + d16 * dscale
  {case}_eref_{N}            max|y32 - y64| / max|y64|
  vae_S_16                   CVAERegression(hidden_channels=A's).predict_snapshot on q16 with the latent noise of size 16
  ols_S_16                   OLSModel(hidden_channels=B's, batch_norm=False, bias=False).predict_snapshot on q16
both built through the reference's classes from a temporary folder; stored as float32 without loss.

Run:  python tests/golden/make_golden_arch.py      (build machine, with the reference checked out)
"""
import copy
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_inert_stubs, REF  # noqa: E402
from make_golden_div import install_grid_stub  # noqa: E402
from make_golden_ols import eddy_like_q  # noqa: E402
import arch_restatement as AR  # noqa: E402


def main():
    install_inert_stubs()
    install_grid_stub()
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.cnn_tools import AndrewCNN
    from pyqg_generative.models.cvae_regression import CVAERegression
    from pyqg_generative.models.ols_model import OLSModel
    from pyqg_generative_amd import weights as W

    x_std, y_std = AR.scales()
    out = {'x_std': x_std, 'y_std': y_std, 'z_seed': np.array(AR.Z_SEED)}
    rs = np.random.RandomState(4444)
    sizes = {}
    for c in AR.CASES.values():
        for N, T in c['sizes'].items():
            sizes[N] = max(sizes.get(N, 0), T)
    for N in sorted(sizes):
        out[f'q{N}'] = eddy_like_q(rs, sizes[N], N, x_std).astype(np.float32)
    xs = x_std.reshape(1, 2, 1, 1)

    def torch_sd(net):
        return {k: torch.as_tensor(v) for k, v in W.state_dict_from_net(net).items()}

    for name, c in AR.CASES.items():
        net = AR.case_net(name)
        out[f'{name}_checksum'] = np.array(W.net_checksum(net))
        ref = AndrewCNN(c['n_in'], 2, batch_norm=c['batch_norm'], bias=c['bias'], div=c['div'], hidden_channels=c['hidden_channels'])
        ref.load_state_dict(torch_sd(net), strict=False)        # (strict=False: num_batches_tracked is not in the dict)
        got = {k for k in ref.state_dict() if not k.endswith('num_batches_tracked')}
        assert got == set(W.state_dict_from_net(net)), got ^ set(W.state_dict_from_net(net))
        ref.eval()
        for N, T in c['sizes'].items():
            X = out[f'q{N}'][:T] / xs
            x = np.concatenate([X, AR.latent_noise(N, T)], axis=1) if c['n_in'] == 4 else X
            with torch.no_grad():
                y32 = ref(torch.as_tensor(x)).numpy()
                y64 = copy.deepcopy(ref).double()(torch.as_tensor(x).double()).numpy()
            assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == (T, 2, N, N)
            d = y64 - y32.astype(np.float64)
            scale = np.abs(d).max() / 1024.0
            d16 = (d / scale).astype(np.float16)
            assert np.abs(y32.astype(np.float64) + d16.astype(np.float64) * scale - y64).max() <= 1e-9 * np.abs(y64).max()
            eref = np.abs(y32 - y64).max() / np.abs(y64).max()
            out[f'{name}_y32_{N}'], out[f'{name}_d16_{N}'] = y32, d16
            out[f'{name}_dscale_{N}'], out[f'{name}_eref_{N}'] = np.array(scale), np.array(eref)
            print(f'{name} N={N}: max|y| {np.abs(y64).max():.3g}, e_ref {eref:.2e}')

    class _M:
        pass
    N, T = 16, 2
    z = AR.latent_noise(N, T)
    a, b = AR.CASES['A'], AR.CASES['B']
    with tempfile.TemporaryDirectory() as folder:
        AR.write_folder(folder, 'vae', [AR.case_net('A')])
        torch.save(AndrewCNN(4, 4).state_dict(), os.path.join(folder, 'encoder.pt'))     # load_model reads nothing without it
        model = CVAERegression(folder=folder, hidden_channels=a['hidden_channels'])
        model.decoder.eval()
        S = np.empty((T, 2, N, N))
        for t in range(T):
            m = _M()
            m.q = out[f'q{N}'][t].astype(np.float64)
            S[t] = model.predict_snapshot(m, z[t:t + 1])
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        out['vae_S_16'] = S.astype(np.float32)
    with tempfile.TemporaryDirectory() as folder:
        AR.write_folder(folder, 'ols', [AR.case_net('B')])
        model = OLSModel(folder=folder, hidden_channels=b['hidden_channels'], batch_norm=False, bias=False)
        S = np.empty((T, 2, N, N))
        for t in range(T):
            m = _M()
            m.q = out[f'q{N}'][t].astype(np.float64)
            S[t] = model.predict_snapshot(m, 0)
        assert np.array_equal(S.astype(np.float32).astype(np.float64), S)
        out['ols_S_16'] = S.astype(np.float32)
    path = os.path.join(HERE, 'generator_arch.npz')
    np.savez(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    main()
