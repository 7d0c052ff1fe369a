"""Offline metrics on the GPU (tools/computational_tools.py, csrc/offline.hip): the metric phase of
Parameterization.test_offline at the reference's test-split size, 25 runs x 87 snapshots x 2 layers x 64^2, against
predict and against the test-side numpy restatement on the host.

  metrics   offline_dataset(ds, preds) on synthetic seeded fields (float32 truth, q and psi as in the dataset, float64
            sample and mean as predict returns them), split into upload, transforms (qgx_rfft2), densities
            (qgx_offline_spectra + finish), moments (qgx_offline_moments), histograms (qgx_histogram) and host (residual
            fields, isotropic binning, dataset assembly, float32 cast); each phase boundary synchronises the device.
  predict   CGANRegression.predict of the shipped GAN weights at M = --members (default 50), scaled linearly to M = 1000.
  numpy     tests/offline_restatement.py::test_offline on the same fields (one host process).
  bytes     algorithmic bytes of the density and moment kernels, for their HBM share (kernel times from a separate
            `rocprofv3 --kernel-trace --stats` run of `--kernels`): densities read the four spectra once (16 B per complex
            value); moments read truth and mean in pass 1 and truth, mean and sample in pass 2.

    python bench_tools/offline_time.py [--out FILE] [--members M] [--no-numpy]
    python bench_tools/offline_time.py --kernels      (5 x the density and moment launches, for rocprofv3)
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R, T, N = 25, 87, 64
HBM = 6.3e12


def fields(seed=0):
    rs = np.random.RandomState(seed)
    shape = (R, T, 2, N, N)
    q = (rs.randn(*shape) * 5e-6).astype('float32')
    true = (rs.randn(*shape) * 3e-11).astype('float32')
    psi = (rs.randn(*shape) * 1e3).astype('float32')
    mean = 0.7 * true + 1e-11 * rs.randn(*shape)
    gen = mean + 2e-11 * rs.randn(*shape)
    var = np.full(shape, 4e-22)
    return q, true, psi, mean, gen, var


def datasets(q, true, psi, mean, gen, var):
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    dims = ['run', 'time', 'lev', 'y', 'x']
    ds = xr.Dataset({'q': (dims, q), 'q_forcing_advection': (dims, true), 'psi': (dims, psi)},
                    coords={'time': (('time',), np.arange(T, dtype='float32'))})
    preds = xr.Dataset({'q_forcing_advection': (dims, gen), 'q_forcing_advection_mean': (dims, mean),
                        'q_forcing_advection_var': (dims, var)})
    return ds, preds


def kernel_bytes(true, mean, gen):
    S, P = R * T, N * (N // 2 + 1)
    dens = S * 2 * 4 * P * 16 + 2 * 22 * P * 8
    n = true.size
    mom = n * (true.itemsize + mean.itemsize) + n * (true.itemsize + mean.itemsize + gen.itemsize)
    return dens, mom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'offline_time.jsonl'))
    ap.add_argument('--members', type=int, default=50)
    ap.add_argument('--no-numpy', action='store_true')
    ap.add_argument('--kernels', action='store_true')
    args = ap.parse_args()
    from pyqg_generative_amd.tools import computational_tools as ct
    q, true, psi, mean, gen, var = fields()

    if args.kernels:
        td, md, gd, pd = (torch.from_numpy(x).cuda() for x in (true, mean, gen, psi))
        for _ in range(5):
            ct.spectra_sums(td, md, gd, pd)
            ct.moment_sums(td, md, gd)
        torch.cuda.synchronize()
        dens, mom = kernel_bytes(true, mean, gen)
        print(json.dumps({'kernels': 5, 'density_bytes': dens, 'moment_bytes': mom}))
        return

    recs = []
    ds, preds = datasets(q, true, psi, mean, gen, var)
    ct.offline_dataset(ds, preds)                       # warm-up: plans, code objects
    torch.cuda.synchronize()
    best = None
    for _ in range(3):
        tm = {}
        t0 = time.perf_counter()
        ct.offline_dataset(ds, preds, timings=tm)
        tm['total'] = time.perf_counter() - t0
        if best is None or tm['total'] < best['total']:
            best = tm
    recs.append({'phase': 'metrics', 'shape': [R, T, 2, N, N], **{k: round(v, 4) for k, v in best.items()}})

    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression
    nets, xs, ys = weights.load_npz(os.path.join(ROOT, 'tests', 'golden', 'weights_gan.npz'), 'gan')
    model = CGANRegression.from_arrays(nets, xs, ys)
    model.predict(ds, 2, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict(ds, args.members, seed=1)
    torch.cuda.synchronize()
    tp = time.perf_counter() - t0
    recs.append({'phase': 'predict', 'members': args.members, 'seconds': round(tp, 3),
                 'seconds_scaled_to_1000': round(tp * 1000 / args.members, 2),
                 'metric_share_of_predict_1000': round(best['total'] / (tp * 1000 / args.members), 4)})

    if not args.no_numpy:
        spec = importlib.util.spec_from_file_location('offline_restatement',
                                                      os.path.join(ROOT, 'tests', 'offline_restatement.py'))
        rst = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(rst)
        t0 = time.perf_counter()
        rst.test_offline(true, mean, gen, psi)
        recs.append({'phase': 'numpy_restatement', 'seconds': round(time.perf_counter() - t0, 2)})

    dens, mom = kernel_bytes(true, mean, gen)
    recs.append({'phase': 'algorithmic_bytes', 'densities': dens, 'moments': mom,
                 'densities_ms_at_hbm': round(dens / HBM * 1e3, 4), 'moments_ms_at_hbm': round(mom / HBM * 1e3, 4)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for r in recs:
            print(json.dumps(r))
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
