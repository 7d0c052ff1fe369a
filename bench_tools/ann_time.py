"""ANNModel (the pointwise stencil network, csrc/ann.hip) on the device:
  * forward: qgx_generator_forward (the stencil kernel + the output kernel k_finish) at 64^2 x 128, 96^2 x 32, 48^2 x 128
    and 64^2 x 1, as a share of the 157.3 TF f32 peak in algorithmic FLOPs (2 (s^2 h0 + h0 h1 + h1) per point: 1632 for the
    default net), HIP events around 200 launches, median of 5 runs after a warm-up;
  * online: ensemble-timesteps per second of a 64^2 x 128 run at the bench's cadence (constant sampling, nsteps 1: every
    step recomputes the forcing; diagnostics every ceil(86400 / dt) steps), ANN next to OLS, median of 3 runs;
  * offline: test_offline at 25 runs x 87 snapshots x 64^2, split into predict and the metrics.
Weights: net a of tests/golden/ann.npz (3 x 3, [24, 24]) and GZ's net_mean as the OLS net.

    python bench_tools/ann_time.py [--out FILE] [--forward-only]   (one JSON line per measurement; default
                                                                     FILE profiles/ann_time.jsonl)
--forward-only: the forward launches alone (for a kernel trace of its own: rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import math
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PEAK_F32 = 157.3e12
FORWARD_CASES = ((64, 128), (96, 32), (48, 128), (64, 1))


def timed(fn, warmup=1, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def eddy_like_q(rs, B, N):
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1)) * 3.0


def flops_per_point(net):
    widths = [net['stencil_size'] ** 2] + list(net['hidden']) + [1]
    return 2 * sum(a * b for a, b in zip(widths[:-1], widths[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ann_time.jsonl'))
    ap.add_argument('--forward-only', action='store_true')
    args = ap.parse_args()
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    from ann_restatement import net_from_fixture
    d = np.load(os.path.join(GOLDEN, 'ann.npz'))
    net = net_from_fixture(d, 'a')
    ann = qa.Generator('ann', [net], float(d['x_scale']), float(d['y_scale']))
    box = dict(host=socket.gethostname(), device=torch.cuda.get_device_name(0))
    lines = []

    def emit(row):
        row.update(box)
        print(json.dumps(row), flush=True)
        lines.append(row)

    fpp = flops_per_point(net)
    for N, B in FORWARD_CASES:
        q = torch.as_tensor(eddy_like_q(np.random.RandomState(N + B), B, N)).cuda()
        S = torch.empty_like(q)
        L = 200
        med, lo, hi = timed(lambda: [ann.forward(q, demean=True, out=S) for _ in range(L)])
        us = 1e3 * med / L
        flop = fpp * 2 * B * N * N
        emit(dict(leg='forward', N=N, B=B, launches_per_run=L, us_per_forward=round(us, 2),
                  us_min=round(1e3 * lo / L, 2), us_max=round(1e3 * hi / L, 2), gflop=round(flop / 1e9, 4),
                  frac_f32_peak=round(flop / (us * 1e-6) / PEAK_F32, 4),
                  note='forward = stencil kernel + k_finish (de-mean); share of peak in algorithmic FLOPs'))
    if args.forward_only:
        return

    gz = np.load(os.path.join(GOLDEN, 'weights_gz.npz'))
    ols = qa.Generator('ols', [weights.net_from_npz(gz, 'net0_')], gz['x_std'], gz['y_std'])
    N, B, dt, K = 64, 128, 14400., 120
    q0 = eddy_like_q(np.random.RandomState(7), B, N)
    for kind, gen in (('ann', ann), ('ols', ols)):
        e = qa.EnsembleEngine(nx=N, n_members=B, dt=dt)
        e.set_q(q0)
        e.diag_config(0, int(math.ceil(86400. / dt)))
        run = lambda: e.step(K, generator=gen, sampling='constant', nsteps_decor=1, seed=7, refresh_diag=False)
        med, lo, hi = timed(run, reps=3)
        e.close()
        emit(dict(leg='online', kind=kind, N=N, B=B, steps_per_run=K, us_per_step=round(1e3 * med / K, 2),
                  ensemble_timesteps_per_s=round(B * K / (med * 1e-3), 1),
                  note='constant sampling nsteps 1, diagnostics every ceil(86400/dt) steps, no ph/u/v refresh'))

    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    R, T, N = 25, 87, 64
    rs = np.random.RandomState(3)
    q = np.concatenate([eddy_like_q(rs, T, N)[None] for _ in range(R)]).astype('float32')
    dims = ['run', 'time', 'lev', 'y', 'x']
    ds = xr.Dataset({'q': (dims, q), 'q_forcing_advection': (dims, (rs.randn(R, T, 2, N, N) * 3e-11).astype('float32')),
                     'psi': (dims, (rs.randn(R, T, 2, N, N) * 1e3).astype('float32'))},
                    coords={'time': (('time',), np.arange(T, dtype='float32') * 1000.)})
    model = ANNModel.from_arrays(net, float(d['x_scale']), float(d['y_scale']))
    model.predict(ds)                                   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.predict(ds)
    t1 = time.perf_counter()
    model.test_offline(ds)
    t2 = time.perf_counter()
    emit(dict(leg='test_offline', R=R, T=T, N=N, predict_s=round(t1 - t0, 3), test_offline_s=round(t2 - t1, 3),
              metrics_s=round((t2 - t1) - (t1 - t0), 3),
              note='wall time, host arrays in and out; metrics = test_offline - predict'))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for row in lines:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
