"""OLSModel (QGX_GEN_OLS) against the CGAN generator: microseconds per online step on the same grid and ensemble, with the
generator's output and next-input kernels folded into the step kernel (genfuse 1) and as kernels of their own (genfuse 0).
In-process, HIP events around runs of steps (constant sampling, nsteps 1: every step recomputes the forcing; no ph, u, v
refresh), best of three runs after a warm-up.  Weights: the shipped CGAN generator and GZ's net_mean (the AndrewCNN(2, 2)
of tests/golden/ols.npz).

    python bench_tools/ols_time.py [--out FILE]      (one JSON line per measurement; default FILE profiles/ols_time.jsonl)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ((64, 1), (64, 128), (96, 32), (48, 64), (128, 16))


def timed(fn, warmup=1, reps=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def eddy_like_q(rs, B, N):
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1)) * 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ols_time.jsonl'))
    args = ap.parse_args()
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    gens = {}
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    gens['gan'] = qa.Generator('gan', nets, xs, ys)
    d = np.load(os.path.join(GOLDEN, 'weights_gz.npz'))
    gens['ols'] = qa.Generator('ols', [weights.net_from_npz(d, 'net0_')], d['x_std'], d['y_std'])
    lines = []
    for N, B in CASES:
        q0 = eddy_like_q(np.random.RandomState(N + B), B, N)
        K = 200 if B <= 16 else 50
        for genfuse in (1, 0):
            row = dict(N=N, B=B, genfuse=genfuse, steps_per_run=K)
            for kind, gen in gens.items():
                e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400. if N <= 64 else 7200.)
                e.set_option('genfuse', genfuse)
                e.set_q(q0)
                run = lambda: e.step(K, generator=gen, sampling='constant', nsteps_decor=1, seed=7, refresh_diag=False)
                ms = timed(run)
                row[f'{kind}_us_per_step'] = round(1e3 * ms / K, 2)
                row['streams'] = e.step_streams(gen)
                e.close()
                why = gen.range_ok()
                assert why is None, why
            row['ols_over_gan'] = round(row['ols_us_per_step'] / row['gan_us_per_step'], 3)
            print(json.dumps(row), flush=True)
            lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for row in lines:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
