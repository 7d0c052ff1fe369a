"""The generic AndrewCNN engine (csrc/conv_generic.hip) against the templated exact-f32 kernels, on the SHIPPED architecture: the
same net (the shipped CGAN generator) as a handle of qgx_generator_create with precision 0 and as a handle of
qgx_generator_create_arch with force_generic, in one process, alternating.  Both compute the same float32 arithmetic.
Per size: microseconds per layer (the handle's own profiler: HIP events on the launch stream around every launch of that layer) and
per whole forward (qgx_cnn_forward, events around runs of launches), best of five alternating runs after a warm-up, the ratio
generic / templated, and for the 128 -> 64 5x5 layer (2 x 25 x 128 x 64 flop per pixel) the fraction of the 157.3 TF f32 matrix peak.
Also: the online step time (constant sampling, nsteps 1, weight 1e-3) of a thin net, hidden_channels [64, 32, 16, 16, 16, 16, 16]
with seeded weights, beside the shipped net's exact-f32 step time — the number a width study wants.

    python bench_tools/arch_time.py [--out FILE]      (one JSON line per size, appended; default FILE profiles/arch_time.jsonl)
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
CASES = ((64, 128), (64, 1), (96, 32))
THIN = [64, 32, 16, 16, 16, 16, 16]
PEAK_F32_MATRIX = 157.3e12


def run_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def eddy_like_q(rs, B, N):
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1)) * 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'arch_time.jsonl'))
    args = ap.parse_args()
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    gens = {'templated': qa.Generator('gan', nets, xs, ys), 'generic': qa.Generator('gan', nets, xs, ys, force_generic=True),
            'thin': qa.Generator('gan', [weights.synthetic_arch(4, THIN, seed=1)], xs, ys)}
    gens['templated'].set_option('precision', 0)
    for g in gens.values():
        assert g.info()['precision'] == 0
        g.check_range = False
    lines = []
    for N, B in CASES:
        x = torch.randn((B, 4, N, N), dtype=torch.float32, device='cuda')
        K = 100 if B <= 16 else 20
        row = dict(N=N, B=B, launches_per_run=K, device=torch.cuda.get_device_name(0))
        y = {k: gens[k].cnn_forward(x) for k in ('templated', 'generic')}
        row['generic_vs_templated_maxrel'] = float((y['generic'] - y['templated']).abs().max() / y['templated'].abs().max())
        fwd = {k: (lambda g=g: [g.cnn_forward(x) for _ in range(K)]) for k, g in gens.items()}
        for k in gens:
            fwd[k]()
        torch.cuda.synchronize()
        best = {}
        for _ in range(5):
            for k in gens:                     # alternating
                best[k] = min(best.get(k, float('inf')), run_ms(fwd[k]))
        for k in gens:
            row[f'forward_{k}_us'] = round(1e3 * best[k] / K, 2)
        row['forward_generic_over_templated'] = round(row['forward_generic_us'] / row['forward_templated_us'], 3)
        row['forward_thin_over_templated'] = round(row['forward_thin_us'] / row['forward_templated_us'], 3)
        layers = {}
        for layer in range(8):
            t = {}
            for k in ('templated', 'generic'):
                g = gens[k]
                g.profile(layer)
                bestl = float('inf')
                for _ in range(3):
                    for _ in range(10):
                        g.cnn_forward(x)
                    ms, n = g.profile_read()
                    bestl = min(bestl, 1e3 * ms / max(n, 1))
                g.profile(-1)
                t[k] = round(bestl, 2)
            t['ratio'] = round(t['generic'] / t['templated'], 3)
            layers[str(layer + 1)] = t
        row['layer_us'] = layers
        flop2 = 2.0 * 25 * 128 * 64 * B * N * N
        for k in ('templated', 'generic'):
            row[f'layer2_{k}_fraction_of_f32_matrix_peak'] = round(flop2 / (layers['2'][k] * 1e-6) / PEAK_F32_MATRIX, 3)
        q0 = eddy_like_q(np.random.RandomState(N + B), B, N)
        engines = {}
        for k in gens:
            e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400. if N <= 64 else 7200.)
            e.set_q(q0)
            engines[k] = e
        step = {k: (lambda k=k: engines[k].step(K, generator=gens[k], sampling='constant', nsteps_decor=1, seed=7, weight=1e-3,
                                                refresh_diag=False)) for k in gens}
        for k in gens:
            step[k]()
        torch.cuda.synchronize()
        best = {}
        for _ in range(5):
            for k in gens:
                engines[k].set_q(q0)
                best[k] = min(best.get(k, float('inf')), run_ms(step[k]))
        for k in gens:
            row[f'step_{k}_us'] = round(1e3 * best[k] / K, 2)
            engines[k].close()
        row['step_thin_over_templated'] = round(row['step_thin_us'] / row['step_templated_us'], 3)
        row['step_generic_over_templated'] = round(row['step_generic_us'] / row['step_templated_us'], 3)
        print(json.dumps(row), flush=True)
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        for row in lines:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
