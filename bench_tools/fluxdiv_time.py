"""The flux head of AndrewCNN(div=True) against the plain head: the SAME layers 1-7 (the shipped CGAN generator) with a two-channel
last layer and with a four-channel one followed by the divergence kernel (csrc/fluxdiv.hip), in one process, alternating.
Per case: microseconds per generator forward (qgx_cnn_forward, HIP events around runs of launches) and per online step
(constant sampling, nsteps 1: every step recomputes the forcing; weight 1e-3; no ph, u, v refresh), best of five alternating runs after a
warm-up; the difference of the forward times is the cost of the second last-layer launch, the unfused (7, 8) pair and the
divergence kernel together.  Bytes the divergence kernel must move: 4 + 2 fields of 4 N^2 bytes per member.

    python bench_tools/fluxdiv_time.py [--out FILE]      (one JSON line per case; default FILE profiles/fluxdiv_time.jsonl)
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
CASES = ((64, 128), (96, 32), (64, 1), (128, 16))


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fluxdiv_time.jsonl'))
    args = ap.parse_args()
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    flux = dict(nets[0])
    rs = np.random.RandomState(501)
    flux['conv_w'] = list(nets[0]['conv_w'][:7]) + [(rs.randn(4, 32, 3, 3) / np.sqrt(32 * 9)).astype(np.float32)]
    flux['conv_b'] = list(nets[0]['conv_b'][:7]) + [(0.1 * rs.randn(4)).astype(np.float32)]
    gens = {'plain': qa.Generator('gan', nets, xs, ys), 'flux': qa.Generator('gan', [flux], xs, ys)}
    lines = []
    for N, B in CASES:
        q0 = eddy_like_q(np.random.RandomState(N + B), B, N)
        x = torch.randn((B, 4, N, N), dtype=torch.float32, device='cuda')
        K = 200 if B <= 16 else 50
        row = dict(N=N, B=B, launches_per_run=K, layer2_kernel={k: g.layer2_kernel(B, N) for k, g in gens.items()},
                   fluxdiv_bytes=6 * 4 * N * N * B)
        engines = {}
        for kind, gen in gens.items():
            e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400. if N <= 64 else 7200.)
            e.set_q(q0)
            engines[kind] = e
        fwd = {k: (lambda g=g: [g.cnn_forward(x) for _ in range(K)]) for k, g in gens.items()}
        for k, g in gens.items():
            g.check_range = False              # no device-to-host read between the timed launches
        # (weight 1e-3 and a fresh state per run: the seeded last layer is not a trained closure, and a run must stay finite)
        step = {k: (lambda k=k: engines[k].step(K, generator=gens[k], sampling='constant', nsteps_decor=1, seed=7,
                                                weight=1e-3, refresh_diag=False)) for k in gens}
        best = {}
        for name, fns in (('forward', fwd), ('step', step)):
            for k in gens:
                fns[k]()                       # warm-up of every shape timed below
            torch.cuda.synchronize()
            for _ in range(5):
                for k in gens:                 # alternating
                    engines[k].set_q(q0)
                    best[name, k] = min(best.get((name, k), float('inf')), run_ms(fns[k]))
            for k in gens:
                row[f'{name}_{k}_us'] = round(1e3 * best[name, k] / K, 2)
            row[f'{name}_flux_minus_plain_us'] = round(row[f'{name}_flux_us'] - row[f'{name}_plain_us'], 2)
            row[f'{name}_flux_over_plain'] = round(row[f'{name}_flux_us'] / row[f'{name}_plain_us'], 4)
        for k, g in gens.items():
            del g.check_range
            why = g.range_ok()
            assert why is None, why
            engines[k].close()
        print(json.dumps(row), flush=True)
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for row in lines:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
