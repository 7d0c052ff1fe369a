"""DeepInversion U-Net generator (unet.hip): forward time with device events after a warm-up, achieved TFLOP/s against
the f32 MFMA peak, the torch-ROCm eval-mode forward of the test-side restatement (tests/unet_restatement.py) on the same
GPU as the yardstick, and the full online step at 64 x 64 with 128 members.

    python bench_tools/unet_time.py [--out FILE]      (one JSON line per measurement; --out also writes them to FILE)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK_TF = 157.3                                  # f32 MFMA peak of the MI355X
GMAC = {48: 0.562, 64: 0.999, 96: 2.248}         # per member, from the layer shapes (MAC)


def gmac(N):
    return GMAC.get(N, 0.999 * (N / 64) ** 2)


def timed(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    import unet_restatement as U
    net = weights.synthetic_unet()
    xs = np.array([7.78e-06, 1.05e-06], np.float32)
    ys = np.array([7.6e-12, 1.66e-13], np.float32)
    gen = qa.Generator('gan', [net], xs, ys)
    sd = U.to_torch(net, 'cuda')
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)
    for N, B in ((64, 1), (64, 32), (64, 128), (96, 32)):
        x = torch.randn(B, 4, N, N, device='cuda')
        ms = timed(lambda: gen.cnn_forward(x))
        tms = timed(lambda: U.forward(sd, x))
        tf = 2 * gmac(N) * 1e9 * B / (ms * 1e-3) / 1e12
        emit(dict(what='forward', N=N, B=B, ms=round(ms, 4), tflops=round(tf, 2), peak_share=round(tf / PEAK_TF, 3),
                  torch_ms=round(tms, 4), speedup_vs_torch=round(tms / ms, 2)))
    N, B, K = 64, 128, 10
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400.)
    rs = np.random.RandomState(0)
    e.set_q(rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None])
    ms = timed(lambda: e.step(K, generator=gen, sampling='AR1', nsteps_decor=1, refresh_diag=False), warmup=1, reps=3)
    emit(dict(what='online_step', N=N, B=B, steps_per_call=K, ms_per_step=round(ms / K, 4),
              ensemble_timesteps_per_s=round(B * K / (ms * 1e-3), 1)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for d in lines:
                f.write(json.dumps(d) + '\n')


if __name__ == '__main__':
    main()
