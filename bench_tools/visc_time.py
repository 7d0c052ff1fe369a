"""Molecular viscosity (models.Laplace, qgx_set_viscosity) in the step kernels: what the term costs.

Steps per second of one ensemble with the term off, on (fused: evaluated inside the step kernels) and through the host
plug-in path of the facade (Laplace(..., fused=False): per step qh and ph to the host, numpy, an inverse transform, S back,
one single-step launch chain), at 64 x 64 x 128 members and 256 x 256 x 64 members.  All in this one process, legs
alternating, every leg repeated so that its spread is on record, HIP events around runs of steps that end in a
synchronise, one warm-up run per leg.  At 256 x 256 "off" runs the single-launch run kernel where the device has one and
"fused" the three-launch step (the viscous run kernel did not fit its registers), so a fourth leg
runs the inviscid model on three launches too (option team = 0).

    python bench_tools/visc_time.py [--out FILE]     (one line per shape; default profiles/visc_time.txt)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, NU = 3, 50.
SHAPES = ((64, 128, 14400., 200, 4), (256, 64, 3600., 40, 2))      # N, members, dt, steps per timed run (device legs / host leg)


def run_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(legs, reps=REPS):
    """legs: {name: callable} -> {name: [ms per repeat]}: one warm-up of every leg, then the legs in turn, `reps` times"""
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            out[name].append(run_ms(fn))
    return out


def eddy_like_q(rs, B, N):
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1)) * 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visc_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'visc_time.py measures on the GPU'
    from pyqg_generative_amd.qgmodel import QGModel
    from pyqg_generative_amd.models import Laplace
    lines = [f'# {torch.cuda.get_device_name(0)}; steps/s of the whole ensemble, best of {REPS} alternating runs (spread = (max - min) / min)']
    for N, B, dt, K, Kh in SHAPES:
        q0 = eddy_like_q(np.random.RandomState(N), B, N)
        kw = dict(nx=N, dt=dt, tmax=1e15, tavestart=1e15, twrite=10 ** 9, log_level=0, n_members=B)
        models = {'off': QGModel(**kw), 'fused': QGModel(parameterization=Laplace(NU), **kw),
                  'host': QGModel(parameterization=Laplace(NU, fused=False), **kw)}
        if N == 256:      # the inviscid model on the path the viscous one takes: what the term costs, apart from the run kernel
            models['off, three launches'] = QGModel(**kw)
            models['off, three launches']._eng.set_option('team', 0)
        for m in models.values():
            m.q = q0
        t = alternate({name: (lambda m=m, n=(Kh if name == 'host' else K): m._advance(n, refresh_diag=False))
                       for name, m in models.items()})
        row = f'N={N} B={B}'
        for name in models:
            n = Kh if name == 'host' else K
            best = min(t[name])
            row += f'  {name}: {1e3 * n / best:.1f} steps/s (spread {(max(t[name]) - best) / best:.3f})'
        row += f"  fused/off {min(t['off']) / min(t['fused']):.3f}  fused/host {(min(t['host']) / Kh) / (min(t['fused']) / K):.1f}x"
        row += f"  run kernel state of 'off': {models['off']._eng.run_kernel_state}"
        print(row, flush=True)
        lines.append(row)
        for m in models.values():
            m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
