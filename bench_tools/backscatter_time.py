"""The Jansen-Held backscatter closure on the device (models.BackscatterBiharmonic, qgx_set_backscatter): what it costs.

Microseconds per step of one ensemble with the closure fused (recomputed on the device inside every step) against two
baselines in this one process: the unparameterized step of the same ensemble, and the host plug-in path of the facade
(BackscatterBiharmonic(..., fused=False): per step u, v, ph to the host, a dozen m.fft / m.ifft round trips, S back, one
single-step launch chain) — the only way to run the closure before it was fused, which is taken one member at a time, so
that leg runs with ONE member whatever the shape.  Shapes: 64 x 64 x 128, 64 x 64 x 1, 96 x 96 x 32, 128 x 128 x 16.
Legs alternate, every leg is repeated so that its spread is on record, HIP events around runs of steps that end in a
synchronise, one warm-up run per leg.

    python bench_tools/backscatter_time.py [--out FILE]     (one line per shape; default profiles/backscatter_time.txt)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_tools.visc_time import alternate, eddy_like_q      # noqa: E402

REPS = 3
# (N, members, dt, steps per timed run of a device leg, steps per timed run of the host leg).  A host step costs
# milliseconds (a dozen transforms through numpy and four copies), so 50 of them per run and REPS runs sample it for some
# tenths of a second per shape; its spread is printed beside it like the others
SHAPES = ((64, 128, 14400., 200, 50), (64, 1, 14400., 200, 50), (96, 32, 7200., 200, 50), (128, 16, 7200., 100, 50))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'backscatter_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'backscatter_time.py measures on the GPU'
    from pyqg_generative_amd.qgmodel import QGModel
    from pyqg_generative_amd.models import BackscatterBiharmonic
    cs, cb = float(np.sqrt(0.007)), 1.2
    lines = [f'# {torch.cuda.get_device_name(0)}; us per step of the whole ensemble, best of {REPS} alternating runs '
             '(spread = (max - min) / min); host: the plug-in path with ONE member']
    for N, B, dt, K, Kh in SHAPES:
        q0 = eddy_like_q(np.random.RandomState(N), B, N)
        kw = dict(nx=N, dt=dt, tmax=1e15, tavestart=1e15, twrite=10 ** 9, log_level=0)
        models = {'off': QGModel(n_members=B, **kw),
                  'fused': QGModel(parameterization=BackscatterBiharmonic(cs, cb), n_members=B, **kw),
                  'host': QGModel(parameterization=BackscatterBiharmonic(cs, cb, fused=False), n_members=1, **kw)}
        for name, m in models.items():
            m.q = q0[0] if name == 'host' else (q0[0] if B == 1 else q0)
        t = alternate({name: (lambda m=m, n=(Kh if name == 'host' else K): m._advance(n, refresh_diag=False))
                       for name, m in models.items()}, REPS)
        us = {name: 1e3 * min(t[name]) / (Kh if name == 'host' else K) for name in models}
        row = f'N={N} B={B}'
        for name in models:
            best = min(t[name])
            row += f'  {name}: {us[name]:.1f} us/step (spread {(max(t[name]) - best) / best:.3f})'
        row += f"  fused/off {us['fused'] / us['off']:.2f}  host(B=1)/fused {us['host'] / us['fused']:.1f}x"
        print(row, flush=True)
        lines.append(row)
        for m in models.values():
            m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
