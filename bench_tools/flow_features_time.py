"""The derived flow fields of dataset_smart_read (omega, KE, Ens, Vabs and the plane sums of KE): what one fused call costs.

Milliseconds per evaluation of all five outputs for a whole stack of snapshots already on the device, two legs in this one
process: `fused`, tools.comparison_tools.flow_features (qgx_flow_features, csrc/flow.hip: u and v read once), against
`composed`, the route of the building blocks that existed before it — `_Snapshots.curl` per layer (float64 copies of u and
v, qgx_rfft2 twice, qgx_spec_curl, qgx_irfft2) plus torch elementwise kernels for KE, Vabs, Ens and the sums, in float64 as
the fused kernel computes them.  Shapes: 10 runs x 87 snapshots at 64 x 64 in float32 (the LDS-resident kernel) and
2 x 16 snapshots at 256 x 256 (the batched path).  Legs alternate, every leg is repeated so that its spread is on record,
HIP events around CALLS evaluations that end in a synchronise, one warm-up run per leg.

    python bench_tools/flow_features_time.py [--out FILE]     (one line per shape; default profiles/flow_features_time.txt)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_tools.visc_time import alternate      # noqa: E402

REPS = 5
CALLS = 5
SHAPES = ((10, 87, 64), (2, 16, 256))


def composed(ct, u, v):
    s = ct._Snapshots.__new__(ct._Snapshots)
    s.f, s.N = {'u': u, 'v': v}, u.shape[-1]
    omega = torch.stack([s.curl(0), s.curl(1)], dim=1).reshape(u.shape)
    u64, v64 = u.to(torch.float64), v.to(torch.float64)
    ke = 0.5 * (u64 * u64 + v64 * v64)
    return {'omega': omega, 'KE': ke.to(u.dtype), 'Ens': 0.5 * omega * omega, 'Vabs': torch.sqrt(2 * ke).to(u.dtype),
            'KE_sum': ke.sum(dim=(-2, -1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'flow_features_time.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'flow_features_time.py measures on the GPU'
    from pyqg_generative_amd.tools import comparison_tools as ct
    lines = [f'# {torch.cuda.get_device_name(0)}; ms per evaluation of omega, KE, Ens, Vabs, KE_sum of the whole stack, float32 '
             f'input on the device; best of {REPS} alternating runs of {CALLS} evaluations (spread = (max - min) / min)']
    for R, T, N in SHAPES:
        rs = np.random.RandomState(N)
        u, v = (torch.from_numpy((rs.randn(R, T, 2, N, N) * 0.05).astype('float32')).cuda() for _ in range(2))
        a, b = ct.flow_features(u, v), composed(ct, u, v)
        top = float(b['omega'].abs().max())
        err = float((a['omega'] - b['omega']).abs().max()) / top
        assert err < 1e-11 and torch.allclose(a['KE'], b['KE'], rtol=2e-7, atol=0), err
        del a, b

        def leg(fn):
            def run():
                for _ in range(CALLS):
                    fn(u, v)
            return run
        t = alternate({'fused': leg(ct.flow_features), 'composed': leg(lambda u, v: composed(ct, u, v))}, REPS)
        ms = {name: min(x) / CALLS for name, x in t.items()}
        nbytes = 2 * R * T * N * N * (2 * 4 + 8 + 4 + 8 + 4)          # u, v read once; omega, KE, Ens, Vabs written once
        row = f'N={N} runs={R} snapshots={T} ({2 * R * T} planes)'
        for name, x in t.items():
            row += f'  {name}: {ms[name]:.3f} ms (spread {(max(x) - min(x)) / min(x):.3f})'
        row += f"  composed/fused {ms['composed'] / ms['fused']:.2f}x  fused: {nbytes / ms['fused'] / 1e9:.2f} TB/s of its {nbytes / 1e6:.1f} MB"
        print(row, flush=True)
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
