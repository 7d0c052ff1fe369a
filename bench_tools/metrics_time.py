"""Online metrics on the GPU (tools/comparison_tools.py, csrc/metrics.hip): times of the exact 1-Wasserstein distance and
of a full diagnostic_differences_Perezhogin, against scipy on one core.

  w1        wasserstein_distance on 128 members x 128 snapshots x 48^2 = 37.7 M float64 values per side, device tensors;
            phases timed with HIP events: keys (qgx_w1_keys, both sides) and sort + merge (qgx_w1_sorted).  Bytes per key
            are what the kernels must move: keys 8 B read + 8 B written; per radix pass 8 B (histogram) + 8 + 8 B
            (scatter) = 24 B, 8 passes; merge 8 B read.  The HBM share is bytes / time / 6.3 TB/s (achievable copy rate).
  scipy     scipy.stats.wasserstein_distance of a 1/8 subsample (4.7 M per side) on one core; the full size is scaled
            by n log n from it (stated as such in the record).
  diag      diagnostic_differences_Perezhogin of two synthetic 128-member datasets (random float32 q, u, v of 128
            snapshots, host numpy as run_simulation returns them; upload included) at 48^2 and 96^2.

  The split of sort + merge by kernel (histogram, scan, scatter, merge) is not timed here: it comes from a run of four
  distances under `rocprofv3 --kernel-trace --stats`, whose records were added to profiles/metrics_time.jsonl
  (phases kernel_trace_*).

    python bench_tools/metrics_time.py [--out FILE]     (one JSON line per measurement; default profiles/metrics_time.jsonl)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
R, T = 128, 128


def events_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out), float(np.median(out))


def bench_w1(emit):
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools import comparison_tools as ct
    n = R * T * 48 * 48
    g = torch.Generator(device='cuda').manual_seed(0)
    u = torch.randn(n, dtype=torch.float64, device='cuda', generator=g)
    v = torch.randn(n, dtype=torch.float64, device='cuda', generator=g) * 1.1 + 0.05

    def keys():
        return (ct._Sample(u, None, _lib.W1_IDENTITY, 64, 1, 1, n, 0, 0),
                ct._Sample(v, None, _lib.W1_IDENTITY, 64, 1, 1, n, 0, 0))
    state = {}

    def do_keys():
        state['ab'] = keys()

    def do_sorted():
        state['out'] = ct._w1(*state['ab'])

    t_keys, _ = events_ms(do_keys)
    # sort + merge: fresh (unsorted) keys before every timed call
    best = []
    for _ in range(6):
        state['ab'] = keys()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        do_sorted()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b))
    t_sorted = min(best[1:])
    t_total, t_med = events_ms(lambda: ct.wasserstein_distance(u, v))
    bytes_keys = 2 * n * 16
    bytes_sort = 2 * n * 8 * 24
    bytes_merge = 2 * n * 8
    est = bytes_sort / HBM * 1e3
    emit(dict(phase='w1_keys', n_per_side=n, ms=round(t_keys, 3), bytes_per_key=16,
              hbm_fraction=round(bytes_keys / (t_keys * 1e-3) / HBM, 3)))
    emit(dict(phase='w1_sort_and_merge', n_per_side=n, ms=round(t_sorted, 3), bytes_per_key=8 * 24 + 8,
              sort_bytes_estimate_GB=round(bytes_sort / 1e9, 2), sort_ms_at_hbm_rate=round(est, 3),
              hbm_fraction=round((bytes_sort + bytes_merge) / (t_sorted * 1e-3) / HBM, 3)))
    emit(dict(phase='w1_total', n_per_side=n, ms_best=round(t_total, 3), ms_median=round(t_med, 3),
              note='wasserstein_distance(u, v) on device tensors: allocation, keys, sort, merge, one .item()'))

    from scipy.stats import wasserstein_distance
    sub = n // 8
    us, vs = u[:sub].cpu().numpy(), v[:sub].cpu().numpy()
    t0 = time.perf_counter()
    ref = wasserstein_distance(us, vs)
    t_sc = time.perf_counter() - t0
    got = ct.wasserstein_distance(us, vs)
    scale = (n * math.log(n)) / (sub * math.log(sub))
    emit(dict(phase='scipy_w1', n_per_side=sub, s=round(t_sc, 3), full_size_s_extrapolated=round(t_sc * scale, 2),
              note='one core, 1/8 subsample; full size scaled by n log n', rel_err_gpu_vs_scipy=abs(got - ref) / abs(ref),
              speedup_full_size=round(t_sc * scale / (t_total * 1e-3), 1)))


def synthetic_dataset(N, seed):
    from pyqg_generative_amd.tools import xr_lite
    g = torch.Generator(device='cuda').manual_seed(seed)
    data = {}
    for name, amp in (('q', 1e-5), ('u', 0.05), ('v', 0.05)):
        data[name] = (('run', 'time', 'lev', 'y', 'x'),
                      (torch.randn((R, T, 2, N, N), generator=g, device='cuda') * amp).cpu().numpy())
    rs = np.random.RandomState(seed)
    NK = N // 2 + 1
    data['KEspec'] = (('run', 'lev', 'l', 'k'), rs.rand(R, 2, N, NK))
    for k in ('KEflux', 'APEflux', 'APEgenspec', 'KEfrictionspec'):
        data[k] = (('run', 'l', 'k'), rs.randn(R, N, NK))
    return xr_lite.Dataset(data)


def bench_diag(emit):
    from pyqg_generative_amd.tools import comparison_tools as ct
    for N in (48, 96):
        d1, d2 = synthetic_dataset(N, 1), synthetic_dataset(N, 2)
        ct.diagnostic_differences_Perezhogin(d1, d2, T=T)      # warm-up (plans, code objects)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            norm, _, _ = ct.diagnostic_differences_Perezhogin(d1, d2, T=T)
            ts.append(time.perf_counter() - t0)
        emit(dict(phase='diagnostic_differences', N=N, members=R, snapshots=T, values_per_feature=R * T * N * N,
                  s_best=round(min(ts), 3), s_median=round(float(np.median(ts)), 3),
                  distrib_score=float(ct.distrib_score(norm)),
                  note='host datasets (upload included), 10 distances + curl FFTs + 4 spectral RMSEs'))
        del d1, d2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_time.jsonl'))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        def emit(rec):
            rec['device'] = torch.cuda.get_device_name(0)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + '\n')
            f.flush()
        bench_w1(emit)
        bench_diag(emit)


if __name__ == '__main__':
    main()
