"""sampling='deterministic' (the mean of M generator realisations per step) on the device: what the fused mode costs.

Three measurements with the shipped CGAN generator at 64 x 64, all in this one process, legs alternating, every leg
repeated so that its spread is on record, HIP events around runs of steps that end in a synchronise, one warm-up run per leg:

  (a) one member, M = 100: the fused device step (QGX_SAMPLING_DETERMINISTIC) against the host-plugin loop the facade took
      before the mode existed — still what a model does whose parameterization is a plain callable: per step q to the host,
      M forwards through predict_mean_snapshot, the mean to the host and back;
  (b) generator evaluations per second of the fused step at 16 members, M = 100, next to Generator.forward on 128 members;
  (c) the chunk (pseudo-members per generator launch: option "mean_chunk") 128, 256, 512 at 1 and 16 members.

    python bench_tools/deterministic_time.py [--out FILE]   (one JSON line per measurement; default profiles/deterministic_time.jsonl)
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
N, M, DT, REPS = 64, 100, 14400., 3


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


def summary(ms, per):
    """best and spread ((max - min) / min) of repeated timings, in microseconds per `per` units"""
    return dict(us=round(1e3 * min(ms) / per, 2), spread=round((max(ms) - min(ms)) / min(ms), 4))


def eddy_like_q(rs, B):
    q = rs.randn(B, 2, N, N) * np.array([8e-6, 1e-6])[None, :, None, None]
    k = np.fft.fftfreq(N) * N
    kk = np.sqrt(k[:, None] ** 2 + k[None, :N // 2 + 1] ** 2)
    return np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * (kk < 2. / 3. * N / 2), s=(N, N), axes=(-2, -1)) * 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deterministic_time.jsonl'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'deterministic_time.py measures on the GPU'
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.stochastic_pyqg import stochastic_QGModel
    nets, xs, ys = weights.load_npz(os.path.join(GOLDEN, 'weights_gan.npz'), 'gan')
    model = CGANRegression.from_arrays(nets, xs, ys)
    gen = model.device_generator()
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    # (a) the facade, one member: the same model object attached directly (fused) and behind a plain callable (host plugin)
    q1 = eddy_like_q(np.random.RandomState(1), 1)[0]
    kw = dict(nx=N, dt=DT, tmax=1e12, log_level=0)
    fused = stochastic_QGModel(dict(kw, parameterization=model), 'deterministic', n_mean=M)
    host = stochastic_QGModel(dict(kw, parameterization=lambda m: model(m)), 'deterministic', n_mean=M)
    for m in (fused, host):
        m.q = q1
    Kf, Kh = 40, 8
    t = alternate({'fused': lambda: fused._advance(Kf, refresh_diag=False), 'host': lambda: host._advance(Kh, refresh_diag=False)})
    f, h = summary(t['fused'], Kf), summary(t['host'], Kh)
    emit(dict(what='a: fused step vs host-plugin loop', N=N, B=1, M=M, fused_us_per_step=f['us'], fused_spread=f['spread'],
              host_us_per_step=h['us'], host_spread=h['spread'], host_over_fused=round(h['us'] / f['us'], 2),
              faster_by_more_than_the_spread=bool(min(t['host']) / Kh > max(t['fused']) / Kf)))
    fused.close()
    host.close()

    # (b) generator evaluations per second: the fused step at 16 members against Generator.forward at 128 members
    B, K, F = 16, 10, 100
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=DT)
    e.set_q(eddy_like_q(np.random.RandomState(2), B))
    q128 = torch.as_tensor(eddy_like_q(np.random.RandomState(3), 128)).cuda()
    z128 = torch.randn((128, 2, N, N), dtype=torch.float32, device='cuda')
    S128 = torch.empty_like(q128)
    gen.check_range = False              # no device-to-host read per launch inside the timed loops; read once below

    def forwards():
        for _ in range(F):
            gen.forward(q128, z128, out=S128)
    t = alternate({'step': lambda: e.step(K, generator=gen, sampling='deterministic', n_mean=M, seed=7, refresh_diag=False),
                   'forward': forwards})
    s, fw = summary(t['step'], K), summary(t['forward'], F)
    step_rate, fwd_rate = B * M / (s['us'] * 1e-6), 128 / (fw['us'] * 1e-6)
    emit(dict(what='b: generator evaluations per second', N=N, B=B, M=M, step_us=s['us'], step_spread=s['spread'],
              step_evals_per_s=round(step_rate), forward128_us=fw['us'], forward128_spread=fw['spread'],
              forward128_evals_per_s=round(fwd_rate), step_over_forward=round(step_rate / fwd_rate, 3)))
    e.close()

    # (c) the chunk
    for B, K in ((1, 40), (16, 10)):
        engines = {}
        for chunk in (128, 256, 512):
            e = qa.EnsembleEngine(nx=N, n_members=B, dt=DT)
            e.set_option('mean_chunk', chunk)
            e.set_q(eddy_like_q(np.random.RandomState(4 + B), B))
            engines[chunk] = e
        t = alternate({c: (lambda e=e: e.step(K, generator=gen, sampling='deterministic', n_mean=M, seed=7, refresh_diag=False))
                       for c, e in engines.items()})
        row = dict(what='c: chunk', N=N, B=B, M=M)
        for c in engines:
            sm = summary(t[c], K)
            row[f'chunk{c}_us_per_step'], row[f'chunk{c}_spread'] = sm['us'], sm['spread']
        row['fastest'] = min(engines, key=lambda c: min(t[c]))
        emit(row)
        for e in engines.values():
            e.close()
    del gen.check_range
    why = gen.range_ok()
    assert why is None, why
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for row in lines:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
