#!/usr/bin/env python
"""Headline benchmark: ensemble-timesteps/sec of the online parameterized-QG loop
(64x64 two-layer eddy configuration + CGAN subgrid parameterization; BASELINE.json `metric`).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" advances every resident ensemble member by one model time step: latent-noise draw
(Philox), generator forward (8 conv layers on the matrix cores), per-layer de-mean, and the
pseudo-spectral step (packed complex FFTs, inversion, advection, friction, AB3 + exponential
filter) in float64.  The timed region is the reference's loop (tools/simulate.py:137-139) at the
reference's cadences: time-averaged spectral diagnostics every ceil(86400/dt) steps,
a snapshot (q, u, v, psi -> float32 on the host) every ceil(3.6e6/dt) steps, the KE/CFL status
check every 1000 steps, and — at snapshot time — the ensemble-mean KE spectrum (the ONE collective
of the path: an all-reduce of per-rank partial sums).  Members are sharded over ranks with no
data-path collective (weak scaling: --members per GPU is fixed; 128/GPU = BASELINE configs[2]'s
1024 members on 8 GPUs).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline line (with the roofline of the HIP events
inside the timed region).  --dump-outputs DIR then writes what the timed loop computed in its last step (dump_outputs).

--full adds the auxiliary legs on one GPU (same JSON line), each with its OWN fixed protocol, independent of --steps:
`steady` (the headline workload under SURVEY §8d's protocol: 100 warm-up + 2,000 timed steps, 8 snapshots and 2 status
checks inside, >= 200 event-bracketed launches of the roofline kernel), `exact_f32` (the same workload on the f32 matrix
cores), `b1` (configs[1]: one member), `b1024` (configs[2] WHOLE on one GPU: 1024 members, the one-workgroup-per-member
step kernel), `config3` (96x96 jet + CVAE, 32 members = configs[3]'s per-GPU shard), `config4` (256x256
unparameterized, 64 members: 1000 steps = one snapshot interval of a forcing-dataset run, pyqg's time-averaged
diagnostics every 24 steps in the second half, ONE coarse-grain + subgrid-forcing diagnostic to 64x64, all timed),
`cpu_baseline` (the CPU oracle on this box's host cores).

    --total-members M    strong scaling: ONE M-member ensemble split over the ranks (M / world each)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MAC_PER_PIXEL = [12800, 204800, 18432, 9216, 9216, 9216, 9216, 576]   # SURVEY §8(d), GAN/VAE nets
F32_MFMA_PEAK_TFLOPS = 157.3                                           # MI355X_MICROARCH.md, dense f32 matrix
F16_MFMA_PEAK_TFLOPS = 2500.0                                          # dense f16/bf16, same guide
HBM_PEAK_GBS = 8000.0                                                  # HBM3E, same guide
DUMP_BYTES = 64_000_000                                                # --dump-outputs: at most this much in all
PRECISIONS = {'f32': 0, 'f16x3': 3}
JET = dict(rek=7e-8, delta=0.1, beta=1e-11)                            # tools/parameters.py:26-27,37


def dt_of(N):
    return 14400. if N <= 64 else (7200. if N <= 128 else 3600.)      # tools/parameters.py:12-31


def eddy_like_q(member_ids, N):
    """Seeded synthetic PV fields with spun-up eddy amplitudes (SURVEY §8d 'value distributions'):
    white noise band-limited to 2/3 of the Nyquist wavenumber, std ~ x_scale."""
    k = np.fft.rfftfreq(N, 1.0 / N)
    l = np.fft.fftfreq(N, 1.0 / N)
    mask = np.sqrt(k[None, :] ** 2 + l[:, None] ** 2) < (2. / 3.) * (N // 2)
    out = np.empty((len(member_ids), 2, N, N))
    for i, mid in enumerate(member_ids):
        rs = np.random.RandomState(int(mid))
        q = rs.randn(2, N, N) * np.array([8e-6, 1e-6])[:, None, None]
        out[i] = np.fft.irfftn(np.fft.rfftn(q, axes=(-2, -1)) * mask, axes=(-2, -1)) * 3.0
    return out


def load_generator(kind, device):
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    fixture = os.path.join(ROOT, 'tests', 'golden', f'weights_{kind}.npz')
    if os.path.exists(fixture):
        nets, xs, ys = weights.load_npz(fixture, kind)
        src = 'pretrained fixture (reference Google-Colab weights)'
    else:
        nets, xs, ys = weights.synthetic(kind)
        src = 'seeded random-init'
    return qa.Generator(kind, nets, xs, ys, device=device), src


class OnlineLoop:
    """The reference's run loop around qgx_step: chunks of steps between cadence boundaries."""

    def __init__(self, eng, dt, step_kw, dist=None, backend='nccl'):
        from pyqg_generative_amd import _lib
        self.L = _lib
        self.eng, self.step_kw, self.dist, self.backend = eng, step_kw, dist, backend
        self.snap_every = int(math.ceil(3.6e6 / dt))          # ANDREW_1000_STEPS (parameters.py:9)
        self.status_every = 1000                               # pyqg twrite
        eng.diag_config(0, int(math.ceil(86400. / dt)))       # pyqg taveint (averaging phase of a run)
        B, N = eng.B, eng.N
        self.host = torch.empty((4, B, 2, N, N), dtype=torch.float32).pin_memory()
        self.nsnap = self.nstatus = 0
        self.mean_spec = None

    def snapshot(self):
        e, L = self.eng, self.L
        for i, f in enumerate((L.F_Q, L.F_U, L.F_V, L.F_P)):
            self.host[i].copy_(e.get(f).to(torch.float32), non_blocking=True)
        # ensemble-mean KE spectrum over ALL members of the job (comparison_tools.py:167-168)
        from pyqg_generative_amd import parallel
        local = e.diag('KEspec').sum(0)
        if self.dist is not None and self.backend == 'gloo':
            local = local.cpu()
        self.mean_spec = parallel.ensemble_mean(local, e.B)
        torch.cuda.current_stream().synchronize()
        self.nsnap += 1

    def rehearse(self):
        """warm-up only (not steps, never inside a timed region): one snapshot and one status check, so that their one-time
        costs (first device-to-host copies into the pinned buffer, the collective's first call, lazily created work fields of
        qgx_get(QGX_F_P) / qgx_status) are not charged to whichever leg of a process happens to run first"""
        n = (self.nsnap, self.nstatus)
        if self.eng.diag_count > 0:               # (every rank takes the same branch: the increments follow the step count)
            self.snapshot()
        else:                                     # --warmup 0: nothing averaged yet, the field copies alone
            for i, f in enumerate((self.L.F_Q, self.L.F_U, self.L.F_V, self.L.F_P)):
                self.host[i].copy_(self.eng.get(f).to(torch.float32), non_blocking=True)
            torch.cuda.current_stream().synchronize()
        self.eng.status()
        self.nsnap, self.nstatus = n

    def run(self, n):
        e = self.eng
        done = 0
        tc = e.tc
        while done < n:
            chunk = min(n - done, self.snap_every - tc % self.snap_every, self.status_every - tc % self.status_every)
            e.step(chunk, **self.step_kw)
            done += chunk
            tc += chunk
            if tc % self.status_every == 0:
                ke, cfl = e.status()
                assert np.isfinite(ke).all() and (cfl < 1).all(), 'CFL condition violated'
                self.nstatus += 1
            if tc % self.snap_every == 0:
                self.snapshot()


def dump_outputs(eng, first, outdir):
    """--dump-outputs: the state the timed loop leaves after its last step, as its caller receives it (float64, members x
    layers x N x N): PV `q`, velocities `u` / `v`, streamfunction `psi` and `s`, the generator's subgrid forcing of that
    step.  An ensemble too large for DUMP_BYTES is written as a fixed seeded sample of its members; `members` holds their
    global ids (float64)."""
    from pyqg_generative_amd import _lib
    fields = {'q': _lib.F_Q, 'u': _lib.F_U, 'v': _lib.F_V, 'psi': _lib.F_P, 's': _lib.F_S}
    B, N = eng.B, eng.N
    keep = min(B, (DUMP_BYTES - 8 * B - 4096) // (len(fields) * 2 * N * N * 8))      # 4096: the .npy headers
    idx = np.arange(B) if keep == B else np.sort(np.random.RandomState(0).choice(B, keep, replace=False))
    sel = torch.as_tensor(idx, device=eng.device)
    os.makedirs(outdir, exist_ok=True)
    for name, f in fields.items():
        np.save(os.path.join(outdir, name + '.npy'), eng.get(f)[sel].cpu().numpy())
    np.save(os.path.join(outdir, 'members.npy'), (first + idx).astype(np.float64))


def timed(fn, barrier=lambda: None):
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    barrier()
    return time.perf_counter() - t0


def prof_stride(K):
    """HIP events around every n-th launch of the roofline kernel (a pair idles the GPU for ~12 us): every 10th in a
    long run, denser in a short one so that even the driver's 20-step run brackets 10 launches"""
    return 10 if K >= 1000 else (5 if K >= 200 else 2)


def layer2_kernel(gen, precision, N, B):
    """(name of the kernel that runs generator layer 2 for this generator / shard, executed f16 MFMA flops per algorithmic flop):
    asked of the library (qgx_generator_layer2_kernel), which applies its own crossovers"""
    k = gen.layer2_kernel(B, N)
    if k == 0:
        return 'k_conv<128,64,5x5>', None
    if k == 4:
        return 'k_convw2 (1-D Winograd F(4,5) along x, f16x3, input transform under the MFMAs)', 3 * 0.4
    if k == 3:
        return 'k_convw (1-D Winograd F(4,5) along x, f16x3)', 3 * 0.4
    if k == 2:
        return 'k_convh2<128,64,5x5,PART> (25 taps, split-K, f16x3)', 3.0
    return 'k_convh2<128,64,5x5> (25 taps, f16x3)', 3.0


def mfma_roofline(gen, precision, N, B, kname, traffic, stride=10, executed_per_flop=3.0):
    """roofline object of the dominant kernel (generator layer 2: 75 % of the FLOPs) from the HIP events the
    library recorded around its launches inside the timed region.  B = members PER LAUNCH (half of the resident
    ensemble when qgx_step advances it as two halves on two streams, EnsembleEngine.step_streams)"""
    ms, n = gen.profile_read()
    gen.profile(-1)
    flop = 2.0 * MAC_PER_PIXEL[1] * N * N * B
    avg_s = (ms / max(n, 1)) * 1e-3
    achieved = flop / avg_s / 1e12 if avg_s > 0 else 0.0
    peak = F32_MFMA_PEAK_TFLOPS if precision == 'f32' else F16_MFMA_PEAK_TFLOPS
    r = {'bound': 'mfma', 'kernel': kname, 'achieved': achieved, 'peak': peak, 'unit': 'TFLOP/s',
         'frac': achieved / peak, 'traffic': traffic, 'flop_per_launch': flop, 'avg_launch_ms': avg_s * 1e3,
         'members_per_launch': B,
         'launches_timed': n, 'launches_timed_note': f'HIP events bracket every {stride}th launch of the timed region',
         'peak_note': ('dense f32 MFMA peak; ALGORITHMIC flops (2 x 204,800 MAC/px x N^2 x B per launch)' if precision == 'f32'
                       else 'dense f16 MFMA peak; `achieved` counts ALGORITHMIC flops (2 x 204,800 MAC/px x N^2 x B per launch)')}
    if precision == 'f16x3':
        r['mfma_pipe_frac'] = executed_per_flop * achieved / peak
        r['mfma_pipe_note'] = ('f16x3 executes three f16 MFMAs per multiply-add (hi*hi + hi*lo + lo*hi); the 1-D Winograd form of the '
                               f'5x5 layer multiplies 0.4 x as often as the 25-tap form: executed MFMA flops = {executed_per_flop:.1f} x achieved')
    return r


def pmc_traffic(name, cfg):
    """HBM bytes per launch of the roofline kernel: cannot be measured from inside this process, comes from
    the committed rocprofv3 PMC passes (profiles/, FETCH_SIZE x2 gfx950 correction + WRITE_SIZE)"""
    try:
        with open(os.path.join(ROOT, 'profiles', name)) as f:
            pt = json.load(f)
        if pt['config'] == cfg:
            return pt['traffic_bytes_per_launch']
    except (OSError, KeyError, ValueError):
        pass
    return None


def cpu_baseline(N, kind, dt, target_seconds=15.0):
    """The CPU oracle (restatement of the reference's pyqg + PyTorch-CPU path) stepping ONE
    member sequentially, as the reference does, on this box's host cores."""
    from oracle import qg_ref, gen_ref, samplers_ref
    d = np.load(os.path.join(ROOT, 'tests', 'golden', f'weights_{kind}.npz'))
    nets = [gen_ref.CNNWeights.from_npz_dict(d, 'net0_')]
    if kind == 'gz':
        nets.append(gen_ref.CNNWeights.from_npz_dict(d, 'net1_'))
    ora = gen_ref.GeneratorRef(kind, nets, d['x_std'], d['y_std'])
    m = qg_ref.QGModelRef(nx=N, dt=dt, twrite=1000)
    m.sampling_type = 'constant'
    m.noise_sampler = samplers_ref.make_sampler('constant', 1)
    m.q_parameterization = gen_ref.ParameterizationRef(ora, rng=np.random.RandomState(0))
    m.set_q(eddy_like_q([0], N)[0])

    def run(threads, seconds):
        torch.set_num_threads(threads)
        for _ in range(3):
            m._step_forward()
        t0 = time.perf_counter()
        n = 0
        while True:
            for _ in range(10):
                m._step_forward()
            n += 10
            el = time.perf_counter() - t0
            if el >= seconds:
                return n, el
    # the reference runs one member per 1-core process (scripts/run_parameterized.py:55-63);
    # also time the box's GPU-share of host cores (16 per GPU) and report the faster one
    share = max(1, min(16, os.cpu_count() or 1))
    n1, el1 = run(1, target_seconds / 2)
    nm, elm = run(share, target_seconds / 2)
    r1, rm = n1 / el1, nm / elm
    best = (rm, share, nm, elm) if rm >= r1 else (r1, 1, n1, el1)
    return dict(value=best[0], unit='ensemble-timesteps/sec', cores=best[1], kind='port',
                sample=f'{best[2]} sequential steps of 1 member ({N}x{N} eddy + {kind.upper()}), '
                       f'numpy pocketfft float64 core + torch-CPU float32 generator, {best[3]:.1f} s',
                one_core=r1, cores_share=share, share_rate=rm)


def leg_config3(qa, device, K=200, W=10, one_stream=False):
    """BASELINE configs[3]'s per-GPU shard: 96x96 jet + CVAE decoder, 32 members; 200 timed steps.
    one_stream (--one-stream; the PMC passes behind profiles/): whole-ensemble launches only, so that per-launch counters
    describe one kernel shape"""
    N, B = 96, 32
    dt = dt_of(N)
    gen, _ = load_generator('vae', device)
    eng = qa.EnsembleEngine(nx=N, n_members=B, device=device, dt=dt, **JET)
    if one_stream:
        eng.set_option('streams', 1)
    eng.set_q(eddy_like_q(np.arange(B), N))
    loop = OnlineLoop(eng, dt, dict(generator=gen, sampling='constant', nsteps_decor=1, seed=2024))
    loop.run(W)
    el = timed(lambda: loop.run(K))
    # roofline of the layer-2 kernel: the timed region advances the ensemble as two halves on two streams (qgx_step_streams),
    # where the wall time of one kernel contains the other stream's share of the GPU; the kernel is therefore timed in a
    # separate pass of 40 steps on ONE stream (whole-ensemble launches, nothing beside them)
    parts = eng.step_streams(gen)
    eng.set_option('streams', 1)
    gen.set_option('prof_every', 2)
    gen.profile(1)
    loop.run(40)
    eng.set_option('streams', 1 if one_stream else 0)
    kn, ex = layer2_kernel(gen, 'f16x3', N, B)
    roof = mfma_roofline(gen, 'f16x3', N, B, kn + ' at 96x96 (generator layer 2)',
                         pmc_traffic('pmc_traffic_config3.json', {'nx': N, 'members_per_gpu': B, 'kind': 'vae'}), 2, ex)
    roof['timed_in'] = ('a separate 40-step pass on one stream after the timed region' if parts > 1 else 'the timed region')
    roof['streams_in_timed_region'] = parts
    ke, cfl = eng.status()
    out = {'workload': f'BASELINE configs[3] shard: jet {N}x{N} + CVAE, {B} members on 1 GPU (256 members / 8 GPUs), '
                       f"sampling='constant' nsteps=1, dt={dt:.0f}s",
           'value': B * K / el, 'unit': 'ensemble-timesteps/sec', 'steps': K, 'ms_per_step': 1e3 * el / K,
           'roofline': roof, 'healthy': bool(np.isfinite(ke).all() and (cfl < 1).all()),
           'note': 'throughput configuration: with the shipped (eddy-trained) CVAE a LONG jet run blows up after ~24,000 '
                   'steps in the CPU oracle too (DESIGN.md section 4, tests/test_gpu_statistics.py)'}
    eng.close()
    gen.close()
    return out


def leg_config4(qa, device, K=1000, W=24):
    """BASELINE configs[4]: 256x256 unparameterized hires members + the coarse-grain / subgrid-forcing diagnostic to
    64x64 (Operator2 and Operator5, 3/2-rule: simulate.py:88-92) once per snapshot interval.  The timed region IS one
    snapshot interval of a forcing-dataset run in its averaging half (run_forcing_datasets.py:17-25: tavestart = half
    of the run): K = ceil(3.6e6/dt) = 1000 steps, pyqg's time-averaged diagnostics every ceil(86400/dt) = 24 steps
    during the second half of them, and ONE coarse-grain at the end — nothing extrapolated."""
    from pyqg_generative_amd.tools.operators import Dev
    from pyqg_generative_amd import _lib
    N, B, nc = 256, 64, 64
    dt = dt_of(N)
    every = int(math.ceil(86400. / dt))
    eng = qa.EnsembleEngine(nx=N, n_members=B, device=device, dt=dt)
    eng.set_q(eddy_like_q(np.arange(B), N))
    # warm-up: W steps, one of them with a diagnostics increment so that the increment's work fields and accumulators (1.7 GB at
    # this size, allocated and zeroed at first use) exist before the timed region, as they do in every snapshot interval of a
    # run but its first; the accumulators are reset afterwards
    eng.diag_config(1, 1)
    eng.step(2)
    eng.diag_reset()
    eng.diag_config(W + K // 2, every)              # tavestart in the middle of the timed interval
    eng.step(W - 2)
    pp = dict(qa.engine.PYQG_DEFAULTS)

    def coarsegrain():                              # as generate_subgrid_forcing does at a snapshot
        q = eng.get(_lib.F_Q)
        qh, adv_hat = Dev.hires_tendency_hat(q, pp, '3/2-rule')
        for op in (Dev.Operator2, Dev.Operator5):
            Dev.subgrid_forcing_from_hat(qh, adv_hat, nc, op, pp, '3/2-rule')
    coarsegrain()                                   # plan creation outside the timed region
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]   # qgx_step launches on torch's current stream

    def body():
        ev[0].record()
        eng.step(K // 2)                            # spin-up half: no diagnostics
        ev[1].record()
        eng.step(K - K // 2)                        # averaging half: one increment every `every` steps
        ev[2].record()
        coarsegrain()
        ev[3].record()
    el = timed(body)
    plain_ms = ev[0].elapsed_time(ev[1]) / (K // 2)
    diag_ms = ev[1].elapsed_time(ev[2]) / (K - K // 2)
    step_ms = ev[0].elapsed_time(ev[2]) / K
    cg_ms = ev[2].elapsed_time(ev[3])
    bytes_step = 5 * (2 * N * (N // 2 + 1) * 16) * B           # 5,283,840 B per member-step
    achieved = bytes_step / (step_ms * 1e-3) / 1e9
    ke, cfl = eng.status()
    out = {'workload': f'BASELINE configs[4]: eddy {N}x{N} unparameterized, {B} members on 1 GPU, dt={dt:.0f}s; {K} steps = one '
                       f'snapshot interval, time-averaged diagnostics every {every} steps in its second half '
                       f'({eng.diag_count} increments), then one coarse-grain + 3/2-rule subgrid forcing to {nc}x{nc} '
                       '(Operator2, Operator5) — all inside the timed region',
           'value': B * K / el, 'unit': 'ensemble-timesteps/sec', 'steps': K, 'ms_per_step': step_ms,
           'ms_per_step_without_diagnostics': plain_ms, 'ms_per_step_with_diagnostics_cadence': diag_ms,
           'coarsegrain_ms': cg_ms, 'diagnostic_increments': eng.diag_count, 'run_kernel_state': eng.run_kernel_state,
           'roofline': {'bound': 'hbm', 'kernel': 'spectral step (spectral_large.hip: XCD-resident run kernel k_l_team_steps between '
                                                  'diagnostics increments + one three-launch step per call)',
                        'achieved': achieved, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': achieved / HBM_PEAK_GBS,
                        'traffic': pmc_traffic('pmc_traffic_config4.json', {'nx': N, 'members': B}),
                        'bytes_per_step': bytes_step, 'avg_step_ms': step_ms,
                        'frac_without_diagnostics': bytes_step / (plain_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                        'peak_note': 'ALGORITHMIC bytes: read qh, dqhdt_p, dqhdt_pp + write qh, dqhdt = 5 x (2 N nk 16 B) per '
                                     'member-step; avg_step_ms averages BOTH halves (with the diagnostics cadence in the second)'},
           'healthy': bool(np.isfinite(ke).all() and (cfl < 1).all())}
    eng.close()
    Dev.close()
    return out


def leg_members(qa, device, gen, B, K, W, name, note):
    """the headline workload with another resident member count (1: configs[1]; 1024: configs[2] whole on one GPU)"""
    N = 64
    dt = dt_of(N)
    e = qa.EnsembleEngine(nx=N, n_members=B, device=device, dt=dt)
    e.set_q(eddy_like_q(np.arange(B), N))
    loop = OnlineLoop(e, dt, dict(generator=gen, sampling='constant', nsteps_decor=1, seed=2024, member_offset=0))
    loop.run(W)
    loop.rehearse()
    gen.set_option('prof_every', prof_stride(K))
    gen.profile(1)
    n0 = (loop.nsnap, loop.nstatus)
    el = timed(lambda: loop.run(K))
    out = {'workload': note, 'value': B * K / el, 'unit': 'ensemble-timesteps/sec', 'steps': K, 'warmup': W,
           'ms_per_step': 1e3 * el / K, 'snapshots_in_timed_region': loop.nsnap - n0[0],
           'status_checks_in_timed_region': loop.nstatus - n0[1]}
    if B >= 8:
        Bl = B // e.step_streams(gen)
        kn, ex = layer2_kernel(gen, 'f16x3', N, Bl)
        out['roofline'] = mfma_roofline(gen, 'f16x3', N, Bl, kn + ' (generator layer 2)', None, prof_stride(K), ex)
    else:
        gen.profile_read()
        gen.profile(-1)
    ke, cfl = e.status()
    out['healthy'] = bool(np.isfinite(ke).all() and (cfl < 1).all())
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=2000, help='timed steps (SURVEY §8d: 2,000 after 100 warm-up)')
    ap.add_argument('--warmup', type=int, default=100)
    ap.add_argument('--members', type=int, default=128, help='ensemble members PER GPU (weak scaling)')
    ap.add_argument('--total-members', type=int, default=0,
                    help='strong scaling: ONE ensemble of this many members split over the ranks (overrides --members)')
    ap.add_argument('--nx', type=int, default=64)
    ap.add_argument('--kind', default='gan', choices=['gan', 'vae', 'gz'])
    ap.add_argument('--precision', default='f16x3', choices=list(PRECISIONS),
                    help='generator conv arithmetic: f16x3 = hi/lo split f16 MFMA, f32-class accuracy (default); '
                         'f32 = exact f32 MFMA')
    ap.add_argument('--full', action='store_true',
                    help='after the headline: the steady / exact_f32 / b1 / b1024 / config3 / config4 legs and the CPU baseline')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write what the timed loop computed in its last step to DIR/<name>.npy (dump_outputs)')
    ap.add_argument('--no-aux', action='store_true', help='with --full: skip the steady / exact_f32 / b1 / b1024 / config3 / config4 legs')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-preheat', action='store_true',
                    help='profiling runs (profiles/): skip the 0.3 s of generator forwards in front of the timed region, so that the '
                         'per-kernel call counts of rocprofv3 are those of the warm-up + timed steps')
    ap.add_argument('--one-stream', action='store_true',
                    help='config3 leg: never advance the ensemble as two halves on two streams (PMC passes of profiles/)')
    ap.add_argument('--leg', default='all', choices=['all', 'config3', 'config4', 'b1', 'b1024'],
                    help='profiling runs: only the named auxiliary leg (prints its JSON object)')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'],
                    help="'gloo' + QGX_BENCH_ONE_DEVICE=1 rehearses the multi-rank path on a 1-GPU box")
    args = ap.parse_args()

    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != args.gpus and world > 1:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}')
    dist = None
    if os.environ.get('QGX_BENCH_ONE_DEVICE') == '1':
        local_rank = 0                      # rehearsal: every rank shares GPU 0 (gloo only)
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if args.backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world,
                                    device_id=torch.device('cuda', local_rank))
        else:
            dist.init_process_group('gloo', rank=rank, world_size=world)

    import pyqg_generative_amd as qa
    from pyqg_generative_amd import parallel
    N, K, W = args.nx, args.steps, args.warmup
    B1 = 'BASELINE configs[1]: 64x64 eddy + CGAN, 1 member on 1 GPU (launch-latency-bound)'
    B1024 = ('BASELINE configs[2] WHOLE on one GPU: 64x64 eddy + CGAN, 1024 members (one workgroup per member in the '
             'spectral step, k_step_small<64,false> at 512 threads)')
    if args.leg != 'all':
        if args.leg in ('config3', 'config4'):
            res = (leg_config3(qa, local_rank, one_stream=args.one_stream) if args.leg == 'config3' else leg_config4(qa, local_rank))
        else:
            g, _ = load_generator(args.kind, local_rank)
            res = leg_members(qa, local_rank, g, *{'b1': (1, 2000, 100, 'b1', B1), 'b1024': (1024, 250, 10, 'b1024', B1024)}[args.leg])
        print(json.dumps({args.leg: res}))
        return
    dt = dt_of(N)
    strong = args.total_members > 0
    if strong:
        first, B = parallel.shard_members(args.total_members, rank, world)      # contiguous blocks, sizes differ by <= 1
        total_members = args.total_members
        if B < 1:
            raise SystemExit(f'--total-members {args.total_members} leaves rank {rank} of {world} without a member')
    else:
        B = args.members
        first, total_members = rank * B, B * world
    gen, wsrc = load_generator(args.kind, local_rank)
    gen.set_option('precision', PRECISIONS[args.precision])
    eng = qa.EnsembleEngine(nx=N, n_members=B, device=local_rank, dt=dt)
    eng.set_q(eddy_like_q(np.arange(first, first + B), N))
    step_kw = dict(generator=gen, sampling='constant', nsteps_decor=1, seed=2024,
                   member_offset=first)                              # run_parameterized.py:50; Philox keyed by GLOBAL member id
    loop = OnlineLoop(eng, dt, step_kw, dist, args.backend)

    def barrier():
        if dist is not None:
            dist.barrier()

    loop.run(W)
    loop.rehearse()
    # Device pre-heat, AFTER the warm-up steps and the rehearsal (whose host round trips leave the GPU idle for milliseconds), right
    # before the timed region (NOT steps of the workload, nothing of it is timed or counted): a process that starts on an idle GPU
    # finds it in a low power state, and the driver's "--steps 20" timed region is 15 ms long — shorter than the clock ramp
    # (the same engine measured 6 % faster a few seconds later: `steady`).  0.3 s of generator forwards on scratch tensors.
    preheat_s = 0.0
    if not args.no_preheat:
        xs_ = torch.randn((B, gen.n_in, N, N), dtype=torch.float32, device='cuda')
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:
            for _ in range(10):
                gen.cnn_forward(xs_)
            torch.cuda.synchronize()
        preheat_s = time.perf_counter() - t0
        del xs_
        gen.range_read()
    stride = prof_stride(K)
    gen.set_option('prof_every', stride)   # HIP events around every n-th launch: each pair idles the GPU for ~12 us
    gen.profile(1)                         # dominant kernel: conv layer 2 (128->64, 5x5), 75% of the FLOPs
    n0 = (loop.nsnap, loop.nstatus)
    elapsed = timed(lambda: loop.run(K), barrier)
    counted = (loop.nsnap - n0[0], loop.nstatus - n0[1])
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device='cuda' if args.backend == 'nccl' else 'cpu')
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ke, cfl = eng.status()
    healthy = bool(np.isfinite(ke).all() and (cfl < 1).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(eng, first, args.dump_outputs)

    out = None
    Bl = B // eng.step_streams(gen)              # members per launch (the ensemble advances as two halves on two streams)
    kname, executed = layer2_kernel(gen, args.precision, N, Bl)
    kname += ' (generator layer 2)'
    cfg = {'nx': N, 'members_per_gpu': B, 'members_per_launch': Bl, 'kind': args.kind}
    traffic = {'f32': pmc_traffic('pmc_traffic.json', cfg), 'f16x3': pmc_traffic('pmc_traffic_f16x3.json', cfg)}[args.precision]
    gen_flop_per_member_step = 2.0 * sum(MAC_PER_PIXEL) * N * N * (2 if args.kind == 'gz' else 1)
    if rank == 0:
        value = total_members * K / elapsed
        roof = mfma_roofline(gen, args.precision, N, Bl, kname, traffic, stride, executed or 3.0)
        roof['whole_step_generator_tflops'] = gen_flop_per_member_step * value / world / 1e12
        dtype = {'f32': 'f64 spectral core + f32 generator (exact-f32 MFMA)',
                 'f16x3': 'f64 spectral core + generator in f16 hi/lo split operands, 3 f16 MFMAs per product, f32 accumulate '
                          '(25-tap kernels: float32 error class; the 5x5 layer as a 1-D Winograd convolution where calibration '
                          'admitted it: within 1e-5 of the exact-f32 kernels, golden-vector tolerance 2e-5; tests/test_gpu_precision.py)'}[args.precision]
        shard = (f'ONE {total_members}-member ensemble split over {world} GPU(s): {B} members on rank 0' if strong else
                 f'{B} members per GPU (BASELINE configs[2] shard: 1024 members / 8 GPUs)')
        out = {
            'metric': 'ensemble-timesteps/sec, 64^2 2-layer eddy + GAN param',
            'value': value, 'unit': 'ensemble-timesteps/sec', 'n_gpus': world, 'steps': K, 'warmup': W,
            'ms_per_step': 1e3 * elapsed / K, 'higher_is_better': True, 'scaling': 'strong' if strong else 'weak',
            'vs_baseline': None, 'dtype': dtype,
            'data': f'synthetic band-limited PV fields (seeded per member); generator weights: {wsrc}',
            'preheat_s': round(preheat_s, 3),
            'config': {'workload': f'eddy {N}x{N} 2-layer + {args.kind.upper()} parameterization, {shard}, '
                                   f"sampling='constant' nsteps=1, dt={dt:.0f}s",
                       'members_per_gpu': B, 'total_members': total_members, 'nx': N,
                       'generator_precision': args.precision,
                       'cadence': {'diagnostics_every': int(math.ceil(86400. / dt)), 'snapshot_every': loop.snap_every,
                                   'status_every': loop.status_every, 'snapshots_in_timed_region': counted[0],
                                   'status_checks_in_timed_region': counted[1],
                                   'ensemble_mean_spectrum': 'one all-reduce of (2,N,N/2+1) f64 per snapshot'},
                       'parallelism': f'ensemble-sharded x{world}, no data-path collective'},
            'roofline': roof,
            'healthy': healthy,
        }

    aux = world == 1 and args.full and not args.no_aux and not strong
    if aux:
        # SURVEY §8(d)'s protocol whatever --steps was: 100 warm-up + 2,000 timed steps of the SAME engine, 8 snapshots
        # and 2 status checks inside, HIP events around every 10th launch of the roofline kernel (200 launches)
        KS, WS = 2000, 100
        loop.run(WS)
        gen.set_option('prof_every', 10)
        gen.profile(1)
        n0 = (loop.nsnap, loop.nstatus)
        els = timed(lambda: loop.run(KS))
        rs = mfma_roofline(gen, args.precision, N, Bl, kname, traffic, 10, executed or 3.0)
        vs = B * KS / els
        rs['whole_step_generator_tflops'] = gen_flop_per_member_step * vs / 1e12
        out['steady'] = {'protocol': 'SURVEY 8(d): 100 warm-up + 2000 timed steps at the reference cadences, independent of --steps',
                         'value': vs, 'unit': 'ensemble-timesteps/sec', 'steps': KS, 'warmup': WS,
                         'ms_per_step': 1e3 * els / KS, 'snapshots_in_timed_region': loop.nsnap - n0[0],
                         'status_checks_in_timed_region': loop.nstatus - n0[1],
                         'diagnostic_increments_in_timed_region': KS // int(math.ceil(86400. / dt)), 'roofline': rs}
    # the same workload on the exact-f32 matrix cores (auxiliary: same-precision-as-the-reference number)
    if aux and args.precision != 'f32':
        K32 = 200
        gen.set_option('precision', 0)
        loop.run(5)
        gen.set_option('prof_every', 5)
        gen.profile(1)
        el32 = timed(lambda: loop.run(K32))
        r32 = mfma_roofline(gen, 'f32', N, Bl, 'k_conv<128,64,5x5> (generator layer 2)',
                            pmc_traffic('pmc_traffic.json', {'nx': N, 'members_per_gpu': B, 'members_per_launch': Bl, 'kind': args.kind}), 5)
        gen.set_option('precision', PRECISIONS[args.precision])
        out['exact_f32'] = {'value': B * K32 / el32, 'unit': 'ensemble-timesteps/sec', 'steps': K32,
                            'ms_per_step': 1e3 * el32 / K32, 'roofline': r32}
    eng.close()

    if aux:
        out['b1'] = leg_members(qa, local_rank, gen, 1, 2000, 100, 'b1', B1)           # configs[1]
        out['b1024'] = leg_members(qa, local_rank, gen, 1024, 250, 10, 'b1024', B1024)  # configs[2] whole
        out['config3'] = leg_config3(qa, local_rank, one_stream=args.one_stream)
        out['config4'] = leg_config4(qa, local_rank)

    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out['cpu_baseline'] = cpu_baseline(N, args.kind, dt)
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
