"""One training step of OLSModel's net (tools/train_CNN.py and tools/train_ops.py over csrc/conv_train.hip) next to plain torch on the same GPU.

The shipped widths [128, 64, 32, 32, 32, 32, 32] at 64 x 64, batch 64, BatchNorm and bias on.  Three tables:
  * per layer: forward, data gradient and weight gradient of the device kernels (packing and reduction kernels included), HIP
    events around --inner back-to-back calls, as TFLOP/s (2 B N^2 cin cout k^2 per operation) and as a share of the 157 TF
    exact-f32 matrix peak; beside them torch's library on the same shapes (F.pad(mode='circular') + aten convolution /
    convolution_backward with one output asked for at a time; its padding is part of its forward, the padding's backward is
    not in its data gradient);
  * per step: zero_grad, compute_loss, backward, Adam step — the device route (TrainableAndrewCNN) against the same modules
    evaluated by torch (nn.Conv2d with padding_mode='circular', nn.BatchNorm2d), same weights, same batch;
  * share: the device route's step with an event pair around every convolution call, the calls' sum against the step: what is
    left is the torch-side BatchNorm / ReLU / MSE / Adam work and the launch gaps.
Times are medians (min, max) of --reps, after a warm-up of every shape, the routes alternating.

    python bench_tools/cnn_train_time.py [--batch B] [--n N] [--reps K] [--inner I] [--out FILE]  (default profiles/cnn_train_time.txt)
"""
import argparse
import copy
import os
import socket
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.0


def event_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def med(v):
    return float(np.median(v)), float(min(v)), float(max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cnn_train_time.txt'))
    args = ap.parse_args()
    from pyqg_generative_amd.tools import train_CNN as T, train_ops as O
    assert torch.cuda.is_available(), 'cnn_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    B, N = args.batch, args.n
    hidden = [128, 64, 32, 32, 32, 32, 32]
    net = T.TrainableAndrewCNN(2, 2, hidden, seed=0).to(dev)
    ref = copy.deepcopy(net)                       # the same modules, evaluated by torch: ref.conv(x)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((B, 2, N, N), generator=g, device=dev)
    y = torch.randn((B, 2, N, N), generator=g, device=dev)
    lines = [f'cnn_train_time: {socket.gethostname()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'AndrewCNN(2, 2, hidden_channels={hidden}), batch {B}, {N} x {N}, BatchNorm and bias on',
             f'HIP events, medians (min, max) of {args.reps}, routes alternating, after a warm-up of every shape; per-layer rows: '
             f'{args.inner} back-to-back calls per event pair', '']

    # ---- per layer ----
    convs = [m for m in net.conv if isinstance(m, torch.nn.Conv2d)]
    lines.append('layer  cin cout k | device: fwd ms (TF, % peak)   dgrad ms (TF, % peak)   wgrad ms (TF, % peak) | torch: fwd ms  dgrad ms  wgrad ms')
    tot = dict(dev=0.0, torch=0.0)
    for l, m in enumerate(convs):
        cout, cin, k = int(m.weight.shape[0]), int(m.weight.shape[1]), int(m.weight.shape[2])
        p = k // 2
        flop = 2.0 * B * N * N * cin * cout * k * k
        xa = O.to_engine_layout(torch.randn((B, cin, N, N), generator=g, device=dev))
        dya = O.to_engine_layout(torch.randn((B, cout, N, N), generator=g, device=dev))
        w, b = m.weight.detach(), m.bias.detach()
        xp = torch.randn((B, cin, N, N), generator=g, device=dev).contiguous(memory_format=torch.channels_last)
        dyp = torch.randn((B, cout, N, N), generator=g, device=dev).contiguous(memory_format=torch.channels_last)
        xpad = F.pad(xp, (p, p, p, p), mode='circular')
        bw = lambda mask: torch.ops.aten.convolution_backward(dyp, xpad, w, [cout], [1, 1], [0, 0], [1, 1], False, [0, 0], 1, mask)
        ops = {
            'd_fwd': lambda: O.conv2d_forward(xa, w, b),
            'd_dgrad': (lambda: O.conv2d_backward_data(dya, w)) if l > 0 else None,
            'd_wgrad': lambda: O.conv2d_backward_weight(xa, dya, cin, cout, k),
            't_fwd': lambda: F.conv2d(F.pad(xp, (p, p, p, p), mode='circular'), w, b),
            't_dgrad': (lambda: bw([True, False, False])) if l > 0 else None,
            't_wgrad': lambda: bw([False, True, True]),
        }
        t = {k_: [] for k_, f in ops.items() if f}
        for k_ in t:
            ops[k_]()                                # warm-up
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for k_ in t:
                t[k_].append(event_ms(ops[k_], args.inner))

        def cell(k_):
            if k_ not in t:
                return '       (not needed)     '
            ms = med(t[k_])[0]
            return f'{ms:7.3f} ({flop / ms / 1e9:5.1f}, {100 * flop / ms / 1e9 / PEAK_TF:4.1f} %)'

        def tcell(k_):
            return f'{med(t[k_])[0]:8.3f}' if k_ in t else '     n/a'
        lines.append(f'{l + 1:5d} {cin:4d} {cout:4d} {k} | {cell("d_fwd")}   {cell("d_dgrad")}   {cell("d_wgrad")} | '
                     f'{tcell("t_fwd")} {tcell("t_dgrad")} {tcell("t_wgrad")}')
        tot['dev'] += sum(med(t[k_])[0] for k_ in t if k_.startswith('d_'))
        tot['torch'] += sum(med(t[k_])[0] for k_ in t if k_.startswith('t_'))
    lines += [f'sum of the rows: device {tot["dev"]:.3f} ms, torch {tot["torch"]:.3f} ms', '']

    # ---- per step ----
    opt_d = torch.optim.Adam(net.parameters(), lr=1e-3)
    opt_t = torch.optim.Adam(ref.parameters(), lr=1e-3)
    net.train()
    ref.train()

    def step_device():
        opt_d.zero_grad()
        loss = net.compute_loss(x, y)['loss']
        loss.backward()
        opt_d.step()
        return loss

    def step_torch():
        opt_t.zero_grad()
        loss = F.mse_loss(ref.conv(x), y)
        loss.backward()
        opt_t.step()
        return loss
    first = (float(step_device()), float(step_torch()))
    for _ in range(2):
        step_device()
        step_torch()
    torch.cuda.synchronize()
    td, tt = [], []
    for _ in range(args.reps):
        td.append(event_ms(step_device, 3))
        tt.append(event_ms(step_torch, 3))
    (md, dlo, dhi), (mt, tlo, thi) = med(td), med(tt)
    lines += [f'first-step loss (same weights, same batch): device {first[0]:.9g}, torch {first[1]:.9g}, relative difference '
              f'{abs(first[0] - first[1]) / first[1]:.2e}',
              f'device step: {md:8.3f} ms   (min {dlo:.3f}, max {dhi:.3f})',
              f'torch step:  {mt:8.3f} ms   (min {tlo:.3f}, max {thi:.3f})',
              f'ratio torch / device: {mt / md:.2f}', '']

    # ---- share of the torch-side ops in the device step ----
    pairs = []

    def bracket(fn):
        def wrapped(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            pairs.append((e0, e1))
            return out
        return wrapped
    saved = (O.conv2d_forward, O.conv2d_backward_data, O.conv2d_backward_weight)
    O.conv2d_forward, O.conv2d_backward_data, O.conv2d_backward_weight = (bracket(f) for f in saved)
    shares = []
    for _ in range(args.reps):
        pairs.clear()
        ms = event_ms(step_device)
        conv_ms = sum(a.elapsed_time(b) for a, b in pairs)
        shares.append((ms, conv_ms, len(pairs)))
    O.conv2d_forward, O.conv2d_backward_data, O.conv2d_backward_weight = saved
    ms, conv_ms, calls = sorted(shares)[len(shares) // 2]
    lines += [f'device step with an event pair around each of its {calls} convolution calls: {ms:.3f} ms, of which the calls {conv_ms:.3f} ms',
              f'share of the BatchNorm / ReLU / MSE / Adam ops and launch gaps: {100 * (1 - conv_ms / ms):.1f} % of that step '
              f'({ms - conv_ms:.3f} ms; against the unbracketed step of {md:.3f} ms: {100 * (md - conv_ms) / md:.1f} %)']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
