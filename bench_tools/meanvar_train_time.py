"""One training step of MeanVarModel's variance net with the fused ends (csrc/train_head.hip) next to the same step with torch
expressions at both ends, on the same GPU, the same net and the same device-resident data set.

The shipped widths [128, 64, 32, 32, 32, 32, 32] at 64 x 64, batch 64, head 'softplus_mse', --samples samples resident:
  * step: zero_grad, loss, backward, Adam step.  Fused route: FusedHeadCNN.indexed_loss (qgx_batch_gather -> the convolutions
    -> qgx_head_loss, and qgx_head_grad in the backward).  Torch route: FusedHeadCNN.compute_loss on X[idx], T[idx] (index
    gather, to_engine_layout's zero fill and permuted copy, slice and permute back, softplus, mse_loss, autograd's backward of
    each).  Everything between the ends — convolutions, BatchNorm, ReLU, Adam — is the same code in both;
  * ends alone: the same two sets of operations around a fixed last activation instead of the net;
  * residual pass: (T - net_mean(X))^2 over all the samples in batches, squared_residuals (gather and qgx_head_apply) against
    the eval-mode forward with torch expressions at both ends.
HIP events, medians (min, max) of --reps, the routes alternating after a warm-up.

    python bench_tools/meanvar_train_time.py [--batch B] [--n N] [--samples S] [--reps K] [--out FILE]
                                                                                 (default profiles/meanvar_train_time.txt)
"""
import argparse
import os
import socket
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def alternate(fused, plain, reps, inner):
    for _ in range(2):
        fused()
        plain()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(reps):
        tf.append(event_ms(fused, inner))
        tp.append(event_ms(plain, inner))
    return med(tf), med(tp)


def rows(name, f, p):
    return [f'{name}, fused ends: {f[0]:8.3f} ms   (min {f[1]:.3f}, max {f[2]:.3f})',
            f'{name}, torch ends: {p[0]:8.3f} ms   (min {p[1]:.3f}, max {p[2]:.3f})',
            f'{name}, torch / fused: {p[0] / f[0]:.3f}   (difference {p[0] - f[0]:+.3f} ms)', '']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'meanvar_train_time.txt'))
    args = ap.parse_args()
    from pyqg_generative_amd.tools import train_CNN as T, train_ops as O
    assert torch.cuda.is_available(), 'meanvar_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    B, N, S = args.batch, args.n, args.samples
    hidden = [128, 64, 32, 32, 32, 32, 32]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X = torch.randn((S, 2, N, N), generator=g, device=dev)
    Tg = torch.randn((S, 2, N, N), generator=g, device=dev) ** 2
    idx = torch.randperm(S, generator=g, device=dev)[:B]
    lines = [f'meanvar_train_time: {socket.gethostname()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f"FusedHeadCNN(2, 2, hidden_channels={hidden}, head='softplus_mse'), batch {B}, {N} x {N}, {S} samples resident",
             f'HIP events, medians (min, max) of {args.reps}, routes alternating, after a warm-up', '']

    # ---- a training step ----
    net = T.FusedHeadCNN(2, 2, hidden, head='softplus_mse', seed=1).to(dev)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    def step(loss_of):
        opt.zero_grad()
        loss = loss_of()
        loss.backward()
        opt.step()
        return loss
    fused = lambda: step(lambda: net.indexed_loss(X, Tg, idx)['loss'])
    plain = lambda: step(lambda: net.compute_loss(X[idx], Tg[idx])['loss'])
    with torch.no_grad():
        net.eval()
        first = (float(net.indexed_loss(X, Tg, idx)['loss']), float(net.compute_loss(X[idx], Tg[idx])['loss']))
        net.train()
    lines.append(f'loss of the first batch (same weights): fused ends {first[0]:.9g}, torch ends {first[1]:.9g}, relative difference '
                 f'{abs(first[0] - first[1]) / first[1]:.2e}')
    lines += rows('training step', *alternate(fused, plain, args.reps, 3))

    # ---- the ends alone ----
    y = torch.randn((B, N, N, 8), generator=g, device=dev)
    y[..., 2:] = 0
    y.requires_grad_(True)

    def ends_fused():
        y.grad = None
        a = O.gather_batch(X, idx)
        O.head_loss(y, Tg, idx, 'softplus_mse').backward()
        return a

    def ends_plain():
        y.grad = None
        a = O.to_engine_layout(X[idx])
        F.mse_loss(F.softplus(y[..., :2].permute(0, 3, 1, 2)), Tg[idx]).backward()
        return a
    lines += rows('the two ends alone', *alternate(ends_fused, ends_plain, args.reps, 10))

    # ---- the residual pass ----
    net_mean = T.FusedHeadCNN(2, 2, hidden, head='mse', seed=0).to(dev)

    def residual_plain():
        out = torch.empty_like(Tg)
        net_mean.eval()
        with torch.no_grad():
            for s in range(0, S, B):
                out[s:s + B] = (Tg[s:s + B] - T.TrainableAndrewCNN.forward(net_mean, X[s:s + B])) ** 2
        net_mean.train()
        return out
    residual_fused = lambda: T.squared_residuals(net_mean, X, Tg, B)
    a, b = residual_fused(), residual_plain()
    lines.append(f'residuals of {S} samples: largest difference between the routes {float((a - b).abs().max()):.2e} of {float(b.abs().max()):.2e}')
    lines += rows(f'residual pass over {S} samples', *alternate(residual_fused, residual_plain, args.reps, 1))
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
