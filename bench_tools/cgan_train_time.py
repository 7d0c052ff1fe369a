"""The training of CGANRegression on the device route (tools/train_CGAN.py over csrc/dconv_train.hip and csrc/conv_train.hip) next
to plain torch on the same GPU, the same weights and the same device-resident data.

At nx = 64, batch 64 and the shipped widths:
  * the discriminator's four strided layers at batch 256 (a step's four evaluations): forward, data gradient and weight gradient
    through train_ops.dconv2d_*, against torch's F.conv2d(stride=2, padding=1), torch.nn.grad.conv2d_input and conv2d_weight on
    NCHW tensors (torch's library convolutions).  MACs are computed from the shapes: B (N/2)^2 cout 16 cin for each of the three;
  * one whole discriminator step (two generator forwards without a graph, the three losses with the gradient penalty, backward,
    Adam) and one discriminator + generator step (the forwards with a graph, then G_loss against the updated discriminator,
    backward, Adam), against a torch-only restatement of the same step on the nets' own nn.Sequential modules with torch.randn
    for the latent noise.
HIP events, medians (min, max) of --reps, every shape warmed up, the routes alternating.

    python bench_tools/cgan_train_time.py [--batch B] [--n N] [--samples S] [--reps K] [--out FILE]
                                                                                 (default profiles/cgan_train_time.txt)
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


def alternate(device, plain, reps, inner):
    for _ in range(2):
        device()
        plain()
    torch.cuda.synchronize()
    td, tp = [], []
    for _ in range(reps):
        td.append(event_ms(device, inner))
        tp.append(event_ms(plain, inner))
    return med(td), med(tp)


def torch_critic_losses(D, x, y, f1, f2, eps, coin):
    """cgan_regression.py:297-302 and :197-222 on D's plain torch modules, planar tensors"""
    f1, f2 = f1.detach(), f2.detach()
    Dtrue1 = D(torch.cat([x, y, f2], dim=1))
    Dtrue2 = D(torch.cat([x, f1, y], dim=1))
    Dfake = D(torch.cat([x, f1, f2], dim=1))
    D_loss = -0.5 * (Dtrue1.mean() + Dtrue2.mean()) + Dfake.mean()
    D_drift = 1e-3 * (Dtrue1 ** 2).mean()
    e = eps.reshape(-1, 1, 1, 1)
    true_cat = torch.cat((y, f2), dim=1) if coin == 0 else torch.cat((f1, y), dim=1)
    yinterp = (e * true_cat + (1 - e) * torch.cat((f1, f2), dim=1)).detach().requires_grad_(True)
    out = D(torch.cat((x, yinterp), dim=1))
    dDdy, = torch.autograd.grad(out, yinterp, grad_outputs=torch.ones_like(out), retain_graph=True, create_graph=True)
    D_grad = 10 * torch.mean((torch.linalg.norm(dDdy.view(len(x), -1), 2, dim=1) - 1) ** 2)
    return D_loss + D_grad + D_drift


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--samples', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cgan_train_time.txt'))
    args = ap.parse_args()
    from pyqg_generative_amd.tools import train_CGAN as T, train_ops as O
    assert torch.cuda.is_available(), 'cgan_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    B, N, S = args.batch, args.n, args.samples
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rand = lambda *s: torch.randn(s, generator=g, device=dev)
    lines = [f'cgan_train_time: {socket.gethostname()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'TrainableCGAN of the shipped widths (ndf 64), nx = {N}, batch {B}, {S} samples resident',
             f'HIP events, medians (min, max) of {args.reps}, routes alternating, after a warm-up of every shape', '']

    # ---- the four strided layers at the 4 B batch ----
    lines.append(f'{"layer (N, cin -> cout), batch " + str(4 * B):34s} {"operation":16s} {"GMAC":>7s} {"device ms (min, max)":>26s} {"torch ms (min, max)":>26s} '
                 f'{"torch/device":>12s} {"device TFLOP/s":>14s}')
    total = {'device': 0.0, 'torch': 0.0}
    shapes = [(N, 6, 64), (N // 2, 64, 128), (N // 4, 128, 256), (N // 8, 256, 512)]
    for n, cin, cout in shapes:
        Bb, no = 4 * B, n // 2
        xp, w, dyp = rand(Bb, cin, n, n), 0.02 * rand(cout, cin, 4, 4), rand(Bb, cout, no, no)
        xe, dye = O.to_engine_layout(xp), O.to_engine_layout(dyp)
        gmac = Bb * no * no * cout * 16 * cin / 1e9
        ops = [('forward', lambda: O.dconv2d_forward(xe, w), lambda: F.conv2d(xp, w, None, stride=2, padding=1)),
               ('data gradient', lambda: O.dconv2d_backward_data(dye, w),
                lambda: torch.nn.grad.conv2d_input(xp.shape, w, dyp, stride=2, padding=1)),
               ('weight gradient', lambda: O.dconv2d_backward_weight(xe, dye, cin, cout),
                lambda: torch.nn.grad.conv2d_weight(xp, w.shape, dyp, stride=2, padding=1))]
        for name, device, plain in ops:
            a, b = device(), plain()
            if a.dim() == 4 and a.shape[-1] != 4:             # an activation in the engine layout
                a = a[..., :b.shape[1]].permute(0, 3, 1, 2)
            err = float((a - b).abs().max() / b.abs().max())
            assert err < 1e-4, (n, cin, cout, name, err)
            d, p = alternate(device, plain, args.reps, 10)
            total['device'] += d[0]
            total['torch'] += p[0]
            lines.append(f'{f"({n}, {cin} -> {cout})":34s} {name:16s} {gmac:7.3f} {f"{d[0]:.3f} ({d[1]:.3f}, {d[2]:.3f})":>26s} '
                         f'{f"{p[0]:.3f} ({p[1]:.3f}, {p[2]:.3f})":>26s} {p[0] / d[0]:12.3f} {2 * gmac / d[0]:14.2f}')
    lines += [f'sum of the twelve medians: device {total["device"]:.3f} ms, torch {total["torch"]:.3f} ms, torch / device '
              f'{total["torch"] / total["device"]:.3f}', '']

    # ---- whole steps ----
    X, Y = rand(S, 2, N, N), rand(S, 2, N, N)
    idx = torch.randperm(S, generator=g, device=dev)[:B]
    eps = torch.rand((B,), generator=g, device=dev)
    net = T.TrainableCGAN('None', N, False, seed=1).to(dev)
    net.train()
    optD = torch.optim.Adam(net.D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    optG = torch.optim.Adam(net.G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    count = [0]

    def device_fakes():
        out = []
        for _ in range(2):
            out.append(net.G.forward_engine(O.latent_prior(X, idx, 1, count[0])))
            count[0] += 1
        return out

    def device_step(with_G):
        xe, ye = O.gather_batch(X, idx), O.gather_batch(Y, idx)
        net.D.zero_grad()
        if with_G:
            f1, f2 = device_fakes()
        else:
            with torch.no_grad():
                f1, f2 = device_fakes()
        losses = net.critic_losses(xe, ye, f1, f2, eps, count[0] % 2)
        (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()
        optD.step()
        if with_G:
            net.G.zero_grad()
            G_loss = net.generator_loss(xe, f1, f2)
            with O.data_gradient_only():
                G_loss.backward()
            optG.step()

    def torch_fakes(x):
        return [net.G.conv(torch.cat([x, torch.randn_like(x)], dim=1)) for _ in range(2)]

    def torch_step(with_G):
        x, y = X[idx], Y[idx]
        net.D.zero_grad()
        count[0] += 2
        if with_G:
            f1, f2 = torch_fakes(x)
        else:
            with torch.no_grad():
                f1, f2 = torch_fakes(x)
        torch_critic_losses(net.D, x, y, f1, f2, eps, count[0] % 2).backward()
        optD.step()
        if with_G:
            net.G.zero_grad()
            (-net.D(torch.cat([x, f1, f2], dim=1)).mean()).backward()
            optG.step()

    with torch.no_grad():                                        # the two routes state the same discriminator
        f1, f2 = rand(B, 2, N, N), rand(B, 2, N, N)
        a = net.D.forward_engine(T.critic_input(*(O.to_engine_layout(t) for t in (X[idx], f1, f2))))
        b = net.D(torch.cat([X[idx], f1, f2], dim=1)).reshape(-1)
        lines.append(f'D of one batch (same weights, same input): largest |device route - torch modules| / largest |torch modules| = '
                     f'{float((a - b).abs().max() / b.abs().max()):.2e}')
    for name, with_G in (('discriminator step', False), ('discriminator + generator step', True)):
        d, p = alternate(lambda: device_step(with_G), lambda: torch_step(with_G), args.reps, 3)
        lines += [f'{name}, device route: {d[0]:8.3f} ms   (min {d[1]:.3f}, max {d[2]:.3f})',
                  f'{name}, torch modules: {p[0]:8.3f} ms   (min {p[1]:.3f}, max {p[2]:.3f})',
                  f'{name}, torch / device: {p[0] / d[0]:.3f}   (difference {p[0] - d[0]:+.3f} ms)', '']
    text = '\n'.join(lines)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
