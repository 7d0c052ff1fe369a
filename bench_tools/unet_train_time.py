"""The training of the DeepInversion U-Net generator on the device route (tools/train_UNet.py over csrc/uconv_train.hip) next to the
SAME module's planar forward (torch's library convolutions) on the same GPU, in the same process, back to back.

At nx = 64, batch 64:
  * each distinct convolution shape of the net: forward, data gradient and weight gradient through train_ops.uconv2d_*, against
    F.conv2d on the circularly padded NCHW tensor, the same with the flipped, transposed weights over dy (a circular
    convolution's data gradient) and torch.nn.grad.conv2d_weight.  MACs from the shapes: B n^2 cout k^2 cin for each of the three;
  * one generator step: forward_engine plus backward of sum(y r), against forward plus backward;
  * one full train_CGAN batch with a generator step (two generator forwards with a graph, the discriminator's losses with the
    gradient penalty, backward, Adam, G_loss against the updated discriminator, backward, Adam), against the same step with the
    generator's planar forward and the discriminator's torch modules.
Device events, medians (min, max) of --reps after a warm-up of every shape, the routes alternating.  Boxes differ by 5-10 %: only
the ratios of one process count.  One JSON object per line.

    python bench_tools/unet_train_time.py [--batch B] [--n N] [--reps K] [--out FILE]   (default profiles/unet_train_time.jsonl)
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_tools.cgan_train_time import alternate, torch_critic_losses  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unet_train_time.jsonl'))
    args = ap.parse_args()
    from pyqg_generative_amd.tools import train_CGAN as T, train_ops as O
    from pyqg_generative_amd.tools.train_UNet import unet_layer_shapes
    assert torch.cuda.is_available(), 'unet_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    B, N = args.batch, args.n
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rand = lambda *s: torch.randn(s, generator=g, device=dev)
    rows = [dict(kind='meta', host=socket.gethostname(), gpu=torch.cuda.get_device_name(0), torch=torch.__version__, nx=N, batch=B,
                 reps=args.reps, timing='device events, median (min, max) ms, routes alternating, every shape warmed up')]

    def record(row, d, p):
        row.update(device_ms=round(d[0], 4), device_min=round(d[1], 4), device_max=round(d[2], 4), torch_ms=round(p[0], 4),
                   torch_min=round(p[1], 4), torch_max=round(p[2], 4), torch_over_device=round(p[0] / d[0], 3))
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- each distinct convolution shape ----
    shapes = sorted(set(unet_layer_shapes(N)), key=lambda s: (-s[3], s[2], s[0], s[1]))
    calls = {s: unet_layer_shapes(N).count(s) for s in shapes}
    total = {'device': 0.0, 'torch': 0.0}
    for cin, cout, k, n in shapes:
        p = k // 2
        xp, w, b, dyp = rand(B, cin, n, n), 0.02 * rand(cout, cin, k, k), rand(cout), rand(B, cout, n, n)
        xe, dye = O.to_engine_layout(xp), O.to_engine_layout(dyp)
        pad = (lambda t: F.pad(t, (p, p, p, p), mode='circular')) if p else (lambda t: t)
        xpad = pad(xp)
        wft = w.flip(2, 3).transpose(0, 1).contiguous()      # a circular convolution's data gradient is one with these weights
        ops = [('forward', lambda: O.uconv2d_forward(xe, w, b), lambda: F.conv2d(pad(xp), w, b)),
               ('data gradient', lambda: O.uconv2d_backward_data(dye, w), lambda: F.conv2d(pad(dyp), wft)),
               ('weight gradient', lambda: O.uconv2d_backward_weight(xe, dye, cin, cout, k)[0],
                lambda: torch.nn.grad.conv2d_weight(xpad, w.shape, dyp))]
        gmac = B * n * n * cout * k * k * cin / 1e9
        for name, device, plain in ops:
            a, c = device(), plain()
            if name != 'weight gradient':                                        # an activation in the engine layout
                a = a[..., :c.shape[1]].permute(0, 3, 1, 2)
            err = float((a - c).abs().max() / c.abs().max())
            assert err < 1e-4, (cin, cout, k, n, name, err)
            d, t = alternate(device, plain, args.reps, 10)
            total['device'] += d[0] * calls[(cin, cout, k, n)]
            total['torch'] += t[0] * calls[(cin, cout, k, n)]
            record(dict(kind='layer', grid=n, cin=cin, cout=cout, k=k, op=name, calls_per_forward=calls[(cin, cout, k, n)], gmac=round(gmac, 4),
                        device_tflops=round(2 * gmac / d[0], 2)), d, t)
    rows.append(dict(kind='layers_sum', what='the medians weighted by the calls of one forward and backward', device_ms=round(total['device'], 3),
                     torch_ms=round(total['torch'], 3), torch_over_device=round(total['torch'] / total['device'], 3)))
    print(json.dumps(rows[-1]), flush=True)

    # ---- one generator step, one full batch ----
    S = 4 * B
    X, Y = rand(S, 2, N, N), rand(S, 2, N, N)
    idx = torch.randperm(S, generator=g, device=dev)[:B]
    eps = torch.rand((B,), generator=g, device=dev)
    r = rand(B, 2, N, N)
    re = O.to_engine_layout(r)
    net = T.TrainableUNetCGAN('None', N, seed=1).to(dev)
    net.train()
    optD = torch.optim.Adam(net.D.parameters(), lr=2e-4, betas=(0.5, 0.999))
    optG = torch.optim.Adam(net.G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    count = [0]

    def device_generator():
        net.G.zero_grad()
        (net.G.forward_engine(O.latent_prior(X, idx, 1, 0)) * re).sum().backward()

    def torch_generator():
        net.G.zero_grad()
        x = X[idx]
        (net.G(torch.cat([x, torch.randn_like(x)], dim=1)) * r).sum().backward()
    d, t = alternate(device_generator, torch_generator, args.reps, 3)
    record(dict(kind='generator_step', what='forward and backward of the U-Net, no optimizer'), d, t)

    def device_batch():
        xe, ye = O.gather_batch(X, idx), O.gather_batch(Y, idx)
        net.D.zero_grad()
        f1, f2 = (net.G.forward_engine(O.latent_prior(X, idx, 1, count[0] + i)) for i in range(2))
        count[0] += 2
        losses = net.critic_losses(xe, ye, f1, f2, eps, count[0] % 2)
        (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()
        optD.step()
        net.G.zero_grad()
        G_loss = net.generator_loss(xe, f1, f2)
        with O.data_gradient_only():
            G_loss.backward()
        optG.step()

    def torch_batch():
        x, y = X[idx], Y[idx]
        net.D.zero_grad()
        count[0] += 2
        f1, f2 = (net.G(torch.cat([x, torch.randn_like(x)], dim=1)) for _ in range(2))
        torch_critic_losses(net.D, x, y, f1, f2, eps, count[0] % 2).backward()
        optD.step()
        net.G.zero_grad()
        (-net.D(torch.cat([x, f1, f2], dim=1)).mean()).backward()
        optG.step()
    d, t = alternate(device_batch, torch_batch, args.reps, 3)
    record(dict(kind='train_batch', what='one train_CGAN batch with a generator step: D step, then G step, both Adams'), d, t)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for row in rows:
            f.write(json.dumps(row) + '\n')


if __name__ == '__main__':
    main()
