"""The flux head of a flux-form net in a training step (csrc/fluxdiv_train.hip): the two calls alone, and a training step of
FluxFormCNN next to the same net with a torch.fft divergence under autograd and next to the div=False net, on the same GPU.

The shipped widths [128, 64, 32, 32, 32, 32, 32] at 64 x 64, batch 64:
  * the two calls alone: qgx_fluxdiv_forward and qgx_fluxdiv_backward in the engine layout on (B, N, N, 8) records;
  * step: zero_grad, compute_loss, backward, Adam step.  HIP route: FluxFormCNN (the convolutions, then flux_divergence).  torch.fft
    route: the same convolutions, then slice and permute to planar, 10000 irfftn(ik rfftn(fx) + il rfftn(fy)) under autograd.
    Everything before the divergence — convolutions, BatchNorm, ReLU — and Adam is the same code in both;
  * that step against the step of TrainableAndrewCNN (div=False: a two-channel last layer and no divergence).
HIP events, medians (min, max) of --reps, the routes alternating after a warm-up.

    python bench_tools/fluxdiv_train_time.py [--batch B] [--n N] [--reps K] [--out FILE]
                                                                                 (default profiles/fluxdiv_train_time.txt)
"""
import argparse
import os
import sys

import numpy as np
import torch

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


def alternate(routes, reps, inner):
    """routes: {name: fn} -> {name: (median, min, max) ms}, the routes taking turns within every repetition"""
    for _ in range(2):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t[name].append(event_ms(fn, inner))
    return {name: med(v) for name, v in t.items()}


def rows(title, res):
    out = [f'{title}, {name}: {m:8.3f} ms   (min {lo:.3f}, max {hi:.3f})' for name, (m, lo, hi) in res.items()]
    return out + ['']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fluxdiv_train_time.txt'))
    args = ap.parse_args()
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools import train_CNN as T, train_ops as O
    assert torch.cuda.is_available(), 'fluxdiv_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    B, N = args.batch, args.n
    hidden = [128, 64, 32, 32, 32, 32, 32]
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((B, 2, N, N), generator=g, device=dev)
    y = torch.randn((B, 2, N, N), generator=g, device=dev)
    y = y - y.mean(dim=(-2, -1), keepdim=True)
    lines = [f'fluxdiv_train_time: {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
             f'hidden_channels={hidden}, batch {B}, {N} x {N}',
             f'HIP events, medians (min, max) of {args.reps}, routes alternating, after a warm-up', '']

    # ---- the two calls alone ----
    Fe = torch.randn((B, N, N, 8), generator=g, device=dev)
    out = torch.empty_like(Fe)
    st = _lib.current_stream_ptr

    def call(fn):
        return lambda: _lib.check(fn(Fe.data_ptr(), out.data_ptr(), B, N, _lib.FLUX_ENGINE, st()))
    lines += rows('one call, engine layout', alternate({'qgx_fluxdiv_forward': call(_lib.lib.qgx_fluxdiv_forward),
                                                        'qgx_fluxdiv_backward': call(_lib.lib.qgx_fluxdiv_backward)}, args.reps, 20))

    # ---- a training step ----
    L = 1e6
    dk = 2 * np.pi / L
    kk = dk * np.arange(0., N / 2 + 1)
    ll = dk * np.append(np.arange(0., N / 2), np.arange(-N / 2, 0.))
    ik = torch.as_tensor((1j * kk[None, :] + 0 * ll[:, None]).astype('complex64')).to(dev)
    il = torch.as_tensor((1j * ll[:, None] + 0 * kk[None, :]).astype('complex64')).to(dev)

    class TorchFFTFlux(T.FluxFormCNN):
        """the same net; the divergence is torch.fft under autograd (the reference's expression)"""

        def forward(self, xx):
            Fl = T.TrainableAndrewCNN.forward_engine(self, O.to_engine_layout(self._input(xx)))[..., :4].permute(0, 3, 1, 2)
            ix = torch.fft.rfftn(Fl, dim=(-2, -1))
            return 10000. * torch.fft.irfftn(ix[:, :2] * ik + ix[:, 2:] * il, dim=(-2, -1))

    nets = {'FluxFormCNN (HIP divergence)': T.FluxFormCNN(2, 2, hidden, seed=1),
            'torch.fft divergence': TorchFFTFlux(2, 2, hidden, seed=1),
            'div=False net': T.TrainableAndrewCNN(2, 2, hidden, seed=1)}
    steps = {}
    for name, net in nets.items():
        net.to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)

        def step(net=net, opt=opt):
            opt.zero_grad()
            loss = net.compute_loss(x, y)['loss']
            loss.backward()
            opt.step()
            return loss
        steps[name] = step
    with torch.no_grad():
        for net in nets.values():
            net.eval()
        a, b = nets['FluxFormCNN (HIP divergence)'](x), nets['torch.fft divergence'](x)
        lines.append(f'forward of the first batch (same weights): largest difference between the HIP and the torch.fft route '
                     f'{float((a - b).abs().max()):.2e} of {float(b.abs().max()):.2e}')
        for net in nets.values():
            net.train()
    res = alternate(steps, args.reps, 3)
    lines += rows('training step', res)
    hip, fft, plain = (res[k][0] for k in nets)
    lines += [f'training step, torch.fft - HIP divergence: {fft - hip:+.3f} ms', f'training step, HIP divergence - div=False: {hip - plain:+.3f} ms']
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
