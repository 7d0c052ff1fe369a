"""One training step of ANNModel's stencil network (csrc/ann_train.hip) next to the reference's route on the same GPU.

10^7 synthetic stencil rows resident on the device, the default net (3 x 3, [24, 24]), batches of 2^15 rows, one epoch =
ceil(rows / batch) steps over one permutation of the rows.  Both routes see the same rows, the same initial weights and the
same batch indices:
  * device: qgx_ann_trainer_step per batch (two launches: loss + gradient partials, reduction + Adam), the epoch's loss
    accumulated on the device;
  * torch:  the reference's loop (tools/cnn_tools.py:645-700) with the rows already on the GPU: an nn.Sequential ANN, MSELoss,
    torch.optim.Adam, index_select per step.  The reference reads the loss back every step (.item()); here it is summed on
    the device instead, which favours the torch route.
Times: HIP events around one epoch, after a warm-up epoch of each route, the two routes alternating, median (min, max) of
--reps epochs.  us per step = epoch time / steps.

    python bench_tools/ann_train_time.py [--rows R] [--batch B] [--reps K] [--out FILE]   (default profiles/ann_train_time.txt)
    python bench_tools/ann_train_time.py --device-only    (one epoch of device steps, for a kernel trace of its own)
"""
import argparse
import math
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=10 ** 7)
    ap.add_argument('--batch', type=int, default=2 ** 15)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--device-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ann_train_time.txt'))
    args = ap.parse_args()
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    assert torch.cuda.is_available(), 'ann_train_time.py needs cuda:0'
    dev = torch.device('cuda', 0)
    R, B, lr = args.rows, args.batch, 1e-3
    steps = math.ceil(R / B)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    X = torch.randn((R, 9), generator=g, device=dev, dtype=torch.float32)
    Y = (torch.tanh(X[:, 4:5] - 0.5 * X[:, 1:2] * X[:, 7:8]) + 0.1 * torch.randn((R, 1), generator=g, device=dev)).contiguous()
    xs = float(X[:, 4].double().std(unbiased=False).float())
    ys = float(Y.double().std(unbiased=False).float())
    order = torch.randperm(R, generator=g, device=dev)
    batches = [order[b0:b0 + B] for b0 in range(0, R, B)]
    net = weights.synthetic_ann(3, [24, 24], False, 0)

    trainer = AnnTrainer(net, device=0)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)

    def device_epoch():
        acc.zero_()
        for idx in batches:
            trainer.step(X, Y, idx, xs, ys, lr, acc)

    if args.device_only:
        device_epoch()
        torch.cuda.synchronize()
        print('device epoch loss', float(acc[0] / acc[1]))
        return

    layers = []
    for l in range(3):
        w = torch.as_tensor(net['w'][l])
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(torch.as_tensor(net['b'][l]))
        layers += [lin] + ([torch.nn.ReLU()] if l < 2 else [])
    model = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    crit = torch.nn.MSELoss()
    Xn, Yn = X / xs, Y / ys                       # the reference normalises the rows once (ann_model.py:40-43)
    tacc = torch.zeros((), dtype=torch.float64, device=dev)

    def torch_epoch():
        tacc.zero_()
        for idx in batches:
            opt.zero_grad()
            loss = crit(model(Xn.index_select(0, idx)), Yn.index_select(0, idx))
            loss.backward()
            opt.step()
            tacc.add_(loss.detach().double() * idx.numel())

    # warm-up: one epoch each (code objects, allocator, rocBLAS's choices); their losses are the first epoch's of both routes
    device_epoch()
    torch_epoch()
    torch.cuda.synchronize()
    first = (float(acc[0] / acc[1]), float(tacc / R))
    t_dev, t_torch = [], []
    for _ in range(args.reps):
        t_dev.append(event_ms(device_epoch))
        t_torch.append(event_ms(torch_epoch))
    md, mt = float(np.median(t_dev)), float(np.median(t_torch))
    lines = [
        f'ann_train_time: {socket.gethostname()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}',
        f'rows {R}, batch {B}, steps per epoch {steps}, net 3x3 [24, 24] (865 parameters), lr {lr}',
        f'first-epoch loss (same start, same batches): device {first[0]:.9g}, torch {first[1]:.9g}, '
        f'relative difference {abs(first[0] - first[1]) / first[1]:.2e}',
        f'HIP events around one epoch, after one warm-up epoch of each route, routes alternating, {args.reps} epochs each',
        f'device step: {1e3 * md / steps:8.2f} us per step   {md / 1e3:.4f} s per epoch   '
        f'(min {1e3 * min(t_dev) / steps:.2f}, max {1e3 * max(t_dev) / steps:.2f} us per step)',
        f'torch route: {1e3 * mt / steps:8.2f} us per step   {mt / 1e3:.4f} s per epoch   '
        f'(min {1e3 * min(t_torch) / steps:.2f}, max {1e3 * max(t_torch) / steps:.2f} us per step)',
        f'ratio torch / device: {mt / md:.2f}',
    ]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)
    trainer.close()


if __name__ == '__main__':
    main()
