#!/usr/bin/env python
"""Golden vectors of the DeepInversion U-Net generator in TRAIN mode (CGANRegression(generator='DeepInversion')): imports the
reference's own DeepInversionGenerator (pyqg_generative/tools/deep_inversion.py:44-94) with the inert stubs of make_golden.py,
loads the deterministic recipe weights of pyqg_generative_amd.weights.synthetic_unet() into it, sets train mode and evaluates
one forward and the backward of the loss sum(y r) in float64 and in float32, at 32 x 32 / 2 members and 48 x 48 / 1 member.
The 52 MB of weights and gradients are not stored: the recipe regenerates the weights bit for bit, and of every gradient the
file holds the sum, the sum of magnitudes, the largest magnitude and a fixed strided sample of at most 64 elements.

Writes unet_train.npz:
  keys, shapes                  the state dict's keys in order and their shapes as a string "a,b,c" ('' for a counter)
  params                        the parameters' keys in order (what the g_* rows are indexed by)
  per case c in ('32x2', '48x1'):
    x_c (B, 4, N, N), r_c (B, 2, N, N) float32       input and the loss's weights
    y64_c, y32_c                                      the output of the float64 and of the float32 evaluation
    buf_c (concatenated, float64), buf32_c            every BatchNorm buffer after the float64 / float32 forward in state-dict
                                                      order (running_mean, running_var, num_batches_tracked of each layer)
    gstat_c (P, 3)                                    sum, sum of magnitudes, largest magnitude of each float64 gradient
    gsample_c (P, 64)                                 gradient.reshape(-1)[sample_index(n)], padded with zeros
  counters_after_two                                  the counters after a second float64 forward at 32 x 32 (4 and 2)
  weights_checksum

Run:  python tests/golden/make_golden_unet_train.py      (build machine, with the reference checked out)
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import install_inert_stubs, REF  # noqa: E402

CASES = {'32x2': (32, 2), '48x1': (48, 1)}
SAMPLE = 64


def sample_index(n):
    """at most 64 indices of a flat tensor of n elements, a fixed function of n"""
    return np.linspace(0, n - 1, min(n, SAMPLE)).astype(np.int64)


def main():
    install_inert_stubs()
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.deep_inversion import DeepInversionGenerator
    from pyqg_generative_amd import weights as W

    net = W.synthetic_unet()
    G0 = DeepInversionGenerator(4, 2)
    keys = list(G0.state_dict())
    params = [k for k, _ in G0.named_parameters()]
    buffers = [k for k in keys if k not in params]

    def fresh(dtype):
        G = DeepInversionGenerator(4, 2).to(dtype)
        sd = {k: torch.as_tensor(v).to(dtype) for k, v in net.items()}
        for k in keys:
            if k.endswith('num_batches_tracked'):
                sd[k] = torch.tensor(0, dtype=torch.long)
        G.load_state_dict(sd, strict=True)
        return G.train()

    rs = np.random.RandomState(2025)
    out = {'weights_checksum': np.array(W.unet_checksum(net)), 'keys': np.array(keys), 'params': np.array(params),
           'shapes': np.array([','.join(str(s) for s in G0.state_dict()[k].shape) for k in keys])}
    for name, (N, B) in CASES.items():
        x, r = rs.randn(B, 4, N, N).astype(np.float32), rs.randn(B, 2, N, N).astype(np.float32)
        out[f'x_{name}'], out[f'r_{name}'] = x, r
        for dtype, tag in ((torch.float64, '64'), (torch.float32, '32')):
            G = fresh(dtype)
            y = G(torch.as_tensor(x).to(dtype))
            (y * torch.as_tensor(r).to(dtype)).sum().backward()
            sd = G.state_dict()
            out[f'y{tag}_{name}'] = y.detach().numpy()
            out['buf' + ('' if tag == '64' else '32') + f'_{name}'] = np.concatenate([sd[k].detach().double().reshape(-1).numpy() for k in buffers])
            if tag == '64':
                grads = dict((k, p.grad.detach().numpy().reshape(-1)) for k, p in G.named_parameters())
                out[f'gstat_{name}'] = np.array([[grads[k].sum(), np.abs(grads[k]).sum(), np.abs(grads[k]).max()] for k in params])
                gs = np.zeros((len(params), SAMPLE))
                for i, k in enumerate(params):
                    idx = sample_index(grads[k].size)
                    gs[i, :len(idx)] = grads[k][idx]
                out[f'gsample_{name}'] = gs
                if name == '32x2':
                    with torch.no_grad():
                        G(torch.as_tensor(x).to(dtype))
                    sd = G.state_dict()
                    out['counters_after_two'] = np.array([int(sd[k]) for k in buffers if k.endswith('num_batches_tracked')])
        print(f'{name}: max|y| {np.abs(out[f"y64_{name}"]).max():.3g}, float32 deviates '
              f'{np.abs(out[f"y32_{name}"] - out[f"y64_{name}"]).max() / np.abs(out[f"y64_{name}"]).max():.2e}')
    np.savez_compressed(os.path.join(HERE, 'unet_train.npz'), **out)
    print('unet_train.npz:', os.path.getsize(os.path.join(HERE, 'unet_train.npz')), 'bytes')


if __name__ == '__main__':
    main()
