#!/usr/bin/env python
"""Golden vectors of the DeepInversion U-Net generator (CGANRegression(generator='DeepInversion')): imports the
reference's own DeepInversionGenerator (pyqg_generative/tools/deep_inversion.py:44-94) with the inert stubs of
make_golden.py, loads the deterministic recipe weights of pyqg_generative_amd.weights.synthetic_unet() into it and
records eval-mode float32 CPU forwards.  The 52 MB of weights are not stored: the file holds their checksum, and the
recipe regenerates them bit for bit.

Writes unet.npz: x{N} (B, 4, N, N) inputs and y{N} (B, 2, N, N) outputs for N = 32, 48, 64 (2 members) and 96, 128
(1 member), bottleneck64 (the res512 output at 64 x 64) and weights_checksum.

Run:  python tests/golden/make_golden_unet.py      (build machine, with the reference checked out)
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import install_inert_stubs, REF  # noqa: E402

SIZES = {32: 2, 48: 2, 64: 2, 96: 1, 128: 1}


def main():
    install_inert_stubs()
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.deep_inversion import DeepInversionGenerator
    from pyqg_generative_amd import weights as W

    net = W.synthetic_unet()
    G = DeepInversionGenerator(4, 2)
    sd = {k: torch.as_tensor(v) for k, v in net.items()}
    for k in G.state_dict():
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.tensor(0, dtype=torch.long)
    G.load_state_dict(sd, strict=True)
    G.eval()
    keep = {}
    G.res512.register_forward_hook(lambda mod, inp, out: keep.__setitem__('b', out.detach().clone()))
    rs = np.random.RandomState(2024)
    out = {'weights_checksum': np.array(W.unet_checksum(net))}
    for N, B in SIZES.items():
        x = rs.randn(B, 4, N, N).astype(np.float32)
        with torch.no_grad():
            y = G(torch.as_tensor(x)).numpy()
        out[f'x{N}'], out[f'y{N}'] = x, y
        if N == 64:
            out['bottleneck64'] = keep['b'].numpy()
        print(f'N={N}: max|y| {np.abs(y).max():.3g}, max|bottleneck| {keep["b"].abs().max().item():.3g}')
    np.savez(os.path.join(HERE, 'unet.npz'), **out)


if __name__ == '__main__':
    main()
