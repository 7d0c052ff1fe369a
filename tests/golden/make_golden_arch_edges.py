#!/usr/bin/env python
"""Pins the float64 truth of the generic engine's edge cases (tests/arch_restatement.py::EDGE_CASES) to the reference: imports the
reference's own AndrewCNN (pyqg_generative/tools/cnn_tools.py:125-176) with the inert stubs of make_golden.py and the grid-line
stub of make_golden_div.py, loads the seeded weights (weights.synthetic_arch; NOT stored), runs it in float64 with torch on the CPU
on the seeded inputs (arch_restatement.edge_inputs; NOT stored), and keeps EDGE_SAMPLES values of every output.

  {case}_checksum        weights.net_checksum of the case's net
  {case}_y_{N}           (256,) float64: AndrewCNN(...).double()(x).reshape(-1)[arch_restatement.edge_positions(case, N)]
  {case}_ymax_{N}        max|y| of the whole output

Case K (kernel sizes [3, 5, 5]) is stored like the others: the constructor's `kernels=` argument builds it (kernels[0],
kernels[i + 1], kernels[-1]: with two hidden layers the list is read as given).

Run:  python tests/golden/make_golden_arch_edges.py      (build machine, with the reference checked out)
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import install_inert_stubs, REF  # noqa: E402
from make_golden_div import install_grid_stub  # noqa: E402
import arch_restatement as AR  # noqa: E402


def main():
    install_inert_stubs()
    install_grid_stub()
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.cnn_tools import AndrewCNN
    from pyqg_generative_amd import weights as W

    out = {}
    for name, c in AR.EDGE_CASES.items():
        net = AR.edge_net(name)
        out[f'{name}_checksum'] = np.array(W.net_checksum(net))
        kernels = AR.edge_kernels(name)
        assert len(kernels) == len(c['hidden_channels']) + 1
        kw = dict(kernels=kernels) if 'kernels' in c else {}
        ref = AndrewCNN(c['n_in'], 2, batch_norm=c['batch_norm'], bias=c['bias'], div=c['div'], hidden_channels=c['hidden_channels'], **kw)
        sd = {k: torch.as_tensor(v) for k, v in W.state_dict_from_net(net).items()}
        ref.load_state_dict(sd, strict=False)        # (strict=False: num_batches_tracked is not in the dict)
        have = {k: tuple(v.shape) for k, v in ref.state_dict().items() if not k.endswith('num_batches_tracked')}
        assert have == {k: tuple(v.shape) for k, v in sd.items()}, (name, have)
        ref = ref.double().eval()
        for N in c['sizes']:
            x = AR.edge_inputs(name, N)
            with torch.no_grad():
                y = ref(torch.as_tensor(x).double()).numpy()
            assert y.dtype == np.float64 and y.shape == (AR.EDGE_T, 2, N, N)
            out[f'{name}_y_{N}'] = y.reshape(-1)[AR.edge_positions(name, N)]
            out[f'{name}_ymax_{N}'] = np.array(np.abs(y).max())
            print(f'{name} N={N}: max|y| {np.abs(y).max():.3g}')
    path = os.path.join(HERE, 'generator_arch_edges.npz')
    np.savez(path, **out)
    print(f'{path}: {os.path.getsize(path)} bytes')
    assert os.path.getsize(path) < 128 * 1024


if __name__ == '__main__':
    main()
