#!/usr/bin/env python
"""Golden vectors of ANNModel, the pointwise stencil-ANN parameterization: imports the reference's own ANNModel
(pyqg_generative/models/ann_model.py) with the inert stubs of make_golden.py plus a minimal xarray.DataArray stand-in (what
predict_snapshot and xarray_to_stencil use of it: astype, pad(mode='wrap'), values, shape), builds it from a
reference-layout model folder written in a temporary directory, and records predict_snapshot(m, 0).

Each folder holds a seeded ANN (the reference's own class, torch's default initialisation) as net.pt, scale.json with
training-like magnitudes, and model_args.json from the reference's save_model_args.  Three nets:
  a  the default: stencil 3, hidden [24, 24]
  b  scale_invariant=True (ANN degree 2), otherwise the default
  c  stencil 5, hidden [32, 16, 8]

Writes ann.npz (compressed): the nets' weights ({tag}_w{l}, {tag}_b{l}, {tag}_s, {tag}_hidden, {tag}_si), x_scale,
y_scale, q{N} (2, N, N) seeded eddy-like PV for N = 32, 48, 64, 96, 128 and S{tag}{N} the forcing of each net; for net b
also qz{N} / Sbz{N}, a field whose lower layer is zero (the reference's set_initial_condition leaves it so): its stencils
have norm 0 and the forcing there is NaN.  q and S are stored as float32 without loss: predict_snapshot reads q as
float32, and its forcing is a float32 product cast to float64.

Run:  python tests/golden/make_golden_ann.py      (build machine, with the reference checked out)
"""
import json
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import install_inert_stubs, REF  # noqa: E402
from make_golden_ols import eddy_like_q  # noqa: E402

SIZES = (32, 48, 64, 96, 128)
ZERO_LOWER = (32,)
X_STD = np.array([7.784383342368528e-06, 1.0471941322975908e-06])     # PV amplitude per layer (eddy configuration)
X_SCALE, Y_SCALE = 4.87e-06, 5.21e-12                                   # scale.json as prepare_data_ANN writes it: floats
NETS = {'a': dict(stencil_size=3, hidden_channels=[24, 24], scale_invariant=False),
        'b': dict(stencil_size=3, hidden_channels=[24, 24], scale_invariant=True),
        'c': dict(stencil_size=5, hidden_channels=[32, 16, 8], scale_invariant=False)}


class DataArray:
    """what ann_model.predict_snapshot and cnn_tools.xarray_to_stencil use of xarray.DataArray"""
    def __init__(self, data, dims=None):
        self.values = np.asarray(data)
        self.dims = list(dims)

    @property
    def shape(self):
        return self.values.shape

    def astype(self, dtype):
        return DataArray(self.values.astype(dtype), self.dims)

    def pad(self, mode='constant', **widths):
        assert mode == 'wrap'
        pw = [(0, 0)] * self.values.ndim
        for dim, w in widths.items():
            pw[self.dims.index(dim)] = (w, w)
        return DataArray(np.pad(self.values, pw, mode='wrap'), self.dims)


def main():
    install_inert_stubs()
    sys.modules['xarray'].DataArray = DataArray
    sys.path.insert(0, REF)
    import torch
    torch.set_num_threads(4)
    from pyqg_generative.tools.cnn_tools import ANN, save_model_args
    from pyqg_generative.models.ann_model import ANNModel

    class _M:
        pass
    rs = np.random.RandomState(2024)
    out = {'x_scale': np.float64(X_SCALE), 'y_scale': np.float64(Y_SCALE)}
    qs = {N: eddy_like_q(rs, 1, N, X_STD)[0].astype(np.float32) for N in SIZES}
    qz = {}
    for N in ZERO_LOWER:
        qz[N] = eddy_like_q(rs, 1, N, X_STD)[0].astype(np.float32)
        qz[N][1] = 0
    for N in SIZES:
        out[f'q{N}'] = qs[N]
    for N in ZERO_LOWER:
        out[f'qz{N}'] = qz[N]
    for seed, (tag, args) in enumerate(NETS.items()):
        torch.manual_seed(100 + seed)
        s, hidden, si = args['stencil_size'], args['hidden_channels'], args['scale_invariant']
        net = ANN(s ** 2, 1, hidden, degree=2 if si else None)
        with tempfile.TemporaryDirectory() as folder:
            torch.save(net.state_dict(), os.path.join(folder, 'net.pt'))
            with open(os.path.join(folder, 'scale.json'), 'w') as f:
                json.dump({'x_scale': X_SCALE, 'y_scale': Y_SCALE}, f)
            save_model_args('ANNModel', folder=folder, **args)
            model = ANNModel(folder=folder, **args)
        sd = model.net.state_dict()
        for l in range(len(hidden) + 1):
            out[f'{tag}_w{l}'] = sd[f'layers.{2 * l}.weight'].numpy().astype(np.float32)
            out[f'{tag}_b{l}'] = sd[f'layers.{2 * l}.bias'].numpy().astype(np.float32)
        out[f'{tag}_s'], out[f'{tag}_hidden'], out[f'{tag}_si'] = np.int32(s), np.array(hidden, np.int32), np.int32(si)
        fields = [(f'S{tag}{N}', qs[N]) for N in SIZES]
        if si:
            fields += [(f'S{tag}z{N}', qz[N]) for N in ZERO_LOWER]
        for key, q in fields:
            m = _M()
            m.q = q.astype(np.float64)
            S = model.predict_snapshot(m, 0)
            assert S.dtype == np.float64 and S.shape == q.shape
            assert np.array_equal(S.astype(np.float32).astype(np.float64), S, equal_nan=True)
            out[key] = S.astype(np.float32)
            print(f'{key}: max|S| {np.nanmax(np.abs(S)):.3g}, NaN {int(np.isnan(S).sum())}')
    np.savez_compressed(os.path.join(HERE, 'ann.npz'), **out)
    print(f'ann.npz: {os.path.getsize(os.path.join(HERE, "ann.npz"))} bytes')


if __name__ == '__main__':
    main()
