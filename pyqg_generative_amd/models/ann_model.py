"""Pointwise stencil-ANN parameterization, inference surface of pyqg_generative/models/ann_model.py (:18-31 constructor,
:54-77 save_model / load_model, :79-93 generate_latent_noise / predict_snapshot, :95-113 predict).

One small MLP (tools/cnn_tools.py:184-210, ANN) maps the s x s PV stencil around every grid point, divided by the scalar
x_scale, to the forcing at that point times y_scale; both layers of every member share the net.  It runs on the device
(csrc/ann.hip): the kernel reads q itself, so an online step needs no input assembly."""
import os
import numpy as np
import torch

from .parameterization import Parameterization
from ..engine import Generator
from .. import weights as _weights


class ANNModel(Parameterization):
    kind = 'ann'
    NET_NAMES = ()       # the torch ANN of the reference (self.net) is not bound: stencil rows are not an input here

    def __init__(self, scale_invariant=False, stencil_size=3, hidden_channels=[24, 24], folder='model', read=True,
                 device=0):
        self.stencil_size, self.hidden_channels = int(stencil_size), [int(h) for h in hidden_channels]
        self.scale_invariant = bool(scale_invariant)
        self.folder = folder
        # the reference builds an untrained net without read (ann_model.py:29-31) or without net.pt (:68-70), for fit()
        if not read:
            raise NotImplementedError('ANNModel(read=False) is an untrained net for fit(); training is '
                                      'tools.train_ANN.fit_ann, which writes the model folder and returns the model: here, '
                                      'give a trained model folder (net.pt, scale.json)')
        path = os.path.join(folder, 'net.pt')
        if not os.path.exists(path):
            raise FileNotFoundError(f'{path} is missing: ANNModel needs a trained model folder (net.pt, scale.json)')
        sd = torch.load(path, map_location='cpu', weights_only=True)
        if not _weights.is_ann_state_dict(sd):
            raise NotImplementedError(f'{path} holds no ANN (keys {", ".join(sorted(sd)[:2])}, ...): ANNModel runs the ANN of '
                                      'cnn_tools.py (layers.{2l}.weight / bias) only')
        net = _weights.ann_from_state_dict(sd, self.stencil_size, self.hidden_channels, self.scale_invariant)
        x_scale, y_scale = _weights.read_ann_scale(folder)
        self._init(net, x_scale, y_scale, device)

    def _init(self, net, x_scale, y_scale, device):
        self.x_scale, self.y_scale = x_scale, y_scale          # Python floats, as the reference reads them (:71-75)
        self._gen = Generator('ann', [net], x_scale, y_scale, device=device)

    @classmethod
    def from_arrays(cls, net, x_scale, y_scale, device=0):
        """Build from in-memory weights (a weights.ann_from_state_dict / weights.synthetic_ann dict) instead of a folder."""
        self = cls.__new__(cls)
        self.folder = None
        self.stencil_size, self.hidden_channels = int(net['stencil_size']), list(net['hidden'])
        self.scale_invariant = bool(net['scale_invariant'])
        self._init(net, float(x_scale), float(y_scale), device)
        return self

    def fit(self, *args, **kw):
        raise NotImplementedError('ANNModel.fit: training is tools.train_ANN.fit_ann(ds_train, ds_test, ...), which writes '
                                  'the model folder and returns the ANNModel read from it')

    def generate_latent_noise(self, ny, nx):
        return 0

    def predict_snapshot(self, m, noise):
        """S = y_scale * net(stencil(float32(q)) / x_scale) for ONE snapshot (2, N, N) or a batch (B, 2, N, N); `noise` is
        ignored"""
        return self._forward(m.q, None, demean=False)

    # snapshots per device launch of predict: 2^24 float64 values of q (128 MiB) at most
    PREDICT_VALUES = 1 << 24

    def predict(self, ds, M=1000):
        """Offline prediction for a dataset with q (run, time, lev, y, x) (ann_model.py:95-113): the net's output is the
        sample and the mean, the variance is 0.  q is taken as float32, as the reference's stencils are."""
        from ..tools.simulate import dataset_backend
        xr = dataset_backend()
        qv = np.asarray(ds['q'].values).astype('float32')
        shape = qv.shape
        q = qv.reshape((-1,) + shape[-3:])
        n = q.shape[0]
        chunk = max(1, self.PREDICT_VALUES // int(np.prod(shape[-3:])))
        Y = np.empty(q.shape, np.float64)
        for s0 in range(0, n, chunk):
            qd = torch.as_tensor(q[s0:s0 + chunk]).cuda(self._gen.device).to(torch.float64).contiguous()
            Y[s0:s0 + chunk] = self._gen.forward(qd, None, demean=False).cpu().numpy()
        Y = Y.reshape(shape)
        dims = ['run', 'time', 'lev', 'y', 'x']
        return xr.Dataset({'q_forcing_advection': (dims, Y), 'q_forcing_advection_mean': (dims, Y),
                           'q_forcing_advection_var': (dims, Y * 0)})
