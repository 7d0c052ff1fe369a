"""Deterministic CNN parameterization (the "MSE" baseline), inference surface of
pyqg_generative/models/ols_model.py (:13-31 constructor, :57-66 load_model, :68-75 generate_latent_noise /
predict_snapshot, :77-94 predict)."""
import os
import numpy as np

from .parameterization import Parameterization
from ..tools.cnn_tools import apply_function
from ..weights import check_hidden_channels

HIDDEN = [128, 64, 32, 32, 32, 32, 32]


class OLSModel(Parameterization):
    kind = 'ols'
    NET_NAMES = ('net',)

    def __init__(self, div=False, batch_norm=True, bias=True, final_activation='None',
                 hidden_channels=[128, 64, 32, 32, 32, 32, 32], folder='model', device=0):
        # AndrewCNN(2, 2, batch_norm=, bias=, div=, hidden_channels=) (ols_model.py:29-31).  The default widths with BatchNorm
        # and bias run the shipped kernels, every other admitted architecture (1 ... 7 widths of 1 ... 256) the generic engine;
        # div=True: a four-channel last layer and the device's divergence behind it
        if final_activation != 'None':
            raise NotImplementedError(f'final_activation={final_activation!r} has no device path: the reference evaluates the '
                                      "string with eval(), an arbitrary function of the output; only 'None' runs")
        self.div, self.batch_norm, self.bias = bool(div), bool(batch_norm), bool(bias)
        self.final_activation, self.hidden_channels = final_activation, check_hidden_channels(hidden_channels)
        # the reference builds an untrained net when the folder holds none (ols_model.py:57-60); there is no training here
        if not os.path.exists(os.path.join(folder, 'net.pt')):
            raise FileNotFoundError(f'{os.path.join(folder, "net.pt")} is missing: OLSModel needs a trained model folder '
                                    '(net.pt, x_scale.json, y_scale.json)')
        self._load(folder, device)

    def generate_latent_noise(self, ny, nx):
        return 0

    def predict_snapshot(self, m, noise):
        """S = y_std * net(q / x_std) for ONE snapshot (2, N, N) or a batch (B, 2, N, N); `noise` is ignored"""
        return self._forward(m.q, None, demean=False)

    def predict(self, ds, M=1000):
        """Offline prediction for a dataset with q (run, time, lev, y, x) (ols_model.py:77-94): the net's output is the
        sample and the mean, the variance is 0."""
        from ..tools.simulate import dataset_backend
        xr = dataset_backend()
        qv = np.asarray(ds['q'].values)
        X = self.x_scale.normalize(qv.reshape((-1,) + qv.shape[-3:]).astype('float32'))
        Y = self.y_scale.denormalize(apply_function(self.net, X)).reshape(qv.shape)
        dims = ['run', 'time', 'lev', 'y', 'x']
        return xr.Dataset({'q_forcing_advection': (dims, Y), 'q_forcing_advection_mean': (dims, Y),
                           'q_forcing_advection_var': (dims, Y * 0)})
