"""Test-side restatement of OLSModel's inference (pyqg_generative/models/ols_model.py:65-75) on the oracle's CNN:
generate_latent_noise returns 0 and predict_snapshot(q, noise) = y_std * net(float32(q) / x_std), noise ignored.  It has
the interface oracle.gen_ref.ParameterizationRef calls, so it plugs into that and into oracle.qg_ref.QGModelRef unchanged.

The net is GZ's trained net_mean (tests/golden/weights_gz.npz), the AndrewCNN(2, 2) tests/golden/make_golden_ols.py
ran through the reference's OLSModel.
"""
import os

import numpy as np

from oracle.gen_ref import CNNWeights, ScalerRef, cnn_forward

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


class OLSRef:
    def __init__(self, net, x_std, y_std):
        self.nets = [net]
        self.x_scale = ScalerRef(x_std)
        self.y_scale = ScalerRef(y_std)

    @classmethod
    def from_fixture(cls):
        d = np.load(os.path.join(GOLDEN, 'weights_gz.npz'), allow_pickle=False)
        return cls(CNNWeights.from_npz_dict(d, 'net0_'), d['x_std'], d['y_std'])

    def generate_latent_noise(self, ny, nx, rng=None):
        return 0                                                          # ols_model.py:65-66

    def predict_snapshot(self, q, noise):
        """q: (2, N, N) or (T, 2, N, N) float64 -> S of the same shape, float64 (not de-meaned)"""
        X = self.x_scale.normalize(np.asarray(q).astype('float32'))       # ols_model.py:69
        if X.ndim == 3:
            X = X[None]
        return self.y_scale.denormalize(cnn_forward(self.nets[0], X)).squeeze().astype('float64')
