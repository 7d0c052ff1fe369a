"""CVAE decoder parameterization, inference surface of
pyqg_generative/models/cvae_regression.py (:18-52 constructor, :114-118 generate,
:128-145 generate_latent_noise / predict_snapshot / predict_mean_snapshot)."""
from .cgan_regression import _LatentCNN


class CVAERegression(_LatentCNN):
    kind = 'vae'
    NET_NAMES = ('decoder',)

    def __init__(self, regression='None', folder='model', div=False, decoder_var='adaptive',
                 hidden_channels=[128, 64, 32, 32, 32, 32, 32], device=0, **kw):
        # div=True (:45, :50): decoder and net_mean in flux form, the divergence on the device; hidden_channels reaches the
        # decoder alone (:45) — net_mean keeps the default widths (:50), the encoder is training-only
        from ..weights import check_hidden_channels
        self._set_regression(regression)
        self.div, self.decoder_var = bool(div), decoder_var
        self.hidden_channels = check_hidden_channels(hidden_channels)
        self._load(folder, device)          # needs decoder.pt (the encoder is training-only), net_mean.pt with regression != 'None'
