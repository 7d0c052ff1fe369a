"""DeepInversionGenerator(4, 2), the U-Net generator of CGANRegression(generator='DeepInversion') (reference:
tools/deep_inversion.py:44-160), as a trainable module whose convolutions run on the device kernels.

``TrainableUNet`` has the reference's module tree, hence its state-dict keys, shapes and order (a G.pt it writes loads in the
reference and in ``CGANRegression(generator='DeepInversion', folder=...)``), and two forwards of one function:

  forward(x)          planar (B, 4, N, N) -> (B, 2, N, N) through torch ops (F.conv2d on circular padding, F.conv_transpose2d,
                      F.avg_pool2d, F.batch_norm): the comparison side; any device, any floating dtype
  forward_engine(a)   (B, N, N, 8) = [x1, x2, z1, z2, 0, ...] -> (B, N, N, 8) = [y1, y2, 0, ...] in the engine layout: every
                      convolution is ``train_ops.unet_conv2d`` (csrc/uconv_train.hip), a ConvTranspose2d(C, C/2, 2, stride=2)
                      is the 1 x 1 convolution to 4 C/2 channels with the weight permuted to rows (ky, kx, co) and a torch
                      reshape onto the 2 x finer grid; pooling, concatenation, the residual add, BatchNorm (F.batch_norm on the
                      zero-copy channels_last view) and LeakyReLU are torch ops on the layout

What the reference's module does in train mode, and this one reproduces:

  * a residual unit is conv(bn(x)) + conv1(bn(x)) with in-place LeakyReLUs.  In the two bn='None' units (res32_start, res32_end)
    bn is the identity, the first LeakyReLU overwrites x itself, and the skip sees conv1(LeakyReLU(x)); in the BatchNorm units
    bn(x) is a fresh tensor each time and the skip sees conv1(BN(x)).
  * bn(x) is evaluated TWICE per BatchNorm unit: its running statistics are updated twice per forward with the same batch
    statistics and its num_batches_tracked goes up by 2 (that of conv.2 by 1).  Here the normalisation is computed once and the
    second update is applied explicitly.
  * the reference's weights_init matches class names containing 'Conv', so it draws the ConvTranspose2d weights from
    N(0, 0.02) as well; ``unet_weights_init`` does.

``slopes`` / ``use_slopes``: LeakyReLU is written y * slope(y) with the slopes (1 or 0.2) a constant of the graph.  Given a list
``slopes``, each of the 22 sites appends its slope tensor in call order; given ``use_slopes``, the sites take their slopes from
that list instead of from the sign.  Both forwards record and take them planar, (B, C, n, n), so a list goes from one to the other.  Two
evaluations in different arithmetic then evaluate the same smooth function, which is what a gradient comparison needs: a
single sign flip of a near-zero input changes a gradient by 1e-3 ... 1e-1 of its largest entry.
"""
import torch
from torch import nn
import torch.nn.functional as F

from .train_ops import unet_conv2d

UNET_GRIDS = (32, 48, 64, 96, 128)         # what the device inference of the U-Net admits (csrc/unet.hip: unet_size_ok)
SLOPE = 0.2
N_SITES = 22


def unet_layer_shapes(N):
    """every unet_conv2d call of one forward_engine at an N x N input, in call order, as (cin, cout, k, grid)"""
    unit = lambda ci, co, n: [(ci, co, 3, n), (co, co, 3, n), (ci, co, 1, n)]
    out = [(4, 32, 3, N)] + unit(32, 32, N)
    for i, (ci, co) in enumerate(TrainableUNet.DOWN):
        out += unit(ci, co, N >> (i + 1))
    out += unit(512, 512, N >> 4)
    for i, c in enumerate(TrainableUNet.UP):
        out += [(c, 2 * c, 1, N >> (4 - i))] + unit(c, c // 2, N >> (3 - i))
    return out + unit(32, 32, N) + [(32, 2, 1, N)]


def unet_weights_init(m):
    """the reference's weights_init (cnn_tools.py:54-65) as it acts on this net: Conv2d AND ConvTranspose2d weights N(0, 0.02),
    BatchNorm weights N(1, 0.02) and biases 0; convolution biases keep torch's default"""
    if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif isinstance(m, nn.BatchNorm2d):
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


def _unit(cin, cout, bn):
    """res_unit(cin, cout, bn): the module tree alone (keys bn.*, conv.1.*, conv.2.*, conv.4.*, conv1.*)"""
    m = nn.Module()
    m.bn = nn.BatchNorm2d(cin) if bn else nn.Identity()
    m.conv = nn.Sequential(nn.LeakyReLU(SLOPE), nn.Conv2d(cin, cout, 3, padding=1, padding_mode='circular'),
                           nn.BatchNorm2d(cout) if bn else nn.Identity(), nn.LeakyReLU(SLOPE),
                           nn.Conv2d(cout, cout, 3, padding=1, padding_mode='circular'))
    m.conv1 = nn.Conv2d(cin, cout, 1)
    return m


class _Ops:
    """the operations the two forwards differ in; x is planar (B, C, n, n) or in the engine layout (B, n, n, C)"""

    def __init__(self, engine, training, slopes, use_slopes):
        self.engine, self.training, self.slopes = engine, training, slopes
        self.use = None if use_slopes is None else list(use_slopes)
        self.site = 0

    def conv(self, x, m):
        if self.engine:
            return unet_conv2d(x, m.weight, m.bias)
        p = m.kernel_size[0] // 2
        return F.conv2d(F.pad(x, (p, p, p, p), mode='circular') if p else x, m.weight, m.bias)

    def up(self, x, m):
        """ConvTranspose2d(C, C/2, 2, stride=2): out[b, co, 2i + ky, 2j + kx] = sum_c x[b, c, i, j] W[c, co, ky, kx] + bias[co]"""
        if not self.engine:
            return F.conv_transpose2d(x, m.weight, m.bias, stride=2)
        C, Ch = int(m.weight.shape[0]), int(m.weight.shape[1])
        B, n = int(x.shape[0]), int(x.shape[1])
        y = unet_conv2d(x, m.weight.permute(2, 3, 1, 0).reshape(4 * Ch, C, 1, 1), m.bias.repeat(4))   # channels (ky, kx, co)
        return y.reshape(B, n, n, 2, 2, Ch).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * n, 2 * n, Ch)

    def pool(self, x):
        if not self.engine:
            return F.avg_pool2d(x, 2)
        return F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)       # channels_last in, channels_last out: no copy

    def cat(self, a, b):
        return torch.cat((a, b), dim=-1 if self.engine else 1)

    def bn(self, x, m, updates=1):
        """BatchNorm2d m on x; in train mode the running statistics are updated `updates` times with the batch's statistics and
        the counter goes up by as much, as `updates` evaluations of the module would"""
        xv = x.permute(0, 3, 1, 2) if self.engine else x                         # the zero-copy channels_last view
        if self.training:
            # F.batch_norm keeps the two buffers for its backward, and its own update of them does not count as a modification;
            # an explicit one does, and two forwards precede one backward in a GAN's step: hence .data, whose writes autograd
            # does not count either
            with torch.no_grad():
                if updates > 1:
                    var, mean = torch.var_mean(xv, dim=(0, 2, 3), unbiased=True)
                for _ in range(updates - 1):
                    m.running_mean.data.mul_(1 - m.momentum).add_(mean, alpha=m.momentum)
                    m.running_var.data.mul_(1 - m.momentum).add_(var, alpha=m.momentum)
                m.num_batches_tracked += updates
            y = F.batch_norm(xv, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)
        else:
            y = F.batch_norm(xv, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
        return y.permute(0, 2, 3, 1) if self.engine else y

    def lrelu(self, y):
        with torch.no_grad():
            if self.use is None:
                # two Python scalars give float32; another dtype takes SLOPE rounded to it, not float32's 0.2
                s = torch.where(y > 0, 1.0, SLOPE) if y.dtype == torch.float32 else torch.where(y > 0, 1.0, y.new_full((), SLOPE))
            else:
                if self.site >= len(self.use):
                    raise ValueError(f'use_slopes: {len(self.use)} tensors for more than {self.site} LeakyReLU sites')
                s = torch.as_tensor(self.use[self.site]).to(device=y.device, dtype=y.dtype)
                s = s.permute(0, 2, 3, 1) if self.engine else s
                if s.shape != y.shape:
                    raise ValueError(f'use_slopes[{self.site}]: {tuple(self.use[self.site].shape)} is not the site\'s planar shape')
        self.site += 1
        if self.slopes is not None:
            self.slopes.append(s.permute(0, 3, 1, 2) if self.engine else s)
        return y * s

    def unit(self, x, m):
        """res_unit (see the module docstring): a BatchNorm unit normalises once and feeds both branches; a bn='None' unit's
        skip sees the LeakyReLU the reference applies in place"""
        if isinstance(m.bn, nn.BatchNorm2d):
            t = self.bn(x, m.bn, updates=2)
            a = self.bn(self.conv(self.lrelu(t), m.conv[1]), m.conv[2])
        else:
            t = self.lrelu(x)
            a = self.conv(t, m.conv[1])
        return self.conv(self.lrelu(a), m.conv[4]) + self.conv(t, m.conv1)


class TrainableUNet(nn.Module):
    """DeepInversionGenerator(4, 2): conv32 -> res32_start -> down64 ... down512 (AvgPool2d(2), residual unit) -> res512 ->
    up512 ... up64 (ConvTranspose2d, concatenation with the skip, residual unit) -> res32_end -> conv_end, circular padding
    everywhere.  Constructed under `seed` (torch's defaults for the biases, unet_weights_init for the rest), without touching
    the global torch stream.  See the module docstring for the two forwards and the hook."""

    DOWN = ((32, 64), (64, 128), (128, 256), (256, 512))
    UP = (512, 256, 128, 64)

    def __init__(self, seed=0):
        super().__init__()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            self.conv32 = nn.Conv2d(4, 32, 3, padding=1, padding_mode='circular')
            self.res32_start = _unit(32, 32, False)
            for ci, co in self.DOWN:
                d = nn.Module()
                d.conv = nn.Sequential(nn.AvgPool2d(2, 2), _unit(ci, co, True))
                setattr(self, f'down{co}', d)
            self.res512 = _unit(512, 512, True)
            for c in self.UP:
                u = nn.Module()
                u.upsampling = nn.ConvTranspose2d(c, c // 2, 2, stride=2)
                u.conv = _unit(c, c // 2, True)
                setattr(self, f'up{c}', u)
            self.res32_end = _unit(32, 32, False)
            self.conv_end = nn.Conv2d(32, 2, 1)
            self.apply(unet_weights_init)
        self.seed = int(seed)

    def _run(self, o, x):
        h = o.unit(o.conv(x, self.conv32), self.res32_start)
        skips = [h]
        for _, co in self.DOWN:
            skips.append(o.unit(o.pool(skips[-1]), getattr(self, f'down{co}').conv[1]))
        h = o.unit(skips.pop(), self.res512)
        for c in self.UP:
            u = getattr(self, f'up{c}')
            h = o.unit(o.cat(o.up(h, u.upsampling), skips.pop()), u.conv)
        y = o.conv(o.unit(h, self.res32_end), self.conv_end)
        if o.use is not None and o.site != len(o.use):
            raise ValueError(f'use_slopes: {len(o.use)} tensors for {o.site} LeakyReLU sites')
        return y

    @staticmethod
    def _check_grid(n):
        if n % 16 or n < 32:
            raise ValueError(f'a {n} x {n} grid: the U-Net halves it four times and keeps at least 2 x 2')

    def forward(self, x, slopes=None, use_slopes=None):
        """planar (B, 4, N, N) -> (B, 2, N, N) through torch ops, in x's dtype and on its device"""
        if x.dim() != 4 or x.shape[1] != 4 or x.shape[2] != x.shape[3]:
            raise ValueError(f'input {tuple(x.shape)}: expected (B, 4, N, N)')
        self._check_grid(int(x.shape[-1]))
        return self._run(_Ops(False, self.training, slopes, use_slopes), x)

    def forward_engine(self, a, slopes=None, use_slopes=None):
        """(B, N, N, 8) = [x1, x2, z1, z2, 0, 0, 0, 0] float32 on the device -> (B, N, N, 8) = [y1, y2, 0, ...]"""
        if a.dim() != 4 or a.shape[1] != a.shape[2] or a.shape[3] != 8:
            raise ValueError(f'input {tuple(a.shape)}: expected (B, N, N, 8)')
        self._check_grid(int(a.shape[1]))
        return self._run(_Ops(True, self.training, slopes, use_slopes), a)
