"""Test-side restatement of the DeepInversion U-Net generator (DeepInversionGenerator(4, 2), eval mode, float32) from a
flat state dict, written from the architecture description: conv32 -> res32_start -> down64 .. down512 -> res512 ->
up512 .. up64 -> res32_end -> conv_end, circular padding everywhere.

A residual unit is conv(bn(x)) + conv1(bn(x)), conv = LeakyReLU(0.2) -> 3x3 -> bn2 -> LeakyReLU(0.2) -> 3x3, conv1 1x1.
The LeakyReLUs are in place: in the two bn='None' units the first one overwrites x itself, so their skip sees
LeakyReLU(x); in the BatchNorm units bn(x) is a fresh tensor and the skip sees BN(x).

Device-agnostic torch: the CPU tests run it on the CPU, bench_tools/unet_time.py on the GPU as the timing yardstick.
"""
import torch
import torch.nn.functional as F

UNITS = [('res32_start', False), ('down64.conv.1', True), ('down128.conv.1', True), ('down256.conv.1', True),
         ('down512.conv.1', True), ('res512', True), ('up512.conv', True), ('up256.conv', True), ('up128.conv', True),
         ('up64.conv', True), ('res32_end', False)]


def _conv3(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='circular'), w, b)


def _bn(x, sd, p, eps=1e-5):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'],
                        False, 0.0, eps)


def _res(x, sd, p, bn):
    xb = _bn(x, sd, p + '.bn') if bn else F.leaky_relu(x, 0.2)     # bn='None': x overwritten by the in-place LeakyReLU
    a = _conv3(F.leaky_relu(xb, 0.2) if bn else xb, sd[p + '.conv.1.weight'], sd[p + '.conv.1.bias'])
    if bn:
        a = _bn(a, sd, p + '.conv.2')
    a = _conv3(F.leaky_relu(a, 0.2), sd[p + '.conv.4.weight'], sd[p + '.conv.4.bias'])
    return a + F.conv2d(xb, sd[p + '.conv1.weight'], sd[p + '.conv1.bias'])


def to_torch(net, device='cpu'):
    return {k: torch.as_tensor(v, dtype=torch.float32, device=device) for k, v in net.items()}


@torch.no_grad()
def forward(sd, x, keep=None):
    """x (B, 4, N, N) float32 tensor -> (B, 2, N, N); keep: optional dict that receives the bottleneck (res512 output)"""
    h = _conv3(x, sd['conv32.weight'], sd['conv32.bias'])
    skips = [_res(h, sd, 'res32_start', False)]
    for i in range(1, 5):
        skips.append(_res(F.avg_pool2d(skips[-1], 2), sd, UNITS[i][0], True))
    h = _res(skips.pop(), sd, 'res512', True)
    if keep is not None:
        keep['bottleneck'] = h
    for i, up in enumerate(('up512', 'up256', 'up128', 'up64')):
        u = F.conv_transpose2d(h, sd[up + '.upsampling.weight'], sd[up + '.upsampling.bias'], stride=2)
        h = _res(torch.cat((u, skips.pop()), dim=1), sd, up + '.conv', True)
    h = _res(h, sd, 'res32_end', False)
    return F.conv2d(h, sd['conv_end.weight'], sd['conv_end.bias'])
