"""Test-side restatement of the differentiable circular convolution of include/qgx_conv_train.h, in float64 numpy and in the
ABI's layout: activations (B, N, N, C8) with C8 = channels rounded up to 8 and zero pad channels, weights (cout, cin, k, k).

  forward(x, w, b)                  y  = conv_circular(x, w) + b
  backward_data(dy, w)              dx[b, ci, y, x] = sum dy[b, co, y - ky + P, x - kx + P] w[co, ci, ky, kx]
  backward_weight(x, dy, cin, k)    dw[co, ci, ky, kx] = sum dy[b, co, y, x] x[b, ci, y + ky - P, x + kx - P],  db = sum dy

tests/test_conv_train_cpu.py pins the three to torch CPU autograd of F.conv2d(F.pad(x, circular), w, b), and the identity the
device's data gradient rests on: backward_data(dy, w) = forward(dy, flip_transpose(w)).  The net restated for the training
tests (TorchNet) is the reference's AndrewCNN block order on plain torch modules, in any dtype, on the CPU.
"""
import numpy as np

from arch_restatement import conv_circular


def c8(c):
    return (int(c) + 7) // 8 * 8


def to_layout(a):
    """planar (B, C, N, N) -> (B, N, N, C8) with zero pad channels, same dtype"""
    B, C, N = a.shape[0], a.shape[1], a.shape[-1]
    out = np.zeros((B, N, N, c8(C)), a.dtype)
    out[..., :C] = np.transpose(a, (0, 2, 3, 1))
    return out


def from_layout(a, C):
    """(B, N, N, C8) -> planar (B, C, N, N)"""
    return np.ascontiguousarray(np.transpose(a[..., :C], (0, 3, 1, 2)))


def flip_transpose(w):
    """w'[ci, co, ky, kx] = w[co, ci, k - 1 - ky, k - 1 - kx]"""
    return np.ascontiguousarray(np.transpose(w, (1, 0, 2, 3))[:, :, ::-1, ::-1])


def forward(x, w, b=None):
    w = np.asarray(w, np.float64)
    y = conv_circular(from_layout(np.asarray(x, np.float64), w.shape[1]), w, None if b is None else np.asarray(b, np.float64))
    return to_layout(y)


def backward_data(dy, w):
    """the definition, tap by tap (NOT through the flipped-weights identity, which the CPU test checks against this)"""
    w = np.asarray(w, np.float64)
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    p = k // 2
    g = from_layout(np.asarray(dy, np.float64), cout)
    dx = np.zeros((g.shape[0], cin) + g.shape[2:])
    for ky in range(k):
        for kx in range(k):
            # dx[y, x] += dy[y - ky + P, x - kx + P] w[ky, kx]: roll dy by (ky - P, kx - P)
            dx += np.einsum('oc,boyx->bcyx', w[:, :, ky, kx], np.roll(g, (ky - p, kx - p), axis=(2, 3)), optimize=True)
    return to_layout(dx)


def backward_weight(x, dy, cin, cout, k):
    p = k // 2
    xs, g = from_layout(np.asarray(x, np.float64), cin), from_layout(np.asarray(dy, np.float64), cout)
    dw = np.zeros((cout, cin, k, k))
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = np.einsum('boyx,bcyx->oc', g, np.roll(xs, (p - ky, p - kx), axis=(2, 3)))
    return dw, g.sum(axis=(0, 2, 3))


def case_data(cin, cout, k, B, N, seed, integer):
    """x, w, bias, dy of one case in the ABI's layout (float32, zero pad channels); integer: drawn from -3 ... 3, so that every
    product and partial sum of the shapes tested stays an integer below 2^24"""
    rs = np.random.RandomState(seed)
    if integer:
        draw = lambda *s: rs.randint(-3, 4, size=s).astype(np.float32)
    else:
        draw = lambda *s: rs.randn(*s).astype(np.float32)
    x, dy = to_layout(draw(B, cin, N, N)), to_layout(draw(B, cout, N, N))
    return x, draw(cout, cin, k, k), draw(cout), dy


# ---- the net of the training tests --------------------------------------------------------------------------------------
def torch_net(n_in, n_out, hidden, batch_norm, bias, dtype, state_dict=None):
    """the reference's AndrewCNN (cnn_tools.py:79-98, 125-163): Conv2d(padding='same', padding_mode='circular') -> ReLU ->
    [BatchNorm2d] blocks in one nn.Sequential `conv`, kernels 5, 5, 3, ..., the last block the convolution alone"""
    import torch
    from torch import nn
    from pyqg_generative_amd import weights
    ch = [n_in] + list(hidden) + [n_out]
    ks = weights.arch_kernels(list(hidden))
    blocks = []
    for l in range(len(ch) - 1):
        blocks.append(nn.Conv2d(ch[l], ch[l + 1], ks[l], padding='same', padding_mode='circular', bias=bias))
        if l < len(ch) - 2:
            blocks.append(nn.ReLU())
            if batch_norm:
                blocks.append(nn.BatchNorm2d(ch[l + 1]))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Sequential(*blocks)

        def forward(self, x):
            return self.conv(x)

        def compute_loss(self, x, y):
            return {'loss': nn.functional.mse_loss(self.forward(x), y)}
    net = Net().to(dtype)
    if state_dict is not None:
        net.load_state_dict({k: v.detach().cpu().to(dtype if v.dtype.is_floating_point else v.dtype) for k, v in state_dict.items()})
    return net


def lr_sequence(E, lr):
    """train()'s schedule restated without torch: epoch e runs at lr * 0.1^(milestones <= e) — a milestone listed twice
    counts twice, as torch's Counter does, and a milestone 0 (a small E) fires when the scheduler is built"""
    ms = [int(E / 2), int(E * 3 / 4), int(E * 7 / 8)]
    return [float(lr) * 0.1 ** sum(1 for m in ms if m <= e) for e in range(E)]


def reference_loop(net, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, orders):
    """train (cnn_tools.py:645-700) with evaluate_test (:624-643) on CPU tensors of the net's dtype, the batch order given by
    orders(epoch, n) in place of the shuffle: Adam, MultiStepLR stepped per epoch, the epoch's mean losses -> {'loss': [...],
    'loss_test': [...]}"""
    import torch
    dtype = next(net.parameters()).dtype
    X_train, Y_train, X_test, Y_test = (torch.as_tensor(np.asarray(a)).to(dtype) for a in (X_train, Y_train, X_test, Y_test))
    E, n = int(num_epochs), len(X_train)
    net.train()
    optimizer = torch.optim.Adam(net.parameters(), lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    log = {'loss': [], 'loss_test': []}
    for epoch in range(E):
        order = torch.as_tensor(np.asarray(orders(epoch, n), dtype=np.int64))
        tot = 0.0
        for s in range(0, n, batch_size):
            idx = order[s:s + batch_size]
            optimizer.zero_grad()
            loss = net.compute_loss(X_train[idx], Y_train[idx])['loss']
            loss.backward()
            optimizer.step()
            tot += float(loss.detach()) * len(idx)
        scheduler.step()
        log['loss'].append(tot / n)
        net.eval()
        tot = 0.0
        with torch.no_grad():
            for s in range(0, len(X_test), batch_size):
                x, y = X_test[s:s + batch_size], Y_test[s:s + batch_size]
                tot += float(net.compute_loss(x, y)['loss']) * len(x)
        net.train()
        log['loss_test'].append(tot / len(X_test))
    return log


def fixed_orders(seed):
    """orders(epoch, n): a permutation per epoch from a seed of its own (no global stream)"""
    return lambda epoch, n: np.random.RandomState(seed + epoch).permutation(n)


# ---- the dataset of the end-to-end fit -----------------------------------------------------------------------------------
STENCIL = np.array([[0.5, -1.0, 0.0], [2.0, -3.0, 1.0], [0.0, 1.0, -0.5]])
FIT = dict(hidden_channels=[8], batch_size=4, learning_rate=0.01, seed=3, N=16, runs=2, times=6)


def fit_fields(seed):
    """q (runs, times, 2, N, N) Gaussian at the layers' physical scales, and q_forcing_advection = 1e-6 * the fixed circular
    3 x 3 stencil of q: something a net with one hidden layer can learn"""
    f = FIT
    q = np.random.RandomState(seed).randn(f['runs'], f['times'], 2, f['N'], f['N']) * np.array([8e-6, 1e-6]).reshape(1, 1, 2, 1, 1)
    y = np.zeros_like(q)
    for dy in range(3):
        for dx in range(3):
            y += STENCIL[dy, dx] * np.roll(q, (1 - dy, 1 - dx), axis=(-2, -1))
    return q, 1e-6 * y


def fit_dataset(seed):
    from pyqg_generative_amd.tools import xr_lite
    q, y = fit_fields(seed)
    dims = ['run', 'time', 'lev', 'y', 'x']
    return xr_lite.Dataset({'q': (dims, q), 'q_forcing_advection': (dims, y)})
