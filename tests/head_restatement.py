"""Test-side restatement of include/qgx_head_train.h in float64 numpy, and of MeanVarModel's two-stage fit on torch CPU.

Layouts are the ABI's: `engine` (B, N, N, 8) with channels C ... 7 zero, `planar` (n, C, N, N); idx is None (rows 0 ... B - 1)
or B row numbers of the planar array.

  batch_gather(src, idx, B)               engine layout of src[idx] (without idx: of the first B rows)
  head_loss(y, t, idx, mode)              sum (h(y) - t[idx])^2 / (B C N N)
  scale(gout, B, C, N)                    the ONE float32 number the device multiplies by: float32(gout * 2 / (B C N N)), the
                                          quotient formed in float64
  head_grad(y, t, idx, mode, gout)        scale (h(y) - t[idx]) h'(y) in the engine layout, pad channels zero (float64 products
                                          of the float32 scale: what a float32 product of integers rounds once)
  head_apply(y, t, idx, mode, C)          planar h(y), or (t[idx] - h(y))^2

mode 'mse': h(y) = y; 'softplus_mse': torch's softplus (beta 1, threshold 20): y if y > 20, else log1p(exp(y)), with
h' = exp(y) / (1 + exp(y)), and 1 where y > 20.  tests/test_head_train_cpu.py pins all of it to torch CPU autograd.
"""
import numpy as np

import conv_train_restatement as cr

MODES = {'mse': 0, 'softplus_mse': 1}


def head(y, mode):
    y = np.asarray(y, np.float64)
    if mode == 'mse':
        return y
    assert mode == 'softplus_mse'
    return np.where(y > 20, y, np.log1p(np.exp(np.minimum(y, 20))))


def slope(y, mode):
    y = np.asarray(y, np.float64)
    if mode == 'mse':
        return np.ones_like(y)
    e = np.exp(np.minimum(y, 20))
    return np.where(y > 20, 1.0, e / (1 + e))


def rows(idx, B):
    return np.arange(B) if idx is None else np.asarray(idx, np.int64)


def batch_gather(src, idx=None, B=None):
    """without idx: the first B rows (all of them without B)"""
    src = np.asarray(src)
    return cr.to_layout(src[rows(idx, len(src) if B is None else B)])


def _difference(y, t, idx, mode):
    """h(y) - t[idx], planar (B, C, N, N) float64"""
    y, t = np.asarray(y, np.float64), np.asarray(t, np.float64)
    C = t.shape[1]
    return head(cr.from_layout(y, C), mode) - t[rows(idx, len(y))]


def head_loss(y, t, idx, mode):
    d = _difference(y, t, idx, mode)
    return float((d * d).sum() / d.size)


def scale(gout, B, C, N):
    return np.float32(np.float64(gout) * 2.0 / np.float64(B * C * N * N))


def head_grad(y, t, idx, mode, gout):
    d = _difference(y, t, idx, mode)
    B, C, N = d.shape[0], d.shape[1], d.shape[-1]
    s = np.float64(scale(gout, B, C, N))
    return cr.to_layout(s * d * slope(cr.from_layout(np.asarray(y, np.float64), C), mode))


def head_apply(y, t, idx, mode, C):
    y = np.asarray(y, np.float64)
    if t is None:
        return head(cr.from_layout(y, C), mode)
    d = _difference(y, t, idx, mode)
    assert d.shape[1] == C
    return d * d


# ---- data of the kernel tests ------------------------------------------------------------------------------------------------
def case_data(B, N, C, n, seed, integer):
    """y in the engine layout (B, N, N, 8), src and t planar (n, C, N, N), float32.  integer: drawn from -8 ... 8, so that every
    difference, square and sum of the shapes tested is an integer far below 2^53 (and every difference below 2^24); else
    Gaussian, scaled so that the largest magnitude is 30, and y's first four values 30, -30, 20 and the next float32 above 20:
    both branches of softplus, its threshold and its flat tail"""
    rs = np.random.RandomState(seed)
    if integer:
        draw = lambda *s: rs.randint(-8, 9, size=s).astype(np.float32)
    else:
        def draw(*s):
            a = rs.randn(*s)
            return (a * (30.0 / np.abs(a).max())).astype(np.float32)
    y = draw(B, C, N, N)
    if not integer:
        y.reshape(-1)[:4] = [30, -30, 20, np.nextafter(np.float32(20), np.float32(21))]
    return cr.to_layout(y), draw(n, C, N, N), draw(n, C, N, N)


# ---- the nets and the two-stage fit ------------------------------------------------------------------------------------------
def var_net(n_in, n_out, hidden, dtype, state_dict=None):
    """the reference's VarCNN (mean_var_model.py:14-17): AndrewCNN whose forward ends in softplus; no parameter of its own"""
    import torch
    net = cr.torch_net(n_in, n_out, hidden, True, True, dtype, state_dict)
    conv = net.forward
    net.forward = lambda x: torch.nn.functional.softplus(conv(x))
    return net


def two_stage_fit(mean_state, var_state, hidden, X_train, Y_train, X_test, Y_test, num_epochs, batch_size, learning_rate, orders,
                  dtype):
    """MeanVarModel.fit (mean_var_model.py:41-64) on the CPU in `dtype` from the two initial state dicts: train net_mean with
    MSE, evaluate it in eval mode over both sets, train net_var on the squared residuals -> (log_mean, log_var, net_mean,
    net_var); the logs as conv_train_restatement.reference_loop gives them"""
    import torch
    net_mean = cr.torch_net(2, 2, hidden, True, True, dtype, mean_state)
    net_var = var_net(2, 2, hidden, dtype, var_state)
    data = [torch.as_tensor(np.asarray(a)).to(dtype) for a in (X_train, Y_train, X_test, Y_test)]
    log_mean = cr.reference_loop(net_mean, *data, num_epochs, batch_size, learning_rate, orders)
    net_mean.eval()
    with torch.no_grad():
        rsq_train = (data[1] - net_mean(data[0])) ** 2
        rsq_test = (data[3] - net_mean(data[2])) ** 2
    log_var = cr.reference_loop(net_var, data[0], rsq_train, data[2], rsq_test, num_epochs, batch_size, learning_rate, orders)
    return log_mean, log_var, net_mean, net_var


def noisy_fit_dataset(seed):
    """conv_train_restatement.fit_dataset's fields plus heteroscedastic noise on the target: 0.5 std(y) |q / std(q)| eps per
    layer, eps Gaussian from a seed of its own: a conditional variance for net_var to learn"""
    from pyqg_generative_amd.tools import xr_lite
    q, y = cr.fit_fields(seed)
    eps = np.random.RandomState(1000 + seed).randn(*q.shape)
    sd = lambda a: a.std(axis=(0, 1, 3, 4), keepdims=True)
    y = y + 0.5 * sd(y) * np.abs(q / sd(q)) * eps
    dims = ['run', 'time', 'lev', 'y', 'x']
    return xr_lite.Dataset({'q': (dims, q), 'q_forcing_advection': (dims, y)}), q, y
