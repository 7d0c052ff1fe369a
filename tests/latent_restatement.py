"""Test-side restatement of include/qgx_latent_train.h in float64 numpy, and of CVAERegression's loss and loop
(cvae_regression.py:165-231 forward / compute_loss, :256-320 train_CVAE) on torch CPU modules in any dtype.

Layouts are the ABI's: `engine` (B, N, N, 8), `planar` (n, C, N, N); idx is None (rows 0 ... B - 1) or B row numbers.

  latent_forward(enc, x, idx, eps)            dec_in (B, N, N, 8) = [x[idx], eps std + mu, 0 ...], the three statistics, and the
                                              magnitude sums the bounds are stated in
  scale(gout, B)                              the ONE float32 number the device multiplies by: float32(gout / B), formed in float64
  latent_backward(enc, eps, d_dec_in, gout)   d_enc (B, N, N, 8) = [dz + s mu, 0.5 dz eps std + 0.5 s (var - 1), 0 ...] and its
                                              magnitudes
  normals(seed, step, B, N)                   the eps the device draws: oracle.samplers_ref.philox_normal(seed, b, step, 2 N N)

An elementwise bound is 16 * 2^-24 * A with A the float64 value of the expression with every term replaced by its magnitude; a
sum's bound is 2^-24 * sum |term|.  tests/test_latent_train_cpu.py pins the two calls to torch CPU autograd of the loss as the
reference writes it.
"""
import numpy as np

import conv_train_restatement as cr

EPS32 = 2.0 ** -24
ELEMENTWISE = 16 * EPS32
DEFAULT_HIDDEN = [128, 64, 32, 32, 32, 32, 32]
KEYS = ['loss', 'loss_recon', 'loss_KL', 'MSE', 'var_latent', 'var_aggr']


LATENT_BLOCK, LATENT_MAX_PARTIALS, LATENT_SUMS = 256, 256, 4


def latent_plan(B, N):
    """how csrc/latent_train.hip cuts the sums: a lane owns quads of four pixels; at most 256 ranges of qpb quads, qpb a multiple
    of the block of 256 threads; a thread of the forward kernel takes `passes` quads"""
    cdiv = lambda a, b: (a + b - 1) // b
    nq = B * N * N // 4
    nb = min(cdiv(nq, LATENT_BLOCK), LATENT_MAX_PARTIALS)
    qpb = cdiv(cdiv(nq, nb), LATENT_BLOCK) * LATENT_BLOCK
    nb = cdiv(nq, qpb)
    return dict(nq=nq, nb=nb, qpb=qpb, last_quads=nq - (nb - 1) * qpb, passes=qpb // LATENT_BLOCK)


def latent_workspace_bytes(B, N):
    """four float64 per range, rounded up to 256 bytes: the size resolves nb to 8 ranges only"""
    return (latent_plan(B, N)['nb'] * LATENT_SUMS * 8 + 255) // 256 * 256


# the GPU cases (B, N, n rows of x) and the regime each is there for, as data: every key is asserted against latent_plan
LATENT_REGIMES = {
    (3, 16, 5): dict(nq=192, nb=1, last_quads=192, passes=1),          # 768 pixels: a partial block when a lane owns four
    (1, 48, 1): dict(nb=3, last_quads=64, passes=1),                   # a grid that is no power of two; a last block of one wave
    (2, 96, 2): dict(nb=18, last_quads=256, passes=1),
    (17, 128, 17): dict(nb=136, qpb=512, passes=2),                    # 278 528 pixels > 1024 * 256: a lane takes two quads
}


def rows(idx, B):
    return np.arange(B) if idx is None else np.asarray(idx, np.int64)


def _parts(enc):
    """mu, logvar, std, var planar (B, 2, N, N) float64 of an engine-layout enc"""
    e = cr.from_layout(np.asarray(enc, np.float64), 4)
    mu, lv = e[:, :2], e[:, 2:]
    std = np.exp(0.5 * lv)
    return mu, lv, std, std * std


def latent_forward(enc, x, idx, eps):
    """-> dict(dec_in, A_dec_in, stats (3), stat_bounds (3)); enc None is the prior (no statistics)"""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    B, N = eps.shape[0], eps.shape[-1]
    xs = x[rows(idx, B)]
    if enc is None:
        mu, lv, std, var = np.zeros_like(eps), np.zeros_like(eps), np.ones_like(eps), np.ones_like(eps)
    else:
        mu, lv, std, var = _parts(enc)
    z = eps * std + mu
    out = dict(dec_in=cr.to_layout(np.concatenate([xs, z], 1)),
               A_dec_in=cr.to_layout(np.concatenate([np.zeros_like(xs), np.abs(eps) * std + np.abs(mu)], 1)))
    if enc is not None:
        n = mu.size
        kl = 0.5 * (mu * mu + var - 1 - lv)
        var_latent = var.sum() / n
        centred = mu - mu.sum() / n
        out['stats'] = np.array([kl.sum() / B, var_latent, (centred * centred).sum() / (n - 1) + var_latent])
        kl_abs = (0.5 * (mu * mu + var + 1 + np.abs(lv))).sum() / B
        out['stat_bounds'] = EPS32 * np.array([kl_abs, var_latent, (centred * centred).sum() / (n - 1) + var_latent])
    return out


def scale(gout, B):
    return np.float32(np.float64(gout) / np.float64(B))


def latent_backward(enc, eps, d_dec_in, gout):
    """-> (d_enc, A) in the engine layout, float64; the products take the float32 scale"""
    mu, lv, std, var = _parts(enc)
    eps = np.asarray(eps, np.float64)
    dz = cr.from_layout(np.asarray(d_dec_in, np.float64), 4)[:, 2:]
    s = np.float64(scale(gout, len(mu)))
    d_mu = dz + s * mu
    d_lv = 0.5 * dz * eps * std + 0.5 * s * (var - 1)
    A_mu = np.abs(dz) + np.abs(s * mu)
    A_lv = 0.5 * np.abs(dz * eps) * std + 0.5 * np.abs(s) * (var + 1)
    return cr.to_layout(np.concatenate([d_mu, d_lv], 1)), cr.to_layout(np.concatenate([A_mu, A_lv], 1))


def normals(seed, step, B, N):
    """planar (B, 2, N, N) float32: element c N N + y N + x of member b's 2 N N normals"""
    from oracle.samplers_ref import philox_normal
    return np.stack([philox_normal(seed, b, step, 2 * N * N)[0].reshape(2, N, N) for b in range(B)]).astype(np.float32)


def case_data(B, N, n, seed):
    """enc, d_dec_in in the engine layout (4 channels, zero pads), x planar (n, 2, N, N), eps planar (B, 2, N, N), float32:
    Gaussian, mu of scale 1.5 around 0.25 (a mean for var_aggr to remove), logvar of scale 1 (std from 0.1 to 8)"""
    rs = np.random.RandomState(seed)
    draw = lambda *s: rs.randn(*s).astype(np.float32)
    e = draw(B, 4, N, N)
    e[:, :2] = 1.5 * e[:, :2] + 0.25
    return cr.to_layout(e), draw(n, 2, N, N), draw(B, 2, N, N), cr.to_layout(draw(B, 4, N, N))


# ---- the loss, the model and the loop on torch CPU -------------------------------------------------------------------------
def latent_torch(enc, eps):
    """(z, loss_KL, var_latent, var_aggr) of planar enc (B, 4, N, N) as cvae_regression.py:172-178, :206, :220, :227-228 write them"""
    import torch
    mu, logvar = enc[:, :2], enc[:, 2:]
    std = torch.exp(0.5 * logvar)
    var = torch.square(std)
    z = eps * std + mu
    loss_KL = (0.5 * (torch.square(mu) + var - 1 - logvar)).sum(dim=(1, 2, 3)).mean()
    return z, loss_KL, var.mean(), mu.var() + var.mean()


class TorchCVAE:
    """CVAERegression's three nets (cvae_regression.py:45-50) on torch CPU modules in `dtype`, from state dicts, and its
    compute_loss (:180-231) with eps given"""

    def __init__(self, regression, decoder_var, div, hidden, dtype, states):
        import flux_train_restatement as fr
        dec = (lambda *a: fr.flux_torch_net(4, *a[2:])) if div else cr.torch_net
        mean = (lambda *a: fr.flux_torch_net(2, *a[2:])) if div else cr.torch_net
        self.encoder = cr.torch_net(4, 4, DEFAULT_HIDDEN, True, True, dtype, states['encoder'])
        self.decoder = dec(4, 2, list(hidden), True, True, dtype, states['decoder'])
        self.net_mean = mean(2, 2, DEFAULT_HIDDEN, True, True, dtype, states['net_mean']) if regression != 'None' else None
        self.regression, self.decoder_var, self.dtype = regression, decoder_var, dtype

    def modules(self):
        return [self.encoder, self.decoder]

    def compute_loss(self, x, y, ymean, eps):
        import torch
        z, loss_KL, var_latent, var_aggr = latent_torch(self.encoder(torch.cat([x, y], 1)), eps)
        yhat = self.decoder(torch.cat([x, z], 1))
        if self.regression != 'None':
            yhat = yhat + ymean
        sq = torch.square(yhat - y)
        var_p = {'adaptive': sq.mean().item(), 'fixed': 1.0}.get(self.decoder_var, self.decoder_var)
        loss_recon = 1 / (2. * var_p) * sq.sum(dim=(1, 2, 3)).mean()
        return {'loss': loss_recon + loss_KL, 'loss_recon': loss_recon, 'loss_KL': loss_KL, 'MSE': sq.mean().detach(),
                'var_latent': var_latent.detach(), 'var_aggr': var_aggr.detach()}


def reference_loop(model, X, Y, Y_mean, num_epochs, batch_size, learning_rate, orders, seed):
    """train_CVAE's optimisation (cvae_regression.py:277-300) on CPU tensors: one Adam over encoder and decoder, MultiStepLR
    stepped per epoch, the batch order by orders(epoch, n), eps of the k-th call the oracle's Philox normals (seed, step k);
    -> {key: [per-epoch weighted means]}"""
    import torch
    from itertools import chain
    X, Y, Y_mean = (torch.as_tensor(np.asarray(a)).to(model.dtype) for a in (X, Y, Y_mean))
    E, n, N = int(num_epochs), len(X), X.shape[-1]
    for m in model.modules():
        m.train()
    optimizer = torch.optim.Adam(chain(*[m.parameters() for m in model.modules()]), lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    log, step = {k: [] for k in KEYS}, 0
    for epoch in range(E):
        order = torch.as_tensor(np.asarray(orders(epoch, n), dtype=np.int64))
        tot = {k: 0.0 for k in KEYS}
        for s in range(0, n, batch_size):
            idx = order[s:s + batch_size]
            eps = torch.as_tensor(normals(seed, step, len(idx), N)).to(model.dtype)
            step += 1
            optimizer.zero_grad()
            losses = model.compute_loss(X[idx], Y[idx], Y_mean[idx], eps)
            losses['loss'].backward()
            optimizer.step()
            for k in KEYS:
                tot[k] += float(losses[k].detach()) * len(idx)
        scheduler.step()
        for k in KEYS:
            log[k].append(tot[k] / n)
    return log
