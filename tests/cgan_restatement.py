"""Test-side restatement of CGANRegression's training statement on plain torch CPU modules, in any dtype, with every random
draw given: the discriminator (reference tools/cnn_tools.py:212-244), the three discriminator losses with the gradient penalty
(models/cgan_regression.py:297-304 and :197-222), the generator loss (:310) and the loop (:247-344).  A plain helper module;
tests/test_gpu_cgan_training.py compares the device against it in float64 and measures its float32 evaluation beside."""
import numpy as np
import torch
from torch import nn

import conv_train_restatement as cr

LAMBDA_DRIFT, LAMBDA_GP = 1e-3, 10          # cgan_regression.py:18-19
KEYS = ('D_loss', 'D_grad', 'D_drift', 'G_loss')


def torch_discriminator(nx, ndf, dtype, state_dict=None):
    """DCGAN_discriminator(6, ndf, nx, bn='None') (cnn_tools.py:224-243); LeakyReLU not in place, which changes no value"""
    D = nn.Sequential(
        nn.Conv2d(6, ndf, 4, 2, 1, bias=False), nn.LeakyReLU(0.2),
        nn.Conv2d(ndf, ndf * 2, 4, 2, 1, bias=False), nn.Identity(), nn.LeakyReLU(0.2),
        nn.Conv2d(ndf * 2, ndf * 4, 4, 2, 1, bias=False), nn.Identity(), nn.LeakyReLU(0.2),
        nn.Conv2d(ndf * 4, ndf * 8, 4, 2, 1, bias=False), nn.Identity(), nn.LeakyReLU(0.2),
        nn.Conv2d(ndf * 8, 1, int(nx / 64 * 4), 1, 0, bias=False)).to(dtype)
    if state_dict is not None:
        D.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in state_dict.items()})
    return D


def gradient_penalty(D, xtrue, ytrue, yfake1, yfake2, epsilon, coin):
    """cgan_regression.py:197-222 with epsilon (B,) and the coin (rand_num) given"""
    B = xtrue.shape[0]
    epsilon = epsilon.reshape(B, 1, 1, 1)
    if coin == 0:                                                                    # :203-206
        ytrue_cat = torch.cat((ytrue, yfake2.detach()), dim=1)
    else:
        ytrue_cat = torch.cat((yfake1.detach(), ytrue), dim=1)
    yfake_cat = torch.cat((yfake1.detach(), yfake2.detach()), dim=1)                 # :207
    yinterp = (epsilon * ytrue_cat + (1 - epsilon) * yfake_cat).detach()             # :209-210
    yinterp.requires_grad = True
    out = D(torch.cat((xtrue, yinterp), dim=1))                                      # :212
    dDdy = torch.autograd.grad(outputs=out, inputs=yinterp, grad_outputs=torch.ones_like(out), retain_graph=True,
                               create_graph=True)[0]                                 # :214-217
    dDdy = dDdy.view(B, -1)
    return LAMBDA_GP * torch.mean((torch.linalg.norm(dDdy, 2, dim=1) - 1) ** 2)      # :221


def critic_losses(D, xtrue, ytrue, yfake1, yfake2, epsilon, coin):
    """cgan_regression.py:297-302"""
    Dtrue1 = D(torch.cat([xtrue, ytrue, yfake2.detach()], dim=1))
    Dtrue2 = D(torch.cat([xtrue, yfake1.detach(), ytrue], dim=1))
    Dfake = D(torch.cat([xtrue, yfake1.detach(), yfake2.detach()], dim=1))
    D_loss = - 0.5 * (Dtrue1.mean() + Dtrue2.mean()) + Dfake.mean()
    D_drift = LAMBDA_DRIFT * (Dtrue1 ** 2).mean()
    D_grad = gradient_penalty(D, xtrue, ytrue, yfake1, yfake2, epsilon, coin)
    return {'D_loss': D_loss, 'D_grad': D_grad, 'D_drift': D_drift}


def leaky_inputs_nearest_to_zero(D, inputs):
    """the smallest |input of a LeakyReLU| relative to the layer's largest, over the given evaluations of D: a gradient is
    compared only where no float32 evaluation can come out on the other side of a kink"""
    nearest = []
    hooks = [m.register_forward_hook(lambda _, inp, out: nearest.append(float(inp[0].detach().abs().min() / inp[0].detach().abs().max())))
             for m in D if isinstance(m, nn.LeakyReLU)]
    with torch.no_grad():
        for a in inputs:
            D(a)
    for h in hooks:
        h.remove()
    return min(nearest)


def reference_loop(G, D, X, Y, Y_mean, regression, num_epochs, batch_size, learning_rate, orders, mixes, noise):
    """train_CGAN (cgan_regression.py:255-325) on CPU tensors of the nets' dtype: orders(epoch, n) in place of the shuffle,
    mixes(epoch, steps, batch_size) -> (epsilon (steps, batch_size), coins (steps,)) in place of gradient_penalty's draws,
    noise(step) -> z (B, 2, N, N) in place of generate's torch.randn, step counting the calls of generate from 0.
    -> {key: [per epoch]}, the batches weighted by their size (AverageLoss)"""
    dtype = next(G.parameters()).dtype
    X, Y = (torch.as_tensor(np.asarray(a)).to(dtype) for a in (X, Y))
    Y_mean = torch.zeros_like(Y) if Y_mean is None else torch.as_tensor(np.asarray(Y_mean)).to(dtype)
    E, n = int(num_epochs), len(X)
    G.train(); D.train()
    optimizerD = torch.optim.Adam(D.parameters(), lr=learning_rate, betas=(0.5, 0.999))                      # :267-272
    optimizerG = torch.optim.Adam(G.parameters(), lr=learning_rate, betas=(0.5, 0.999))
    ms = [int(E / 2), int(E * 3 / 4), int(E * 7 / 8)]
    schedulerD = torch.optim.lr_scheduler.MultiStepLR(optimizerD, milestones=ms, gamma=0.5)
    schedulerG = torch.optim.lr_scheduler.MultiStepLR(optimizerG, milestones=ms, gamma=0.5)
    log = {k: [] for k in KEYS}
    step = 0
    steps = (n + batch_size - 1) // batch_size
    for epoch in range(E):
        order = np.asarray(orders(epoch, n), dtype=np.int64)
        eps, coins = mixes(epoch, steps, batch_size)
        tot, G_loss = np.zeros(4), None
        for i in range(steps):
            idx = torch.as_tensor(order[i * batch_size:(i + 1) * batch_size])
            xtrue, ytrue, ymean = X[idx], Y[idx].clone(), Y_mean[idx]
            if regression == 'residual_loss':                                                                # :286-287
                ytrue -= ymean
            D.zero_grad()
            fakes = []
            for _ in range(2):                                                                               # :290-291
                z = torch.as_tensor(np.asarray(noise(step))).to(dtype)
                step += 1
                fakes.append(G(torch.cat([xtrue, z], dim=1)))
            yfake1, yfake2 = fakes
            if regression == 'full_loss':                                                                    # :293-295
                yfake1 = yfake1 + ymean
                yfake2 = yfake2 + ymean
            losses = critic_losses(D, xtrue, ytrue, yfake1, yfake2, torch.as_tensor(np.asarray(eps[i][:len(idx)])).to(dtype), int(coins[i]))
            (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()                             # :304-306
            optimizerD.step()
            if i % 5 == 0:                                                                                   # :308-313
                G.zero_grad()
                G_loss = - (D(torch.cat([xtrue, yfake1, yfake2], dim=1))).mean()
                G_loss.backward()
                optimizerG.step()
            tot += np.array([float(losses[k].detach()) for k in KEYS[:3]] + [float(G_loss.detach())]) * len(idx)
        schedulerD.step()
        schedulerG.step()
        for j, k in enumerate(KEYS):
            log[k].append(tot[j] / n)
    return log


def generator(hidden, dtype, state_dict):
    """the reference's AndrewCNN(4, 2, hidden_channels=hidden) (tests/conv_train_restatement.py::torch_net)"""
    return cr.torch_net(4, 2, hidden, True, True, dtype, state_dict)
