"""GPU: training of CGANRegression(generator='DeepInversion') on the device — ``train_ops.unet_conv2d`` under autograd,
``TrainableUNet.forward_engine`` (csrc/uconv_train.hip) against the same module's planar ``forward`` on the CPU from the same
state dict, one discriminator and one generator step of ``TrainableUNetCGAN``, ``fit_cgan_unet`` end to end and the command line.

The yardstick is the project's (tests/test_gpu_cgan_training.py): the device may deviate from the float64 CPU evaluation by at
most MARGIN = 8 times what the float32 CPU evaluation of the same statement deviates, per tensor, relative to its largest
magnitude, with a floor of 2^-22.  Bias gradients are scaled by the largest bias gradient of the net (23 biases feed a
train-mode BatchNorm alone: their gradient is zero and its float32 value rounding noise).

Gradients are compared with the LeakyReLU slopes of the device run imposed on both CPU evaluations (the `slopes` hook): the
float64 evaluation of this net has several LeakyReLU inputs within float32's rounding of zero at every shape, one flipped sign
moves a gradient by 1e-3 ... 1e-1 of its largest entry, and no seed avoids it.  With the slopes imposed all three evaluate one
smooth function.  Forward values are continuous in the slopes and need no such care.

Measured on an MI355X (device, float32 torch CPU; relative to the tensor's largest magnitude): see DESIGN.md 3.24."""
import json
import os

import numpy as np
import pytest
import torch

import conv_train_restatement as cr
import uconv_train_restatement as ur
from conftest import golden

pytestmark = pytest.mark.gpu

MARGIN, FLOOR = 8.0, 2.0 ** -22
NDF = 4
CONVS = 39                                   # conv32, 11 units of three, four ConvTranspose2d as 1 x 1 products, conv_end


def _dev():
    return torch.device('cuda', 0)


def _rel(a, truth, scale=None):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    return float(np.abs(a - truth).max() / (np.abs(truth).max() if scale is None else scale))


def _recipe_net(dtype=torch.float32, device='cpu'):
    from pyqg_generative_amd import weights as W
    from pyqg_generative_amd.tools.train_UNet import TrainableUNet
    net = TrainableUNet(seed=0)
    sd = net.state_dict()
    for k, v in W.synthetic_unet().items():
        sd[k] = torch.as_tensor(v)
    for k in sd:
        if k.endswith('num_batches_tracked'):
            sd[k] = torch.tensor(0, dtype=torch.long)
    net.load_state_dict(sd, strict=True)
    return net.to(device=device, dtype=dtype).train()


def _engine(a):
    return torch.as_tensor(cr.to_layout(np.asarray(a, np.float32))).to(_dev())


def _compare(got, r64, r32, what, scale_of=None):
    failures = []
    assert list(got) == list(r64) == list(r32)
    print(f'\n  {what}')
    for k in r64:
        assert np.shape(got[k]) == np.shape(r64[k]), k
        scale = None if scale_of is None else scale_of(k)
        dev, cpu = _rel(got[k], r64[k], scale), _rel(r32[k], r64[k], scale)
        print(f'  {k:34s} device {dev:.2e}   float32 torch CPU {cpu:.2e}   ratio {dev / cpu if cpu else float("inf"):.2f}')
        if not dev <= max(MARGIN * cpu, FLOOR):
            failures.append((k, dev, cpu))
    assert not failures, failures


# ---- unet_conv2d under autograd ------------------------------------------------------------------------------------------------
def test_unet_conv2d_under_autograd():
    """launch counts per call, no data gradient for an input that does not require one, gradients against the float64
    restatement, and a second derivative raises (once_differentiable)"""
    from pyqg_generative_amd.tools import train_ops as T
    cin, cout, k, B, N = 7, 12, 3, 3, 6
    x, w, b, dy = ur.case_data(cin, cout, k, B, N, 11, integer=True)
    xe, wt, bt, g = (torch.as_tensor(a).to(_dev()) for a in (x, w, b, dy))
    count = lambda before: [T.UCONV_LAUNCHES[k] - before[k] for k in ('forward', 'backward_data', 'backward_weight')]
    # the first layer of a net: the input asks for no gradient
    wt.requires_grad_(True); bt.requires_grad_(True)
    before = dict(T.UCONV_LAUNCHES)
    y = T.unet_conv2d(xe, wt, bt)
    assert count(before) == [1, 0, 0]
    y.backward(g)
    assert count(before) == [1, 0, 1] and xe.grad is None
    dw, db = ur.backward_weight(x, dy, cin, cout, k)
    assert np.array_equal(y.detach().cpu().numpy(), ur.forward(x, w, b))
    assert np.array_equal(wt.grad.cpu().numpy(), dw) and np.array_equal(bt.grad.cpu().numpy(), db)
    # an inner layer without a bias: both gradients, db not asked for
    xe.requires_grad_(True)
    before = dict(T.UCONV_LAUNCHES)
    y = T.unet_conv2d(xe, wt)
    y.backward(g)
    assert count(before) == [1, 1, 1]
    assert np.array_equal(y.detach().cpu().numpy(), ur.forward(x, w)) and np.array_equal(xe.grad.cpu().numpy(), ur.backward_data(dy, w))
    # only the data gradient
    before = dict(T.UCONV_LAUNCHES)
    T.unet_conv2d(xe, wt.detach(), bt.detach()).backward(g)
    assert count(before) == [1, 1, 0]
    # differentiable once
    y = T.unet_conv2d(xe, wt, bt)
    gx, = torch.autograd.grad((y * y).sum(), xe, create_graph=True)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        (gx * gx).sum().backward()
    with pytest.raises(ValueError, match='channels'):
        T.unet_conv2d(xe[..., :0], wt)


# ---- forward_engine against forward ------------------------------------------------------------------------------------------
def _buffers(net):
    sd = net.state_dict()
    return {k: sd[k].detach().cpu().double().numpy() for k in sd if k.endswith(('running_mean', 'running_var'))}


def _counters(net):
    sd = net.state_dict()
    return {k: int(sd[k]) for k in sd if k.endswith('num_batches_tracked')}


@pytest.mark.parametrize('case', ['32x2', '48x1'])
def test_forward_engine_is_forward_in_train_mode(case):
    d = golden('unet_train.npz')
    x = d[f'x_{case}']
    ref = {}
    for dtype in (torch.float64, torch.float32):
        net = _recipe_net(dtype)
        with torch.no_grad():
            y = net(torch.as_tensor(x).to(dtype))
        ref[dtype] = dict(_buffers(net), y=y.double().numpy())
        assert set(_counters(net).values()) == {1, 2}
    net = _recipe_net(device=_dev())
    with torch.no_grad():
        out = net.forward_engine(_engine(x))
    assert out.shape == (x.shape[0], x.shape[-1], x.shape[-1], 8) and not bool(out[..., 2:].any())
    got = dict(_buffers(net), y=out[..., :2].permute(0, 3, 1, 2).cpu().double().numpy())
    assert all(v == (2 if k.endswith('.bn.num_batches_tracked') else 1) for k, v in _counters(net).items())
    _compare(got, ref[torch.float64], ref[torch.float32], f'train-mode forward and BatchNorm buffers, {case}')
    # the golden is the reference's own module: the same rule against its float64 output
    y64, y32 = d[f'y64_{case}'], d[f'y32_{case}']
    assert _rel(got['y'], y64) <= max(MARGIN * _rel(y32, y64), FLOOR)


def test_gradients_with_the_device_runs_slopes_imposed():
    from pyqg_generative_amd.tools import train_ops as T
    from pyqg_generative_amd.tools.train_UNet import N_SITES
    d = golden('unet_train.npz')
    x, r = d['x_32x2'], d['r_32x2']
    net = _recipe_net(device=_dev())
    slopes = []
    before = dict(T.UCONV_LAUNCHES)
    y = net.forward_engine(_engine(x), slopes=slopes)
    (y[..., :2] * torch.as_tensor(r).to(_dev()).permute(0, 2, 3, 1)).sum().backward()
    assert [T.UCONV_LAUNCHES[k] - before[k] for k in ('forward', 'backward_data', 'backward_weight')] == [CONVS, CONVS - 1, CONVS]
    assert len(slopes) == N_SITES
    got = {k: p.grad.detach().cpu().double().numpy() for k, p in net.named_parameters()}
    imposed = [s.cpu() for s in slopes]

    def on_cpu(dtype, use):
        m = _recipe_net(dtype)
        own = []
        yy = m(torch.as_tensor(x).to(dtype), slopes=own, use_slopes=use)
        (yy * torch.as_tensor(r).to(dtype)).sum().backward()
        return {k: p.grad.double().numpy() for k, p in m.named_parameters()}, own
    (r64, _), (r32, _) = on_cpu(torch.float64, imposed), on_cpu(torch.float32, imposed)
    # a sanity cap: the device's slopes are the float64 run's own signs but for inputs within rounding of zero
    _, own = on_cpu(torch.float64, None)
    flips = sum(int(((a == 1) != (b == 1)).sum()) for a, b in zip(imposed, own))
    total = sum(a.numel() for a in imposed)
    print(f'\n  {flips} of {total} LeakyReLU slopes of the device run differ from the float64 run\'s own')
    assert flips < 1e-4 * total
    bias_scale = max(np.abs(v).max() for k, v in r64.items() if k.endswith('bias'))
    assert bias_scale > 0 and all(np.abs(v).max() > 0 for k, v in r64.items() if not k.endswith('bias'))
    _compare(got, r64, r32, 'parameter gradients of sum(y r), 32 x 32, 2 members', lambda k: bias_scale if k.endswith('bias') else None)


def test_eval_mode_is_the_device_inference(tmp_path):
    """TrainableUNet.eval().forward_engine against CGANRegression(generator='DeepInversion') reading the same state dict from a
    folder: within 2e-5 of max|y|, the bound the project holds its generator goldens to"""
    from pyqg_generative_amd.models.cgan_regression import CGANRegression
    net = _recipe_net(device=_dev()).eval()
    torch.save({k: v.cpu() for k, v in net.state_dict().items()}, tmp_path / 'G.pt')
    for name in ('x_scale.json', 'y_scale.json'):
        with open(tmp_path / name, 'w') as f:
            json.dump({'mean': str([[[0.0]], [[0.0]]]), 'std': str([[[1.0]], [[1.0]]])}, f)
    model = CGANRegression(folder=str(tmp_path), generator='DeepInversion', regression='None', nx=32)
    x = golden('unet_train.npz')['x_32x2']
    want = model._gen.cnn_forward(torch.as_tensor(x).to(_dev())).cpu().double().numpy()
    with torch.no_grad():
        got = net.forward_engine(_engine(x))[..., :2].permute(0, 3, 1, 2).cpu().double().numpy()
    assert set(_counters(net).values()) == {0}
    print(f'\n  eval-mode forward_engine against the device inference: {_rel(got, want):.2e} of max|y|')
    assert np.abs(want).max() > 0 and _rel(got, want) <= 2e-5


# ---- the GAN's steps -----------------------------------------------------------------------------------------------------------
def _zero_gradient_biases():
    import test_unet_train_cpu as c
    return set(c.zero_gradient_biases())


def test_one_discriminator_step_and_one_generator_step():
    from pyqg_generative_amd.tools.train_CGAN import TrainableUNetCGAN
    from pyqg_generative_amd.tools import train_ops as T
    N, B = 32, 2
    net = TrainableUNetCGAN('None', N, seed=41, ndf=NDF).to(_dev()).train()
    assert net.generator == 'DeepInversion' and set(_counters(net.G).values()) == {0}
    rs = np.random.RandomState(42)
    X, Y = (torch.as_tensor(rs.randn(B, 2, N, N).astype(np.float32)).to(_dev()) for _ in range(2))
    xe, ye = T.gather_batch(X), T.gather_batch(Y)
    optD = torch.optim.Adam(net.D.parameters(), lr=2e-3, betas=(0.5, 0.999))
    optG = torch.optim.Adam(net.G.parameters(), lr=2e-3, betas=(0.5, 0.999))
    count = lambda before: [T.UCONV_LAUNCHES[k] - before[k] for k in ('forward', 'backward_data', 'backward_weight')]
    before = dict(T.UCONV_LAUNCHES)
    f1, f2 = (net.G.forward_engine(T.latent_prior(X, None, net.seed, step)) for step in (0, 1))
    assert count(before) == [2 * CONVS, 0, 0]
    losses = net.critic_losses(xe, ye, f1, f2, torch.as_tensor(rs.rand(B).astype(np.float32)).to(_dev()), 0)
    (losses['D_loss'] + losses['D_grad'] + losses['D_drift']).backward()
    assert count(before) == [2 * CONVS, 0, 0]                      # the fakes are detached: nothing of G runs backward
    optD.step()
    G0 = {k: p.detach().clone() for k, p in net.G.named_parameters()}
    D0 = {k: p.detach().clone() for k, p in net.D.named_parameters()}
    net.G.zero_grad()
    net.D.zero_grad()
    with T.data_gradient_only():
        net.generator_loss(xe, f1, f2).backward()
    assert count(before) == [2 * CONVS, 2 * (CONVS - 1), 2 * CONVS]
    optG.step()
    zero = _zero_gradient_biases()
    still = [k for k, p in net.G.named_parameters() if k not in zero and torch.equal(p.detach(), G0[k])]
    assert not still, still
    assert all(torch.equal(p.detach(), D0[k]) for k, p in net.D.named_parameters())
    assert {v for k, v in _counters(net.G).items() if '.bn.' in k} == {4} and {v for k, v in _counters(net.G).items() if '.conv.2.' in k} == {2}


# ---- fit_cgan_unet end to end -------------------------------------------------------------------------------------------------
FILES = ['D.pt', 'G.pt', 'model_args.json', 'stats.nc', 'x_scale.json', 'y_scale.json']
FIT_N = 32


def _fields(seed):
    """conv_train_restatement.fit_fields at 32 x 32: 2 runs x 6 times of Gaussian q and a fixed circular stencil of it"""
    q = np.random.RandomState(seed).randn(2, 6, 2, FIT_N, FIT_N) * np.array([8e-6, 1e-6]).reshape(1, 1, 2, 1, 1)
    y = np.zeros_like(q)
    for dy in range(3):
        for dx in range(3):
            y += cr.STENCIL[dy, dx] * np.roll(q, (1 - dy, 1 - dx), axis=(-2, -1))
    return q, 1e-6 * y


def _dataset(seed):
    from pyqg_generative_amd.tools import xr_lite
    q, y = _fields(seed)
    dims = ['run', 'time', 'lev', 'y', 'x']
    return xr_lite.Dataset({'q': (dims, q), 'q_forcing_advection': (dims, y)})


@pytest.mark.parametrize('regression', ['None', 'full_loss'])
def test_fit_cgan_unet_end_to_end(tmp_path, regression):
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools.train_CGAN import fit_cgan_unet, KEYS
    from pyqg_generative_amd.tools.simulate import load_parameterization, dataset_backend
    E = 2
    ds_train, ds_test = _dataset(1), _dataset(2)
    mixes = lambda epoch, steps, batch: (np.random.RandomState(7 + epoch).rand(steps, batch).astype(np.float32),
                                         np.random.RandomState(9 + epoch).randint(0, 2, steps))
    fit = dict(regression=regression, nx=FIT_N, num_epochs=E, num_epochs_regression=1, batch_size=4, learning_rate=2e-3, nruns=1, seed=3,
               orders=cr.fixed_orders(50), mixes=mixes, runs=lambda R, k: np.arange(R)[::-1][:k], verbose=False, ndf=NDF)
    folder = str(tmp_path / 'model')
    state = np.random.get_state()
    model = fit_cgan_unet(ds_train, ds_test, folder=folder, **fit)
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))       # every draw came from a hook
    assert isinstance(model, CGANRegression) and model.generator == 'DeepInversion'
    assert sorted(os.listdir(folder)) == sorted(FILES + (['net_mean.pt'] if regression != 'None' else []))
    assert json.load(open(os.path.join(folder, 'model_args.json'))) == dict(
        model='CGANRegression', regression=regression, nx=FIT_N, generator='DeepInversion', div=False,
        hidden_channels=[128, 64, 32, 32, 32, 32, 32])
    loaded = load_parameterization(folder).param
    assert isinstance(loaded, CGANRegression) and loaded.generator == 'DeepInversion'

    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    val = lambda k: np.asarray(stats[k].values)
    for k in list(KEYS) + ['L2_mean', 'L2_total', 'L2_residual', 'L2_mean_test', 'L2_total_test', 'L2_residual_test', 'loss']:
        assert val(k).shape == (E,) and np.isfinite(val(k)).all(), k
    assert val('var_ratio').shape == (E, 2) and np.isfinite(val('var_ratio')).all()
    assert 1 <= int(val('Epoch_opt')) <= E

    pred = model.predict(ds_test, M=2)
    for k in ('q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var'):
        v = np.asarray(pred[k].values)
        assert v.shape == (2, 6, 2, FIT_N, FIT_N) and np.isfinite(v).all(), k
    assert np.abs(np.asarray(pred['q_forcing_advection'].values)).max() > 0

    # G.pt is the reference's state dict: it loads into the test-side twin, strictly, and is what the trained net holds
    sd = torch.load(os.path.join(folder, 'G.pt'), map_location='cpu', weights_only=True)
    twin = ur.torch_twin()
    twin.load_state_dict(sd, strict=True)
    assert all(torch.equal(sd[k], v.detach().cpu()) for k, v in model.trained_G.state_dict().items())
    # 3 batches x 2 forwards x 2 epochs in train mode; the scoring between them runs in eval mode
    assert int(sd['res512.bn.num_batches_tracked']) == 2 * 12 and int(sd['res512.conv.2.num_batches_tracked']) == 12

    if regression == 'None':                     # the same hooks and seed: the same bits
        again = str(tmp_path / 'again')
        fit_cgan_unet(ds_train, ds_test, folder=again, **fit)
        sd2 = torch.load(os.path.join(again, 'G.pt'), map_location='cpu', weights_only=True)
        differ = [k for k in sd if not torch.equal(sd[k], sd2[k])]
        assert not differ, differ[:5]


def test_command_line_trains_a_unet_folder(tmp_path):
    """python -m pyqg_generative_amd.tools.train_CGAN --model CGANRegression-Unet, in process"""
    from pyqg_generative_amd.models import CGANRegression
    from pyqg_generative_amd.tools import train_CGAN, xr_lite
    dims = ['run', 'time', 'lev', 'y', 'x']
    for name, seed in (('train', 1), ('val', 2)):
        q, y = _fields(seed)
        for r in range(len(q)):
            xr_lite.Dataset({'q': (dims, q[r:r + 1]), 'q_forcing_advection': (dims, y[r:r + 1])},
                            coords={'time': (('time',), np.arange(q.shape[1], dtype='float32') * 1000.)}).to_netcdf(str(tmp_path / f'{name}_{r}.nc'))
    folder = str(tmp_path / 'model')
    state = np.random.get_state()
    try:
        model = train_CGAN.main(['--model', 'CGANRegression-Unet', '--train', str(tmp_path / 'train_*.nc'), '--validate', str(tmp_path / 'val_*.nc'),
                                 '--model_args', repr({'folder': folder, 'nx': FIT_N}),
                                 '--fit_args', repr({'num_epochs': 1, 'batch_size': 4, 'nruns': 1, 'verbose': False, 'ndf': NDF})])
    finally:
        np.random.set_state(state)
    assert isinstance(model, CGANRegression) and model.generator == 'DeepInversion'
    assert sorted(os.listdir(folder)) == sorted(FILES)
    assert json.load(open(os.path.join(folder, 'model_args.json')))['generator'] == 'DeepInversion'
