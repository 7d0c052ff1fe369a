"""CPU: TrainableUNet (tools/train_UNet.py), the trainable DeepInversion U-Net generator, against tests/golden/unet_train.npz —
the reference's own DeepInversionGenerator in TRAIN mode on the recipe weights (tests/golden/make_golden_unet_train.py): the
planar forward in float64 reproduces the reference's output, every parameter gradient of the loss sum(y r) and every BatchNorm
buffer to 1e-9 of each tensor's largest (float32 through this net deviates up to ~3000 x 2^-24, so float64 deviates ~3e-13; a
wiring error is O(1)); its float32 forward is within the project's MARGIN of the reference's float32; the state dict has the
reference's keys, shapes and order; the seeded initialisation; the slopes hook.

Bias gradients are scaled by the largest bias gradient of the net: 23 biases feed a train-mode BatchNorm alone and have an
exactly zero gradient (1e-17 in float64), so a ratio to their own magnitude means nothing."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from conftest import golden

MARGIN, FLOOR = 8.0, 2.0 ** -22
TOL = 1e-9
CASES = {'32x2': (32, 2), '48x1': (48, 1)}          # what make_golden_unet_train.py evaluates: name -> (N, members)


def sample_index(n):
    """make_golden_unet_train.py's strided sample: at most 64 indices of a flat tensor of n elements"""
    return np.linspace(0, n - 1, min(n, 64)).astype(np.int64)


@pytest.fixture(scope='module')
def gold():
    return golden('unet_train.npz')


def _net(dtype=torch.float64):
    """TrainableUNet with the recipe weights, counters zero, train mode"""
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
    return net.to(dtype).train()


ZERO_GRAD_BIASES = 23


def zero_gradient_biases():
    """the biases whose every consumer is a train-mode BatchNorm: conv.1.bias of the nine BatchNorm units; conv.4.bias and
    conv1.bias of res32_start and down64 ... down512 (pooled or not, their sum feeds the next unit's bn); the four
    upsampling.bias (concatenated into a unit's bn)"""
    bn_units = ['down64.conv.1', 'down128.conv.1', 'down256.conv.1', 'down512.conv.1', 'res512', 'up512.conv', 'up256.conv',
                'up128.conv', 'up64.conv']
    out = [u + '.conv.1.bias' for u in bn_units]
    for u in ['res32_start'] + bn_units[:4]:
        out += [u + '.conv.4.bias', u + '.conv1.bias']
    return out + [f'up{c}.upsampling.bias' for c in (512, 256, 128, 64)]


def test_state_dict_has_the_references_keys_shapes_and_order(gold):
    from pyqg_generative_amd import weights as W
    net = _net()
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in gold['keys']]
    assert [','.join(str(s) for s in sd[k].shape) for k in sd] == [str(s) for s in gold['shapes']]
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in gold['params']]
    shapes = W.unet_shapes()
    assert {k for k in sd if not k.endswith('num_batches_tracked')} == set(shapes)
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    assert sum(k.endswith('num_batches_tracked') for k in sd) == 18
    assert str(gold['weights_checksum']) == W.unet_checksum(W.synthetic_unet())
    zero = zero_gradient_biases()
    assert len(zero) == len(set(zero)) == ZERO_GRAD_BIASES and set(zero) <= set(sd)


@pytest.mark.parametrize('case', list(CASES))
def test_float64_forward_reproduces_the_reference_in_train_mode(gold, case):
    N, B = CASES[case]
    net = _net()
    x = torch.tensor(gold[f'x_{case}'], dtype=torch.float64)
    r = torch.tensor(gold[f'r_{case}'], dtype=torch.float64)
    y = net(x)
    (y * r).sum().backward()
    want = gold[f'y64_{case}']
    assert y.shape == (B, 2, N, N)
    assert np.abs(y.detach().numpy() - want).max() <= TOL * np.abs(want).max()
    # every BatchNorm buffer after the forward, counters included: 2 for a unit's bn, 1 for its conv.2
    sd = net.state_dict()
    params = [str(k) for k in gold['params']]
    buffers = [k for k in sd if k not in params]
    got = np.concatenate([sd[k].double().reshape(-1).numpy() for k in buffers])
    want, at = gold[f'buf_{case}'], 0
    assert got.shape == want.shape
    for k in buffers:
        n = sd[k].numel()
        g, w = got[at:at + n], want[at:at + n]
        at += n
        if k.endswith('num_batches_tracked'):
            assert g[0] == w[0] == (2 if k.endswith('.bn.num_batches_tracked') else 1), k
        else:
            assert np.abs(g - w).max() <= TOL * np.abs(w).max(), k
    # the gradients: sum, sum of magnitudes, largest, and the strided sample
    grads = {k: p.grad.numpy().reshape(-1) for k, p in net.named_parameters()}
    stat, samp = gold[f'gstat_{case}'], gold[f'gsample_{case}']
    bias_scale = max(stat[i, 2] for i, k in enumerate(params) if k.endswith('bias'))
    zero = set(zero_gradient_biases())
    worst = 0.0
    for i, k in enumerate(params):
        g = grads[k]
        scale = bias_scale if k.endswith('bias') else stat[i, 2]
        assert scale > 0
        idx = sample_index(g.size)
        dev = max(abs(g.sum() - stat[i, 0]) / g.size, abs(np.abs(g).sum() - stat[i, 1]) / g.size, abs(np.abs(g).max() - stat[i, 2]),
                  np.abs(g[idx] - samp[i, :len(idx)]).max()) / scale
        worst = max(worst, dev)
        assert dev <= TOL, (k, dev)
        if k in zero:
            assert stat[i, 2] <= 1e-12 * bias_scale and np.abs(g).max() <= 1e-12 * bias_scale, k
        elif k.endswith('bias'):
            assert stat[i, 2] > 1e-6 * bias_scale, k
    print(f'\n  {case}: worst gradient deviation {worst:.2e} of the tensor\'s (the biases\') largest')


def test_counters_after_two_forwards_read_four_and_two(gold):
    net = _net()
    x = torch.tensor(gold['x_32x2'], dtype=torch.float64)
    with torch.no_grad():
        net(x)
        net(x)
    sd = net.state_dict()
    counters = [k for k in sd if k.endswith('num_batches_tracked')]
    assert [int(sd[k]) for k in counters] == [int(v) for v in gold['counters_after_two']]
    assert {int(sd[k]) for k in counters if '.bn.' in k} == {4} and {int(sd[k]) for k in counters if '.conv.2.' in k} == {2}
    net.eval()
    with torch.no_grad():
        net(x)
    assert [int(net.state_dict()[k]) for k in counters] == [int(v) for v in gold['counters_after_two']]      # eval: no update


def test_two_forwards_precede_one_backward(gold):
    """a GAN's generator step: both fakes are generated before G_loss runs backward, so the second forward's update of the
    running statistics must not invalidate what the first one's graph keeps"""
    net = _net(torch.float32)
    x = torch.tensor(gold['x_48x1'])
    y1 = net(x)
    y2 = net(x.flip(-1))
    (y1 * y2).sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert int(net.state_dict()['res512.bn.num_batches_tracked']) == 4


@pytest.mark.parametrize('case', list(CASES))
def test_float32_forward_is_within_the_margin_of_the_references_float32(gold, case):
    net = _net(torch.float32)
    with torch.no_grad():
        y = net(torch.tensor(gold[f'x_{case}'])).numpy().astype(np.float64)
    y64, y32 = gold[f'y64_{case}'], gold[f'y32_{case}'].astype(np.float64)
    scale = np.abs(y64).max()
    dev, ref = np.abs(y - y64).max() / scale, np.abs(y32 - y64).max() / scale
    print(f'\n  {case}: float32 forward {dev:.2e}, the reference\'s float32 {ref:.2e} of the largest output')
    assert dev <= max(MARGIN * ref, FLOOR)
    sd = net.state_dict()
    buffers = [k for k in sd if k not in {str(p) for p in gold['params']}]
    got = np.concatenate([sd[k].double().reshape(-1).numpy() for k in buffers])
    b64, b32, at = gold[f'buf_{case}'], gold[f'buf32_{case}'], 0
    for k in buffers:
        n = sd[k].numel()
        g, w, f = got[at:at + n], b64[at:at + n], b32[at:at + n]
        at += n
        s = np.abs(w).max()
        assert np.abs(g - w).max() / s <= max(MARGIN * np.abs(f - w).max() / s, FLOOR), k


def test_seeded_initialisation():
    """N(0, 0.02) for every Conv2d AND ConvTranspose2d weight, N(1, 0.02) / 0 for BatchNorm; the same for the same seed,
    another for another, and independent of the global torch stream, which it leaves alone"""
    from torch import nn
    from pyqg_generative_amd.tools.train_UNet import TrainableUNet
    torch.manual_seed(123)
    state = torch.random.get_rng_state()
    a = TrainableUNet(seed=5)
    assert torch.equal(state, torch.random.get_rng_state())
    torch.manual_seed(456)
    b, c = TrainableUNet(seed=5), TrainableUNet(seed=6)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert not torch.equal(sa['res512.conv.1.weight'], sc['res512.conv.1.weight'])
    kinds = {nn.Conv2d: 0, nn.ConvTranspose2d: 0, nn.BatchNorm2d: 0}
    for name, m in a.named_modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            kinds[type(m)] += 1
            w = m.weight.detach().double()
            assert float(w.abs().max()) < 0.02 * 6.5, name                          # no default (uniform 1 / sqrt(fan_in)) draw
            if w.numel() >= 2 ** 14:                                                # the sample moments of the large tensors
                n = w.numel()
                assert abs(float(w.mean())) < 5 * 0.02 / n ** 0.5 and abs(float(w.std()) / 0.02 - 1) < 5 / (2 * n) ** 0.5, name
        elif isinstance(m, nn.BatchNorm2d):
            kinds[type(m)] += 1
            w = m.weight.detach().double()
            assert not m.bias.detach().any() and float((w - 1).abs().max()) < 0.02 * 5, name
            assert not m.running_mean.any() and bool((m.running_var == 1).all()) and int(m.num_batches_tracked) == 0
            if w.numel() >= 256:
                assert abs(float(w.mean()) - 1) < 5 * 0.02 / w.numel() ** 0.5 and abs(float(w.std()) / 0.02 - 1) < 5 / (2 * w.numel()) ** 0.5, name
    assert kinds == {nn.Conv2d: 35, nn.ConvTranspose2d: 4, nn.BatchNorm2d: 18}


def test_recorded_slopes_fed_back_reproduce_the_output_bit_for_bit(gold):
    from pyqg_generative_amd.tools.train_UNet import N_SITES
    x = torch.tensor(gold['x_32x2'])
    slopes = []
    with torch.no_grad():
        y = _net(torch.float32)(x, slopes=slopes)
        again = _net(torch.float32)(x, use_slopes=slopes)
        assert len(slopes) == N_SITES and all(set(np.unique(s.numpy())) <= {np.float32(0.2), np.float32(1.0)} for s in slopes)
        assert torch.equal(y, again)
        # imposed slopes are used, not the sign: all ones make the net another function
        other = _net(torch.float32)(x, use_slopes=[torch.ones_like(s) for s in slopes])
        assert not torch.equal(y, other)
        with pytest.raises(ValueError, match='use_slopes'):
            _net(torch.float32)(x, use_slopes=slopes[:-1])
        with pytest.raises(ValueError, match='use_slopes'):
            _net(torch.float32)(x, use_slopes=[slopes[1]] + slopes[1:-1] + [slopes[0][:, :1]])


def test_the_twin_of_the_restatement_loads_the_state_dict_and_agrees_in_eval_mode(gold):
    import uconv_train_restatement as ur
    net = _net(torch.float32)
    twin = ur.torch_twin()
    twin.load_state_dict(net.state_dict(), strict=True)
    x = torch.tensor(gold['x_48x1'])
    with torch.no_grad():
        want, got = twin(x), net.eval()(x)
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
