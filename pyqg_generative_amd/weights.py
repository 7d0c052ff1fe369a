"""Loading generator weights into the layout the C ABI takes (qgx_cnn_weights).

Sources: the reference's on-disk model folders (``*.pt`` state dicts +
``x_scale.json``/``y_scale.json``, written by pyqg_generative/tools/cnn_tools.py:543-553
and models/*.save_model) or this repo's flat ``.npz`` fixtures.
"""
import json
import os
import numpy as np


class ArchitectureMismatch(ValueError, NotImplementedError):
    """A model folder whose state dict is not the one the constructor's arguments describe (other widths, flags or form).  It is a
    ValueError — the arguments are wrong for this folder, which is what the loaders have always raised — and a
    NotImplementedError: the model classes raise that for every configuration that does not run, and there is no conversion of a
    net trained with one architecture into another, so callers that catch either see it."""


class UntrainedFolder(NotImplementedError):
    """A model folder without the trained files of its class.  The reference builds an untrained model there, to be fitted; there
    is no training on the device."""


def net_from_state_dict(sd):
    """AndrewCNN state_dict (keys conv.{3i}.weight/bias, conv.{3i+2}.* BatchNorm) -> dict."""
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], 'detach') else sd[k],
                               dtype=np.float32)
    net = dict(conv_w=[], conv_b=[], bn_g=[], bn_b=[], bn_m=[], bn_v=[])
    for i in range(8):
        net['conv_w'].append(get(f'conv.{3 * i}.weight'))
        net['conv_b'].append(get(f'conv.{3 * i}.bias'))
        if i < 7:
            net['bn_g'].append(get(f'conv.{3 * i + 2}.weight'))
            net['bn_b'].append(get(f'conv.{3 * i + 2}.bias'))
            net['bn_m'].append(get(f'conv.{3 * i + 2}.running_mean'))
            net['bn_v'].append(get(f'conv.{3 * i + 2}.running_var'))
    return net


def is_flux_form(net):
    """an AndrewCNN dict whose last convolution writes four channels: AndrewCNN(n_in, 2, div=True) (cnn_tools.py:139-142), the
    x-fluxes of both layers, then the y-fluxes; its forward is 10000 * divergence(fluxes) (:170-175)"""
    return int(np.shape(net['conv_w'][-1])[0]) == 4


def check_flux_form(net, div, name='net'):
    """ValueError unless the last layer of the AndrewCNN dict is (4, 32, 3, 3) with div, (2, 32, 3, 3) without: a state dict
    trained in one form must not be evaluated in the other (the shapes differ, so the reference's load_state_dict refuses
    it too)"""
    want = (4 if div else 2, 32, 3, 3)
    got = tuple(np.shape(net['conv_w'][7]))
    if got != want or tuple(np.shape(net['conv_b'][7])) != want[:1]:
        raise ArchitectureMismatch(f'{name}: last convolution {got}, but div={bool(div)} takes {want} '
                                   f'({"four flux channels" if div else "two output channels"}): the state dict is that of a '
                                   f'model trained with div={not bool(div)}')


SHIPPED_HIDDEN = [128, 64, 32, 32, 32, 32, 32]
KERNELS = [5, 5, 3, 3, 3, 3, 3, 3]           # AndrewCNN's default `kernels` (cnn_tools.py:131): the only ones a model class passes


def check_hidden_channels(hidden_channels):
    """-> list of ints; ValueError unless it is 1 ... 7 widths of 1 ... 256 (what the device engine admits: the reference's
    default kernels list has eight entries, so AndrewCNN itself takes at most seven hidden layers)"""
    hidden = [int(h) for h in hidden_channels]
    if not 1 <= len(hidden) <= 7 or any(h != v for h, v in zip(hidden, hidden_channels)):
        raise ValueError(f'hidden_channels={list(hidden_channels)!r}: expected 1 ... 7 integer widths')
    if any(not 1 <= h <= 256 for h in hidden):
        raise ValueError(f'hidden_channels={hidden!r}: every width must be 1 ... 256')
    return hidden


def arch_kernels(hidden_channels):
    """kernel size of each of the len(hidden_channels) + 1 convolutions (cnn_tools.py:146-158)"""
    n = len(hidden_channels)
    return KERNELS[:n] + [KERNELS[-1]]


def arch_shapes(n_in, hidden_channels, batch_norm=True, bias=True, div=False, n_out=2):
    """every parameter / buffer of AndrewCNN(n_in, n_out, batch_norm=, bias=, div=, hidden_channels=)'s state dict -> shape
    (num_batches_tracked left out).  Blocks are Conv2d -> ReLU [-> BatchNorm2d] in one nn.Sequential `conv`, so convolution l
    sits at index 3 l with BatchNorm (its BatchNorm at 3 l + 2) and at 2 l without; the last block is the convolution alone."""
    hidden = check_hidden_channels(hidden_channels)
    ch = [int(n_in)] + hidden + [2 * n_out if div else n_out]
    ks = arch_kernels(hidden)
    step = 3 if batch_norm else 2
    s = {}
    for l in range(len(ch) - 1):
        s[f'conv.{step * l}.weight'] = (ch[l + 1], ch[l], ks[l], ks[l])
        if bias:
            s[f'conv.{step * l}.bias'] = (ch[l + 1],)
        if batch_norm and l < len(ch) - 2:
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                s[f'conv.{step * l + 2}.{k}'] = (ch[l + 1],)
    return s


def net_from_state_dict_arch(sd, n_in, hidden_channels=SHIPPED_HIDDEN, batch_norm=True, bias=True, div=False, name='net'):
    """AndrewCNN(n_in, 2, batch_norm=, bias=, div=, hidden_channels=) state dict -> dict(conv_w, conv_b, bn_g, bn_b, bn_m,
    bn_v, arch): conv_b is empty without bias, the bn_* lists without BatchNorm.  Every key and shape is checked against the
    constructor's arguments — a state dict trained with other widths, flags or form (div) raises ValueError naming the key,
    as the reference's load_state_dict would refuse it."""
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], 'detach') else sd[k], dtype=np.float32)
    hidden = check_hidden_channels(hidden_channels)
    want = arch_shapes(n_in, hidden, batch_norm, bias, div)
    have = {k for k in sd.keys() if not k.endswith('num_batches_tracked')}
    what = f'AndrewCNN({n_in}, 2, batch_norm={bool(batch_norm)}, bias={bool(bias)}, div={bool(div)}, hidden_channels={hidden})'
    for k in want:
        if k not in have:
            raise ArchitectureMismatch(f'{name}: key {k!r} is missing: not a state dict of {what}')
    for k in sorted(have):
        if k not in want:
            raise ArchitectureMismatch(f'{name}: unexpected key {k!r}: not a state dict of {what}')
    for k, shape in want.items():
        if tuple(get(k).shape) != shape:
            raise ArchitectureMismatch(f'{name}: {k} has shape {tuple(get(k).shape)}, {what} has {shape}')
    step = 3 if batch_norm else 2
    n = len(hidden) + 1
    net = dict(conv_w=[get(f'conv.{step * l}.weight') for l in range(n)],
               conv_b=[get(f'conv.{step * l}.bias') for l in range(n)] if bias else [],
               bn_g=[], bn_b=[], bn_m=[], bn_v=[],
               arch=dict(n_in=int(n_in), hidden_channels=hidden, batch_norm=bool(batch_norm), bias=bool(bias), div=bool(div)))
    if batch_norm:
        for l in range(n - 1):
            net['bn_g'].append(get(f'conv.{step * l + 2}.weight'))
            net['bn_b'].append(get(f'conv.{step * l + 2}.bias'))
            net['bn_m'].append(get(f'conv.{step * l + 2}.running_mean'))
            net['bn_v'].append(get(f'conv.{step * l + 2}.running_var'))
    return net


def net_arch(net):
    """the architecture of an AndrewCNN dict: its 'arch' entry, or — the dicts of net_from_state_dict / net_from_npz /
    synthetic, which carry none — read off the arrays (BatchNorm and bias present)"""
    if 'arch' in net:
        return net['arch']
    w = net['conv_w']
    return dict(n_in=int(np.shape(w[0])[1]), hidden_channels=[int(np.shape(a)[0]) for a in w[:-1]],
                batch_norm=len(net.get('bn_g', ())) > 0, bias=len(net.get('conv_b', ())) > 0, div=int(np.shape(w[-1])[0]) == 4)


def is_shipped_arch(net):
    """whether the dict is the architecture qgx_generator_create takes: the default widths with BatchNorm and bias"""
    a = net_arch(net)
    return list(a['hidden_channels']) == SHIPPED_HIDDEN and bool(a['batch_norm']) and bool(a['bias'])


def state_dict_from_net(net):
    """the inverse of net_from_state_dict_arch (numpy arrays under the reference's keys): fixtures and temporary model
    folders of the tests are written from synthetic_arch nets with it"""
    a = net_arch(net)
    step = 3 if a['batch_norm'] else 2
    sd = {}
    for l, w in enumerate(net['conv_w']):
        sd[f'conv.{step * l}.weight'] = np.asarray(w, np.float32)
        if a['bias']:
            sd[f'conv.{step * l}.bias'] = np.asarray(net['conv_b'][l], np.float32)
        if a['batch_norm'] and l < len(net['conv_w']) - 1:
            for k, key in (('weight', 'bn_g'), ('bias', 'bn_b'), ('running_mean', 'bn_m'), ('running_var', 'bn_v')):
                sd[f'conv.{step * l + 2}.{k}'] = np.asarray(net[key][l], np.float32)
    return sd


def synthetic_arch(n_in, hidden_channels, batch_norm=True, bias=True, div=False, seed=0):
    """Seeded weights of AndrewCNN(n_in, 2, batch_norm=, bias=, div=, hidden_channels=) from the legacy RandomState stream,
    He-scaled like `synthetic` (conv weight, bias, BatchNorm weight, bias, running mean, running var per block, in that
    order): fixtures store net_checksum instead of weights."""
    hidden = check_hidden_channels(hidden_channels)
    rs = np.random.RandomState(seed)
    ch = [int(n_in)] + hidden + [4 if div else 2]
    ks = arch_kernels(hidden)
    n = len(ch) - 1
    net = dict(conv_w=[], conv_b=[], bn_g=[], bn_b=[], bn_m=[], bn_v=[],
               arch=dict(n_in=int(n_in), hidden_channels=hidden, batch_norm=bool(batch_norm), bias=bool(bias), div=bool(div)))
    for i in range(n):
        cin, cout, k = ch[i], ch[i + 1], ks[i]
        net['conv_w'].append((rs.randn(cout, cin, k, k) * np.sqrt(2.0 / (cin * k * k))).astype('float32'))
        if bias:
            net['conv_b'].append((0.1 * rs.randn(cout)).astype('float32'))
        if batch_norm and i < n - 1:
            net['bn_g'].append((1 + 0.1 * rs.randn(cout)).astype('float32'))
            net['bn_b'].append((0.1 * rs.randn(cout)).astype('float32'))
            net['bn_m'].append((0.5 + 0.1 * rs.randn(cout)).astype('float32'))
            net['bn_v'].append((0.5 + 0.2 * rs.rand(cout)).astype('float32'))
    return net


def net_from_npz(d, prefix):
    return dict(conv_w=[np.asarray(d[f'{prefix}w{i}'], np.float32) for i in range(8)],
                conv_b=[np.asarray(d[f'{prefix}b{i}'], np.float32) for i in range(8)],
                bn_g=[np.asarray(d[f'{prefix}g{i}'], np.float32) for i in range(7)],
                bn_b=[np.asarray(d[f'{prefix}be{i}'], np.float32) for i in range(7)],
                bn_m=[np.asarray(d[f'{prefix}m{i}'], np.float32) for i in range(7)],
                bn_v=[np.asarray(d[f'{prefix}v{i}'], np.float32) for i in range(7)])


def load_npz(path, kind, regression_npz=None):
    """-> (nets, x_std, y_std) from a flat fixture written by tests/golden/make_golden.py.  regression_npz: 'gan' / 'vae'
    with a regression net (regression != 'None'), read from net0_ of that second fixture."""
    d = np.load(path, allow_pickle=False)
    nets = [net_from_npz(d, 'net0_')]
    if kind == 'gz':
        nets.append(net_from_npz(d, 'net1_'))
    elif regression_npz is not None:
        nets.append(net_from_npz(np.load(regression_npz, allow_pickle=False), 'net0_'))
    return nets, np.asarray(d['x_std'], np.float32), np.asarray(d['y_std'], np.float32)


def read_scaler_std(path):
    """ChannelwiseScaler.read (cnn_tools.py:547-553): JSON of stringified nested lists."""
    import ast
    with open(path) as f:
        d = json.load(f)
    return np.array(ast.literal_eval(d['std'])).astype('float32').reshape(-1)


ANN_DEFAULTS = dict(stencil_size=3, hidden_channels=[24, 24], scale_invariant=False)   # ANNModel's (ann_model.py:18)


def ann_from_state_dict(sd, stencil_size=3, hidden_channels=(24, 24), scale_invariant=False):
    """ANN state_dict (cnn_tools.py:184-210: keys layers.{2l}.weight (out, in) / layers.{2l}.bias, l = 0 .. len(hidden)) ->
    dict(stencil_size, hidden, scale_invariant, w, b), float32.  The shapes must be those of ANN(s*s, 1, hidden_channels):
    anything else raises ValueError."""
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], 'detach') else sd[k], dtype=np.float32)
    s, hidden = int(stencil_size), [int(h) for h in hidden_channels]
    widths = [s * s] + hidden + [1]
    want = {}
    for l in range(len(widths) - 1):
        want[f'layers.{2 * l}.weight'] = (widths[l + 1], widths[l])
        want[f'layers.{2 * l}.bias'] = (widths[l + 1],)
    if set(sd) != set(want):
        raise ValueError(f'ANN state dict keys {sorted(sd)} are not those of ANN({s * s}, 1, {hidden}): {sorted(want)}')
    for k, shape in want.items():
        if tuple(get(k).shape) != shape:
            raise ValueError(f'{k}: shape {tuple(get(k).shape)}, ANN({s * s}, 1, {hidden}) has {shape}')
    n = len(widths) - 1
    return dict(stencil_size=s, hidden=hidden, scale_invariant=bool(scale_invariant),
                w=[get(f'layers.{2 * l}.weight') for l in range(n)], b=[get(f'layers.{2 * l}.bias') for l in range(n)])


def is_ann_state_dict(sd):
    return 'layers.0.weight' in sd


def read_ann_scale(folder):
    """scale.json of an ANNModel folder (ann_model.py:61-62, 71-75) -> (x_scale, y_scale) as Python floats"""
    with open(os.path.join(folder, 'scale.json')) as f:
        d = json.load(f)
    return float(d['x_scale']), float(d['y_scale'])


def load_ann_folder(folder, stencil_size=None, hidden_channels=None, scale_invariant=None):
    """ANNModel folder -> ([net], x_scale, y_scale): net.pt, scale.json, and the architecture from the arguments, else from
    model_args.json (save_model_args, cnn_tools.py:21-25), else ANNModel's defaults"""
    import torch
    args = dict(ANN_DEFAULTS)
    path = os.path.join(folder, 'model_args.json')
    if os.path.exists(path):
        with open(path) as f:
            args.update({k: v for k, v in json.load(f).items() if k in ANN_DEFAULTS})
    for k, v in (('stencil_size', stencil_size), ('hidden_channels', hidden_channels), ('scale_invariant', scale_invariant)):
        if v is not None:
            args[k] = v
    sd = torch.load(os.path.join(folder, 'net.pt'), map_location='cpu', weights_only=True)
    xs, ys = read_ann_scale(folder)
    return [ann_from_state_dict(sd, **args)], xs, ys


def synthetic_ann(stencil_size=3, hidden_channels=(24, 24), scale_invariant=False, seed=0):
    """Seeded ANN weights with nn.Linear's initialisation range U(-1/sqrt(in), 1/sqrt(in))."""
    rs = np.random.RandomState(seed)
    widths = [stencil_size * stencil_size] + list(hidden_channels) + [1]
    w, b = [], []
    for l in range(len(widths) - 1):
        k = 1.0 / np.sqrt(widths[l])
        w.append(rs.uniform(-k, k, (widths[l + 1], widths[l])).astype(np.float32))
        b.append(rs.uniform(-k, k, widths[l + 1]).astype(np.float32))
    return dict(stencil_size=int(stencil_size), hidden=[int(h) for h in hidden_channels],
                scale_invariant=bool(scale_invariant), w=w, b=b)


def load_folder(folder, kind, regression=False, generator='Andrew', div=False, hidden_channels=None, batch_norm=True, bias=True):
    """Reference model folder -> (nets, x_std, y_std).  kind: 'gan' | 'vae' | 'gz' | 'ols' (OLSModel: net.pt,
    ols_model.py:59-66) | 'ann' (ANNModel: net.pt, scale.json, ann_model.py:68-77 — see load_ann_folder; x_std, y_std are
    the scalars x_scale, y_scale); regression ('gan' / 'vae' trained with
    regression != 'None'): the folder also holds net_mean.pt (cgan_regression.py:98-101, cvae_regression.py:75-76).
    generator='DeepInversion' (CGAN only, cgan_regression.py:50-53): G.pt is the U-Net, nets[0] its unet_from_state_dict.
    div: the model's `div` flag (model_args.json) — every AndrewCNN of the folder must then be in flux form (a (4, 32, 3, 3)
    last layer), and none without it; a contradiction raises ValueError.
    hidden_channels / batch_norm / bias: the architecture arguments the model was constructed with (model_args.json).  As in
    the reference they reach OLSModel's net (all three), the generator / decoder of a GAN / VAE and both nets of a GZ model
    (hidden_channels); a GAN's / VAE's net_mean always has the default widths (cgan_regression.py:60, cvae_regression.py:50).
    With any of them off the defaults the state dicts go through net_from_state_dict_arch, which checks every key and shape."""
    import torch
    hidden = SHIPPED_HIDDEN if hidden_channels is None else check_hidden_channels(hidden_channels)
    generic = hidden != SHIPPED_HIDDEN or not batch_norm or not bias
    if generator not in ('Andrew', 'DeepInversion') or (generator == 'DeepInversion' and kind != 'gan'):
        raise ValueError(f'generator={generator!r} is not available for kind {kind!r}')
    if kind == 'ann':
        return load_ann_folder(folder)
    files = {'gan': ['G.pt'], 'vae': ['decoder.pt'], 'gz': ['net_mean.pt', 'net_var.pt'], 'ols': ['net.pt']}[kind]
    if regression and kind in ('gan', 'vae'):
        files = files + ['net_mean.pt']
    nets = []
    for f in files:
        if not os.path.exists(os.path.join(folder, f)):
            raise UntrainedFolder(f'{os.path.join(folder, f)} is missing: the reference builds an untrained model there, to be fitted, '
                                  'and there is no training on the device.  Only trained folders load, with the arguments they were '
                                  "trained with (model_args.json; the reference's defaults: div=False, batch_norm=True, bias=True, "
                                  f'hidden_channels={SHIPPED_HIDDEN})')
    for i, f in enumerate(files):
        sd = torch.load(os.path.join(folder, f), map_location='cpu', weights_only=True)
        if generator == 'DeepInversion' and i == 0:
            nets.append(unet_from_state_dict(sd))
        elif generic and not (kind in ('gan', 'vae') and i == 1):
            nets.append(net_from_state_dict_arch(sd, 4 if kind in ('gan', 'vae') else 2, hidden, batch_norm, bias, div, name=f))
        else:
            nets.append(net_from_state_dict(sd))
            check_flux_form(nets[-1], div, f)
    return nets, read_scaler_std(os.path.join(folder, 'x_scale.json')), \
        read_scaler_std(os.path.join(folder, 'y_scale.json'))


def synthetic(kind, seed=0, regression=False, div=False):
    """Seeded random weights of the architecture (throughput runs without fixtures).  div: flux-form nets, AndrewCNN(div=True)
    — a four-channel last layer; layers 1-7 are those of div=False with the same seed (for one net)."""
    if div and kind == 'gz':
        raise ValueError("'gz' (MeanVarModel) has no flux form: its variance net is not a divergence")
    rs = np.random.RandomState(seed)
    hidden = [128, 64, 32, 32, 32, 32, 32]
    ks = [5, 5, 3, 3, 3, 3, 3, 3]

    def one(n_in):
        ch = [n_in] + hidden + [4 if div else 2]
        net = dict(conv_w=[], conv_b=[], bn_g=[], bn_b=[], bn_m=[], bn_v=[])
        for i in range(8):
            cin, cout, k = ch[i], ch[i + 1], ks[i]
            net['conv_w'].append((rs.randn(cout, cin, k, k) * np.sqrt(2.0 / (cin * k * k))).astype('float32'))
            net['conv_b'].append((0.1 * rs.randn(cout)).astype('float32'))
            if i < 7:
                net['bn_g'].append((1 + 0.1 * rs.randn(cout)).astype('float32'))
                net['bn_b'].append((0.1 * rs.randn(cout)).astype('float32'))
                net['bn_m'].append((0.5 + 0.1 * rs.randn(cout)).astype('float32'))
                net['bn_v'].append((0.5 + 0.2 * rs.rand(cout)).astype('float32'))
        return net
    if kind == 'ols':
        nets = [one(2)]
    else:
        nets = [one(2), one(2)] if kind == 'gz' else ([one(4), one(2)] if regression else [one(4)])
    x_std = np.array([7.784383342368528e-06, 1.0471941322975908e-06], np.float32)
    y_std = np.array([7.60611105349307e-12, 1.656513061486578e-13], np.float32)
    return nets, x_std, y_std


# ---- DeepInversion U-Net generator (CGANRegression(generator='DeepInversion'), deep_inversion.py:44-160) -------------
# residual units in qgx_unet_weights order: (state-dict prefix, C_in, C_out, with BatchNorm)
UNET_UNITS = [('res32_start', 32, 32, False), ('down64.conv.1', 32, 64, True), ('down128.conv.1', 64, 128, True),
              ('down256.conv.1', 128, 256, True), ('down512.conv.1', 256, 512, True), ('res512', 512, 512, True),
              ('up512.conv', 512, 256, True), ('up256.conv', 256, 128, True), ('up128.conv', 128, 64, True),
              ('up64.conv', 64, 32, True), ('res32_end', 32, 32, False)]
UNET_UPS = [('up512', 512), ('up256', 256), ('up128', 128), ('up64', 64)]


def unet_shapes():
    """every parameter / buffer of DeepInversionGenerator(4, 2)'s state dict -> shape (num_batches_tracked left out)"""
    s = {'conv32.weight': (32, 4, 3, 3), 'conv32.bias': (32,)}
    for p, ci, co, bn in UNET_UNITS:
        if bn:
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                s[f'{p}.bn.{k}'] = (ci,)
        s[f'{p}.conv.1.weight'] = (co, ci, 3, 3); s[f'{p}.conv.1.bias'] = (co,)
        if bn:
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                s[f'{p}.conv.2.{k}'] = (co,)
        s[f'{p}.conv.4.weight'] = (co, co, 3, 3); s[f'{p}.conv.4.bias'] = (co,)
        s[f'{p}.conv1.weight'] = (co, ci, 1, 1); s[f'{p}.conv1.bias'] = (co,)
    for p, c in UNET_UPS:
        s[f'{p}.upsampling.weight'] = (c, c // 2, 2, 2); s[f'{p}.upsampling.bias'] = (c // 2,)
    s['conv_end.weight'] = (2, 32, 1, 1); s['conv_end.bias'] = (2,)
    return s


def is_unet(net):
    return isinstance(net, dict) and 'conv32.weight' in net


def unet_from_state_dict(sd):
    """DeepInversionGenerator(4, 2) state dict -> {key: float32 array}; raises KeyError on a missing or an unexpected key
    (BatchNorm's num_batches_tracked counters are ignored)"""
    shapes = unet_shapes()
    keys = {k for k in sd.keys() if not k.endswith('num_batches_tracked')}
    missing, extra = sorted(set(shapes) - keys), sorted(keys - set(shapes))
    if missing or extra:
        raise KeyError(f'not a DeepInversionGenerator(4, 2) state dict: missing {missing[:5]}, unexpected {extra[:5]}')
    out = {}
    for k, shp in shapes.items():
        v = sd[k]
        a = np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, dtype=np.float32)
        if a.shape != shp:
            raise ValueError(f'{k}: shape {a.shape}, expected {shp}')
        out[k] = np.ascontiguousarray(a)
    return out


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _hash_uniform(tensor_id, n):
    """n values uniform in [-1, 1) from splitmix64(tensor_id << 32 | index), bit-reproducible on any machine"""
    with np.errstate(over='ignore'):
        z = _splitmix64((np.uint64(tensor_id) << np.uint64(32)) | np.arange(n, dtype=np.uint64))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 2.0 ** 53) - 1.0


def synthetic_unet():
    """Deterministic U-Net weights for tests and timing (no torch / numpy RNG stream): Kaiming-like scales (uniform of
    variance 2 / fan_in; the two branches of a residual unit 1 / 2 each) so that every stage's activations stay O(1),
    BatchNorm with non-trivial running statistics.  Keys and layouts of the reference's state dict."""
    out = {}
    r3 = np.sqrt(3.0)
    for tid, (k, shp) in enumerate(unet_shapes().items()):
        n = int(np.prod(shp))
        u = _hash_uniform(tid + 1, n)
        if k.endswith('running_mean'):
            v = 0.2 * u
        elif k.endswith('running_var'):
            v = 1.0 + 0.5 * u
        elif '.bn.' in k or '.conv.2.' in k:
            v = 1.0 + 0.2 * u if k.endswith('weight') else 0.1 * u
        elif k.endswith('bias'):
            v = 0.05 * u
        else:
            fan_in = n // shp[0] if 'upsampling' not in k else shp[0]
            branch = 0.5 if ('.conv.4.' in k or '.conv1.' in k) else 1.0
            v = u * r3 * np.sqrt(2.0 * branch / fan_in)
        out[k] = v.astype(np.float32).reshape(shp)
    return out


def unet_checksum(net):
    """sha256 of the tensors' float32 bytes in state-dict order, first 16 hex digits"""
    import hashlib
    h = hashlib.sha256()
    for k in unet_shapes():
        h.update(np.ascontiguousarray(net[k], dtype=np.float32).tobytes())
    return h.hexdigest()[:16]


def net_checksum(net):
    """sha256 of an AndrewCNN's float32 parameters in state-dict order (per block: conv weight, bias, BatchNorm weight, bias,
    running mean, running var), first 16 hex digits"""
    import hashlib
    h = hashlib.sha256()
    n = len(net['conv_w'])               # a net of another architecture (synthetic_arch): fewer blocks, BatchNorm / bias absent
    for i in range(n):
        arrays = [net['conv_w'][i]] + ([net['conv_b'][i]] if len(net['conv_b']) else [])
        if i < n - 1 and len(net['bn_g']):
            arrays += [net['bn_g'][i], net['bn_b'][i], net['bn_m'][i], net['bn_v'][i]]
        for a in arrays:
            h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()[:16]
