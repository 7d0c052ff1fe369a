"""GPU: AndrewCNN nets of any hidden_channels on the generic engine (csrc/conv_generic.hip, qgx_generator_create_arch): forward
against the reference's own AndrewCNN (tests/golden/generator_arch.npz), every launch variant and member count, the shipped
architecture through the new entry point bit for bit, online steps with AR1 and deterministic sampling, the model classes from
temporary folders, guard bands around the padded widths, and the grid sizes refused before anything is launched.  The edge cases
of arch_restatement.EDGE_CASES (widths 1 ... 256, 1 ... 8 output tiles, every chunk count, the missing flag combinations, kernel
sizes [3, 5, 5]) against the float64 restatement at every admitted grid size, every tile shape of rows_generic bit for bit
against the one-member launch, and the online and deterministic paths with a generic handle at 32, 64 and 96."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import golden

import arch_restatement as AR

pytestmark = pytest.mark.gpu

GEN_TOL = 2e-5          # the project's generator bound, of max|y|


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


KIND = {'A': 'gan', 'B': 'ols', 'C': 'ols', 'D': 'gan'}


@pytest.fixture(scope='module')
def gens():
    import pyqg_generative_amd as qa
    xs, ys = AR.scales()
    out = {name: qa.Generator(KIND[name], [AR.case_net(name)], xs, ys) for name in AR.CASES}
    yield out
    for g in out.values():
        g.close()


def _members(name, N, B):
    """B members from the fixture's snapshots: beyond them circular shifts (the convolutions are circular and the divergence is
    spectral, so the forward commutes with shifts: the shifted y64 is the float64 forward of the shifted input to 1e-15)"""
    x, b = AR.inputs(name, N), AR.y64(name, N)
    q0 = AR.fixture()[f'q{N}'].astype('float64')
    T = x.shape[0]
    xs, yb, qs = [], [], []
    for m in range(B):
        t, shift = m % T, ((5 * (m // T)) % N, (3 * (m // T)) % N)
        xs.append(np.roll(x[t], shift, axis=(-2, -1)))
        yb.append(np.roll(b[t], shift, axis=(-2, -1)))
        qs.append(np.roll(q0[t], shift, axis=(-2, -1)))
    return np.ascontiguousarray(np.stack(xs)), np.stack(yb), np.ascontiguousarray(np.stack(qs))


# Launch variants of k_convg reached (tiles of 32 output channels per workgroup NT, blockIdx.y slices ny, rows R, M-tiles):
#   first layer, planar input:  n_in = 4 (A, D), n_in = 2 (B, C)
#   NT = 2: A layer 1 (64), B layer 2 (40 -> 64);  NT = 1: every 32-wide-or-thinner layer;  NT = 1 with ny = 5: C (136 -> 160)
#   partly filled 8-channel groups: B (12, 20), C (136 = 4 chunks of 32 + 8);  last layer planar, 2 channels (A, B, C), 4 (D)
#   rows: B = 1, 3 at 16 x 16 -> R = 2, ONE M-tile (three waves idle); B = 40 -> R = 2 still (320 workgroups);
#   A / D at 64 x 64 with 16 members: the full tile of 8 M-tiles, MT = 2;  with 1 member: R = 1, two M-tiles
#   B at 48 x 48 with 44 members: the full tile of 12 M-tiles, MT = 3 (with NT = 1 and NT = 2);  with 22: R = 4, 6 M-tiles on
#   MT = 2 (two waves one tile short);  with 1: R = 2, three M-tiles
SHAPES = AR.SHAPES          # (listed there: the coverage test of tests/test_arch_cpu.py counts them with the edge cases' launches)


@pytest.mark.parametrize('name,N,B', SHAPES)
def test_cnn_forward_matches_the_reference(gens, name, N, B):
    """qgx_cnn_forward against the reference's FLOAT64 forward: 2e-5 of max|y|, the bound every reference-generated vector is held to"""
    x, y64, _ = _members(name, N, B)
    y = gens[name].cnn_forward(torch.as_tensor(x).cuda()).cpu().numpy()
    assert y.shape == (B, 2, N, N)
    err = np.abs(y - y64).max() / np.abs(y64).max()
    print(f'\nARCH case {name} N={N} B={B}: vs float64 {err:.2e} (reference float32 {AR.e_ref(name, N):.2e})')
    assert err < GEN_TOL
    if AR.CASES[name]['div']:
        assert np.abs(y.astype('float64').mean(axis=(-2, -1))).max() < 1e-6 * np.abs(y64).max()


def test_results_do_not_depend_on_the_member_count(gens):
    """the tile shape (rows per workgroup, chosen by the launch size) does not enter the summation order"""
    x, _, _ = _members('A', 64, 16)
    xd = torch.as_tensor(x).cuda()
    y16 = gens['A'].cnn_forward(xd)
    y1 = gens['A'].cnn_forward(xd[:1].contiguous())
    assert torch.equal(y16[:1], y1)


# ---- edge cases of the generic engine (AR.EDGE_CASES) ----------------------------------------------------------------------
def _edge_generator(name):
    import pyqg_generative_amd as qa
    xs, ys = AR.scales()
    return qa.Generator(AR.EDGE_KIND[name], [AR.edge_net(name)], xs, ys)


@pytest.fixture(scope='module')
def edge_gens():
    """name -> the case's handle, made on first use and shared"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _edge_generator(name)
        return made[name]
    yield get
    for g in made.values():
        g.close()


def _cnn_forward_between_canaries(gen, xd, what):
    """qgx_cnn_forward of net 0 with y between guard bands, written completely -> y (B, 2, N, N) float32 on the device"""
    import redzone
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    B, _, N, _ = xd.shape
    gen.check_size(B, N, 0)
    assert xd.dtype == torch.float32 and xd.is_contiguous() and xd.shape[1] == gen.n_in
    gy = redzone.guarded((B, 2, N, N), torch.float32, 'cuda')
    check(lib.qgx_cnn_forward(gen._h, 0, _ptr(xd), _ptr(gy.t), B, N, _stream()))
    torch.cuda.synchronize()
    gy.check(written=True, what=what)
    return gy.t


def _check_against_truth(name, y, y64, what):
    err = np.abs(y - y64).max() / np.abs(y64).max()
    print(f'\nARCH edge case {what}: vs float64 {err:.2e}' + (' (above a third of the bound)' if err > GEN_TOL / 3 else ''))
    assert err < GEN_TOL, what
    if AR.EDGE_CASES[name]['div']:
        assert np.abs(y.astype('float64').mean(axis=(-2, -1))).max() < 1e-6 * np.abs(y64).max(), what
    return err


@pytest.mark.parametrize('name,N', [(n, N) for n, c in AR.EDGE_CASES.items() for N in c['sizes']])
def test_edge_case_forward_matches_the_float64_truth(edge_gens, name, N):
    """qgx_cnn_forward against the float64 restatement (pinned to the reference's AndrewCNN in tests/test_arch_cpu.py): 2e-5 of
    max|y|, where the restatement's own float32 evaluation stays within 1.3e-6; y between canaries, written completely"""
    x, y64 = AR.edge_members(name, N, AR.EDGE_T)
    y = _cnn_forward_between_canaries(edge_gens(name), torch.as_tensor(x).cuda(), f'{name} N={N} y').cpu().numpy()
    assert y.shape == (AR.EDGE_T, 2, N, N)
    _check_against_truth(name, y, y64, f'{name} N={N} B={AR.EDGE_T}')


@pytest.mark.parametrize('name,N', list(AR.LADDER))
def test_every_tile_shape_gives_the_same_bits_and_meets_the_truth(name, N):
    """the member counts of AR.LADDER walk every rows-per-workgroup R that rows_generic gives at this size (tests/test_arch_cpu.py
    computes which), up and then down on ONE fresh handle (its workspaces grow, then are reused for smaller launches): three fixed
    members, placed first, in the middle and last, come out bit for bit as in their one-member launches — the tile shape does not
    enter the summation order — and every member meets the float64 truth"""
    Bs = AR.LADDER[(name, N)]
    gen = _edge_generator(name)
    xa, ya = AR.edge_members(name, N, max(max(Bs), 4))
    fixed = (0, 1, 3)          # members of `xa`: the two inputs and a shifted one
    assert Bs[0] == 1 and len(Bs) > 1
    # the one-member launches: the smallest tile of this size
    alone = [_cnn_forward_between_canaries(gen, torch.as_tensor(xa[f:f + 1].copy()).cuda(), f'{name} N={N} alone y') for f in fixed]
    for B in Bs + Bs[-2::-1]:
        where = {0: 0} if B == 1 else {0: 0, B // 2: 1, B - 1: 2}
        x, y64 = xa[:B].copy(), ya[:B].copy()
        for pos, f in where.items():
            x[pos], y64[pos] = xa[fixed[f]], ya[fixed[f]]
        y = _cnn_forward_between_canaries(gen, torch.as_tensor(x).cuda(), f'{name} N={N} B={B} y')
        for pos, f in where.items():
            assert torch.equal(y[pos], alone[f][0]), (B, pos)
        _check_against_truth(name, y.cpu().numpy(), y64, f'{name} N={N} B={B} (ladder)')
    gen.close()


def test_generic_handle_is_exact_f32_only(gens):
    from pyqg_generative_amd._lib import QgxError
    g = gens['A']
    assert g.info()['precision'] == 0 and g.precision == 0
    assert not g.wino_info()['enabled'] and not g.wino_info(64)['enabled']
    for value in (1, 3):
        with pytest.raises(QgxError, match='precision 0'):
            g.set_option('precision', value)
    g.set_option('precision', 0)
    with pytest.raises(QgxError, match='generic'):
        g.set_option('wino', 1)
    with pytest.raises(QgxError, match='generic engine'):          # the question is about the shipped 128 -> 64 layer
        g.layer2_kernel(2, 64)
    assert g.range_ok() is None


def _via_arch(kind, nets, xs, ys, force_generic=False):
    """a Generator whose handle comes from qgx_generator_create_arch whatever the architecture"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import _lib
    g = qa.Generator.__new__(qa.Generator)
    g.kind, g.device, g._h, g.unet, g.n_nets = kind, 0, C.c_void_p(0), False, len(nets)
    g.x_std, g.y_std = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    g.n_in = 2 if kind in ('gz', 'ols') else 4
    keep = []
    arr = (_lib.qgx_cnn_arch * len(nets))()
    for n, net in enumerate(nets):
        qa.Generator._arch_struct(net, arr[n], keep, force_generic)
    fx, fy = (C.c_float * 2)(*[float(v) for v in g.x_std]), (C.c_float * 2)(*[float(v) for v in g.y_std])
    _lib.check(_lib.lib.qgx_generator_create_arch(qa.Generator.KINDS[kind], arr, len(nets), fx, fy, 0, C.byref(g._h)))
    return g


def test_shipped_architecture_through_the_new_entry_point_is_the_same_handle():
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    d = golden('weights_gan.npz')
    nets, xs, ys = [weights.net_from_npz(d, 'net0_')], d['x_std'], d['y_std']
    a, b = qa.Generator('gan', nets, xs, ys), _via_arch('gan', nets, xs, ys)
    assert a.info() == b.info() and a.info()['precision'] == 3
    assert [a.wino_info(N) for N in (32, 48, 64, 96, 128)] == [b.wino_info(N) for N in (32, 48, 64, 96, 128)]
    rs = np.random.RandomState(12)
    for B in (2, 40):
        x = torch.as_tensor(rs.randn(B, 4, 64, 64).astype(np.float32)).cuda()
        assert a.layer2_kernel(B, 64) == b.layer2_kernel(B, 64)
        assert torch.equal(a.cnn_forward(x), b.cnn_forward(x)), B
    # ... and forced through the generic engine it is the float32 class of the exact-f32 kernels
    c = _via_arch('gan', nets, xs, ys, force_generic=True)
    assert c.info()['precision'] == 0
    a.set_option('precision', 0)
    x = torch.as_tensor(rs.randn(3, 4, 64, 64).astype(np.float32)).cuda()
    y0, yc = a.cnn_forward(x).cpu().numpy(), c.cnn_forward(x).cpu().numpy()
    err = _rel(yc, y0)
    print(f'\nshipped net, generic engine vs exact-f32 kernels: {err:.2e}')
    assert err < 4e-6          # two float32 evaluations of 1-2e-6 each against the exact result
    for g in (a, b, c):
        g.close()


def test_generic_generator_with_a_shipped_regression_net():
    """CGANRegression(regression='full_loss', hidden_channels=A's): net 0 on the generic engine, net_mean — default widths whatever
    hidden_channels says — on the templated exact-f32 kernels of the same handle; S = y_std (G([x, z]) + net_mean(x)) (FIN_SUM),
    and the deterministic mean of it"""
    import pyqg_generative_amd as qa
    from pyqg_generative_amd import weights
    xs, ys = AR.scales()
    mean_net = weights.synthetic('ols', seed=2)[0][0]
    gen = qa.Generator('gan', [AR.case_net('A'), mean_net], xs, ys)
    assert gen.info()['precision'] == 0
    N = 16
    x, y64, q = _members('A', N, 3)
    m64 = AR.forward(mean_net, np.ascontiguousarray(x[:, :2]))
    y1 = gen.cnn_forward(torch.as_tensor(np.ascontiguousarray(x[:, :2])).cuda(), inet=1).cpu().numpy()
    assert _rel(y1, m64) < GEN_TOL
    S = gen.forward(torch.as_tensor(q).cuda(), torch.as_tensor(np.ascontiguousarray(x[:, 2:])).cuda(), demean=False).cpu().numpy()
    want = (y64 + m64) * ys.astype('float64').reshape(1, 2, 1, 1)
    err = (np.abs(S - want) / np.abs(want).max(axis=(-2, -1), keepdims=True)).max()
    print(f'\nARCH regression (generic G + shipped net_mean): {err:.2e}')
    assert err < GEN_TOL
    assert _rel(y64 * ys.reshape(1, 2, 1, 1), want) > 1e-2          # the regression net is not a rounding-level term
    Sm = gen.forward_mean(torch.as_tensor(q).cuda(), 4, seed=3, demean=False)
    assert torch.isfinite(Sm).all() and not torch.equal(Sm, torch.as_tensor(S).cuda())
    gen.close()


# ---- online ---------------------------------------------------------------------------------------------------------------
def _eddy_like_q(rs, B, N):
    from oracle import qg_ref
    m = qg_ref.QGModelRef(nx=N)
    qh = np.fft.rfftn(rs.randn(B, 2, N, N), axes=(-2, -1)) * (m.wv < 2. / 3. * m.kk[-1])
    q = np.fft.irfftn(qh, axes=(-2, -1))
    return q / q.std(axis=(-2, -1), keepdims=True) * AR.scales()[0].astype('float64').reshape(1, 2, 1, 1)


@pytest.mark.parametrize('name,N,sampling,B,opts,M', [
    ('A', 16, 'AR1', 3, {}, 4), ('A', 16, 'AR1', 2, dict(streams=2), 4), ('A', 16, 'constant', 2, dict(genfuse=0), 4),
    ('A', 16, 'deterministic', 2, {}, 4), ('B', 16, 'AR1', 3, {}, 4), ('B', 16, 'AR1', 2, dict(streams=2), 4),
    # edge case I at the sizes ensembles run at: R = 2 of the 64 x 64 ladder; 130 members (full tiles, an odd half); the AUTOMATIC
    # halves at 96 x 96 (16 members: R = 4 as a whole, 8 per half: R = 2, each half in its own workspace); the unfused prologue at
    # 96 x 96; deterministic sampling with M = 128 realisations of 2 members: one pseudo-batch of 256 at 32 x 32 (R = 8)
    ('I', 64, 'AR1', 4, {}, 4), ('I', 64, 'constant', 130, {}, 4), ('I', 96, 'AR1', 16, {}, 4), ('I', 96, 'AR1', 3, dict(genfuse=0), 4),
    ('I', 32, 'deterministic', 2, {}, 128)],
    ids=['gan-ar1', 'gan-ar1-halves', 'gan-const-unfused', 'gan-deterministic', 'ols-ar1', 'ols-ar1-halves',
         'thin-64-ar1', 'thin-64-const-130', 'thin-96-ar1-auto-halves', 'thin-96-ar1-unfused', 'thin-32-deterministic-256'])
def test_online_forcing_is_the_generators_own(gens, edge_gens, name, N, sampling, B, opts, M):
    """three steps (the first table's nets at 16 x 16, the thin edge case at 32, 64 and 96): the forcing the (fused) step applied
    equals qgx_generator_forward / _forward_mean on the state and the latent noise read back from the engine — bit for bit, as the
    fused prologue is against separate kernels (test_gpu_div.py::test_fused_step_prologue_is_bit_identical); the two-halves
    schedule runs the second workspace"""
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    seed, off = 21, 5
    gen = gens[name] if name in gens else edge_gens(name)
    q0 = _eddy_like_q(np.random.RandomState(3 + B), B, N)
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=14400. * 16 / N)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_q(q0)
    if 'streams' in opts or (N, B) == (96, 16):
        assert e.step_streams(gen, sampling=sampling) == 2          # at 96 x 96 with 16 ... 64 members: with no option set
    else:
        assert e.step_streams(gen, sampling=sampling) == 1
    for s in range(3):
        q_pre = e.get(L.F_Q).clone()
        e.step(1, generator=gen, sampling=sampling, nsteps_decor=1, seed=seed, member_offset=off, n_mean=M)
        S = e.get(L.F_S)
        if sampling == 'deterministic':
            want = gen.forward_mean(q_pre, M, seed=seed, member_offset=off, step=s, demean=True)
        elif gen.noise_dtype is None:
            want = gen.forward(q_pre, None, demean=True)
        else:
            want = gen.forward(q_pre, e.get(L.F_Z).contiguous(), demean=True)
        diff = (S - want).abs().max().item() / want.abs().max().item()
        print(f'\nARCH online {name} N={N} {sampling} B={B} {opts} step {s}: |S - forward| / max {diff:.1e}')
        assert torch.equal(S, want), (s, diff)
        assert S.abs().max().item() > 0
    assert e.tc == 3
    if gen.noise_dtype is None:
        # an OLS net takes no latent noise, and the reference defines no predict_mean_snapshot for OLSModel: deterministic sampling
        # (M = 4) is refused for it before anything is launched, on the generic engine as on the shipped nets
        from pyqg_generative_amd._lib import QgxError
        with pytest.raises(QgxError, match='predict_mean_snapshot'):
            e.step(1, generator=gen, sampling='deterministic', n_mean=4, seed=seed)
        with pytest.raises(QgxError, match='predict_mean_snapshot'):
            gen.forward_mean(e.get(L.F_Q), 4)
        assert e.tc == 3
    e.close()


S_TOL = 2e-5            # tests/test_gpu_deterministic.py's bound on a deterministic forcing, of max|S| per member and layer


def test_forward_mean_of_a_generic_net_matches_the_float64_truth(edge_gens):
    """qgx_generator_forward_mean with a generic handle (edge case I, 32 x 32, 2 members, M = 5 realisations: one pseudo-batch of
    10) against y_std * mean_j AR.forward([q / x_std, z_j]) in float64, z_j from the Philox streams the device draws
    (tests/test_gpu_deterministic.py::_realisations); de-mean off and on"""
    from oracle import samplers_ref, gen_ref
    N, B, M, seed, off, t = 32, 2, 5, 31, 7, 3
    gen, net = edge_gens('I'), AR.edge_net('I')
    xs, ys = AR.scales()
    q = _eddy_like_q(np.random.RandomState(29), B, N)
    X = q.astype('float32') / xs.reshape(1, 2, 1, 1)
    assert X.dtype == np.float32
    raw = np.empty((B, 2, N, N))
    for b in range(B):
        z = np.stack([samplers_ref.philox_normal(seed, off + b, t | (j + 1) << 32, 2 * N * N)[0].reshape(2, N, N) for j in range(M)])
        x = np.concatenate([np.broadcast_to(X[b], (M, 2, N, N)), z], axis=1)
        raw[b] = AR.forward(net, x).mean(axis=0) * ys.astype('float64').reshape(2, 1, 1)
    dem = np.stack([gen_ref.demean(r) for r in raw])
    scale = np.abs(dem).max(axis=(-2, -1), keepdims=True)
    qd = torch.as_tensor(q).cuda().contiguous()
    kw = dict(seed=seed, member_offset=off, step=t)
    Sraw = gen.forward_mean(qd, M, demean=False, **kw).cpu().numpy()
    S = gen.forward_mean(qd, M, demean=True, **kw).cpu().numpy()
    e_raw, e_dem = (np.abs(Sraw - raw) / scale).max(), (np.abs(S - dem) / scale).max()
    print(f'\nARCH forward_mean I N={N} B={B} M={M}: raw {e_raw:.2e}, de-meaned {e_dem:.2e}')
    assert e_raw < S_TOL and e_dem < S_TOL
    assert np.abs(S.mean(axis=(-2, -1))).max() < 1e-14 * scale.max() * N * N
    # neither the de-meaning nor the mean over realisations is a rounding-level step of this case
    assert (np.abs(Sraw - dem) / scale).max() > 10 * S_TOL
    one = gen.forward_mean(qd, 1, demean=False, **kw).cpu().numpy()
    assert (np.abs(one - raw) / scale).max() > 10 * S_TOL


# ---- the model classes ------------------------------------------------------------------------------------------------------
class _M:
    pass


def test_cvae_and_ols_classes_from_folders(tmp_path):
    """CVAERegression(hidden_channels=A's) and OLSModel(hidden_channels=B's, batch_norm=False, bias=False) through
    load_parameterization, against the reference's own classes' predict_snapshot (fixture), then a run_simulation"""
    from pyqg_generative_amd.tools.simulate import load_parameterization, run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    from pyqg_generative_amd.tools.cnn_tools import apply_function
    from pyqg_generative_amd.models import CVAERegression, OLSModel
    a, b = AR.CASES['A'], AR.CASES['B']
    fa, fb = tmp_path / 'vae', tmp_path / 'ols'
    fa.mkdir(); fb.mkdir()
    AR.write_folder(fa, 'vae', [AR.case_net('A')], dict(model='CVAERegression', regression='None', decoder_var='adaptive', div=False,
                                                       hidden_channels=a['hidden_channels']))
    AR.write_folder(fb, 'ols', [AR.case_net('B')], dict(model='OLSModel', div=False, batch_norm=False, bias=False, final_activation='None',
                                                       hidden_channels=b['hidden_channels']))
    vae, ols = load_parameterization(str(fa)).param, load_parameterization(str(fb)).param
    assert (ols.batch_norm, ols.bias, ols.hidden_channels) == (False, False, b['hidden_channels'])
    assert isinstance(vae, CVAERegression) and isinstance(ols, OLSModel)
    d = AR.fixture()
    N, T = 16, 2
    z = AR.latent_noise(N, T)
    for t in range(T):
        m = _M()
        m.q = d[f'q{N}'][t].astype('float64')
        for model, key, noise in ((vae, 'vae_S_16', z[t:t + 1]), (ols, 'ols_S_16', 0)):
            S, ref = model.predict_snapshot(m, noise), d[key][t].astype('float64')
            err = (np.abs(S - ref) / np.abs(ref).max(axis=(1, 2), keepdims=True)).max()
            print(f'\nARCH {key} snapshot {t}: {err:.2e}')
            assert S.shape == (2, N, N) and err < GEN_TOL
    # apply_function on the bound nets
    y = apply_function(ols.net, AR.inputs('B', N))
    assert _rel(y, AR.y64('B', N)) < GEN_TOL
    y = apply_function(vae.decoder, AR.inputs('A', N))
    assert _rel(y, AR.y64('A', N)) < GEN_TOL
    # predict's layout (offline) and the Monte-Carlo mean of the VAE
    from pyqg_generative_amd.tools.simulate import dataset_backend
    xr = dataset_backend()
    qv = d[f'q{N}'][:T].astype('float64').reshape(1, T, 2, N, N)
    ds = xr.Dataset({'q': (['run', 'time', 'lev', 'y', 'x'], qv)})
    out = ols.predict(ds)
    assert _rel(np.asarray(out['q_forcing_advection'].values)[0], d['ols_S_16'].astype('float64')) < GEN_TOL
    out = vae.predict(ds, M=3)
    for k in ('q_forcing_advection', 'q_forcing_advection_mean', 'q_forcing_advection_var'):
        assert out[k].shape == qv.shape and np.isfinite(np.asarray(out[k].values)).all()
    Sm = vae.predict_mean_snapshot(m, M=4, seed=9)
    assert Sm.shape == (2, N, N) and np.isfinite(Sm).all()
    # online through the facade
    N = 32
    q0 = _eddy_like_q(np.random.RandomState(2), 1, N)[0]
    params = EDDY_PARAMS.nx(N)._update({'tmax': 14400. * 3, 'log_level': 0})
    ds = run_simulation(dict(params), parameterization=dict(self=vae, sampling='AR1', nsteps=1), q_init=q0, sampling_freq=14400. * 3)
    q = np.asarray(ds['q'].values)
    assert q.shape[-3:] == (2, N, N) and np.isfinite(q).all() and np.abs(q[-1] - q0).max() > 0


def test_mean_var_model_with_three_hidden_layers(tmp_path):
    """GZ with hidden_channels = [32, 16, 16]: both nets on the generic engine; predict's layout and predict_mean_snapshot against
    the float64 restatement"""
    from pyqg_generative_amd import weights
    from pyqg_generative_amd.models import MeanVarModel
    from pyqg_generative_amd.tools.simulate import load_parameterization, dataset_backend
    hidden = [32, 16, 16]
    nets = [weights.synthetic_arch(2, hidden, seed=s) for s in (41, 42)]
    folder = AR.write_folder(tmp_path, 'gz', nets, dict(model='MeanVarModel', hidden_channels=hidden))
    model = load_parameterization(folder).param
    assert isinstance(model, MeanVarModel) and model.hidden_channels == hidden and model.device_generator().info()['precision'] == 0
    N = 16
    d = AR.fixture()
    xs, ys = AR.scales()
    q = d[f'q{N}'].astype('float64')
    X = d[f'q{N}'] / xs.reshape(1, 2, 1, 1)
    mean64 = AR.forward(nets[0], X) * ys.astype('float64').reshape(1, 2, 1, 1)
    var64 = np.logaddexp(0, AR.forward(nets[1], X)) * (ys.astype('float64') ** 2).reshape(1, 2, 1, 1)
    m = _M()
    m.q = q[0]
    Sm = model.predict_mean_snapshot(m)
    assert Sm.shape == (2, N, N) and (np.abs(Sm - mean64[0]) / np.abs(mean64[0]).max(axis=(1, 2), keepdims=True)).max() < GEN_TOL
    xr = dataset_backend()
    qv = q.reshape(1, q.shape[0], 2, N, N)
    out = model.predict(xr.Dataset({'q': (['run', 'time', 'lev', 'y', 'x'], qv)}), seed=3)
    mean, var = np.asarray(out['q_forcing_advection_mean'].values)[0], np.asarray(out['q_forcing_advection_var'].values)[0]
    assert out['q_forcing_advection'].shape == qv.shape
    assert _rel(mean, mean64) < GEN_TOL and _rel(var, var64) < GEN_TOL
    # one forcing through qgx_generator_forward (FIN_GZ): mean + z sqrt(var)
    z = np.random.RandomState(5).randn(1, 2, N, N)
    S = model.predict_snapshot(m, z)
    want = mean64[0] + z[0] * np.sqrt(var64[0])
    assert (np.abs(S - want) / np.abs(want).max(axis=(1, 2), keepdims=True)).max() < GEN_TOL


@pytest.mark.parametrize('N', [16, 64])
def test_ols_and_cvae_div_with_the_shipped_widths(tmp_path, N):
    """OLSModel(div=True) against the reference's AndrewCNN(2, 2, div=True) (generator_div.npz, ols_*); CVAERegression(div=True)
    against the flux-form generator vectors of the same fixture and the restatement; both through load_parameterization"""
    import div_restatement as R
    from pyqg_generative_amd.models import OLSModel, CVAERegression
    from pyqg_generative_amd.tools.simulate import load_parameterization
    fo, fv = tmp_path / 'ols', tmp_path / 'vae'
    fo.mkdir(); fv.mkdir()
    AR.write_folder(fo, 'ols', [R.flux_net_dict('ols')], dict(model='OLSModel', div=True))
    AR.write_folder(fv, 'vae', [R.flux_net_dict('gan')], dict(model='CVAERegression', div=True))
    xs, ys = R.scales()
    np.testing.assert_array_equal(xs, AR.scales()[0])
    ols, vae = load_parameterization(str(fo)).param, load_parameterization(str(fv)).param
    assert isinstance(ols, OLSModel) and isinstance(vae, CVAERegression) and ols.div is True and vae.div is True
    d = R.fixture()
    T = R.y32('ols', N).shape[0]
    for t in range(T):
        m = _M()
        m.q = d[f'q{N}'][t].astype('float64')
        S = ols.predict_snapshot(m, 0)
        ref = R.y64('ols', N)[t] * ys.astype('float64').reshape(2, 1, 1)
        assert (np.abs(S - ref) / np.abs(ref).max(axis=(1, 2), keepdims=True)).max() < GEN_TOL
    y = ols.net(torch.as_tensor(R.inputs('ols', N)).cuda()).cpu().numpy()
    assert _rel(y, R.y64('ols', N)) < GEN_TOL
    x = R.inputs('gan', N)
    y = vae.decoder(torch.as_tensor(x).cuda()).cpu().numpy()
    assert _rel(y, R.y64('gan', N)) < GEN_TOL
    ora = R.FluxGeneratorRef('vae', [R.flux_net_ref('gan')], xs, ys)
    m = _M()
    m.q = d[f'q{N}'][0].astype('float64')
    z = x[:1, 2:]
    S, ref = vae.predict_snapshot(m, z), ora.predict_snapshot(m.q[None], z)
    assert (np.abs(S - ref) / np.abs(ref).max(axis=(1, 2), keepdims=True)).max() < GEN_TOL


# ---- guard bands ------------------------------------------------------------------------------------------------------------
def test_outputs_of_a_padded_net_stay_inside_their_buffers(gens):
    """case B (widths 24, 40, 12, 20: every layer padded in K and N) at 48 x 48 with 3 members — tiles of 3 M-tiles on 4 waves,
    the last workgroup's included: qgx_cnn_forward's y and qgx_generator_forward's S between canaries, written completely"""
    import redzone
    from pyqg_generative_amd._lib import lib, check
    from pyqg_generative_amd.engine import _ptr, _stream
    gen = gens['B']
    N, B = 48, 3
    x, y64, q = _members('B', N, B)
    xd, qd = torch.as_tensor(x).cuda(), torch.as_tensor(q).cuda()
    fx, fq = redzone.frozen(xd), redzone.frozen(qd)
    for fill in (0xFF, 0x00):
        gy = redzone.guarded((B, 2, N, N), torch.float32, 'cuda', fill=fill)
        check(lib.qgx_cnn_forward(gen._h, 0, _ptr(xd), _ptr(gy.t), B, N, _stream()))
        torch.cuda.synchronize()
        gy.check(written=True, what='qgx_cnn_forward y')
        assert _rel(gy.t.cpu().numpy(), y64) < GEN_TOL
        gs = redzone.guarded((B, 2, N, N), torch.float64, 'cuda', fill=fill)
        check(lib.qgx_generator_forward(gen._h, _ptr(qd), None, _ptr(gs.t), B, N, 0, _stream()))
        torch.cuda.synchronize()
        gs.check(written=True, what='qgx_generator_forward S')
        ys = AR.scales()[1].astype('float64').reshape(1, 2, 1, 1)
        assert _rel(gs.t.cpu().numpy() / ys, y64) < GEN_TOL
    fx.check('x'); fq.check('q')


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [24, 192])
def test_other_grid_sizes_are_refused_before_anything_is_launched(gens, N):
    import pyqg_generative_amd as qa
    import pyqg_generative_amd._lib as L
    from pyqg_generative_amd._lib import lib, QgxError
    from pyqg_generative_amd.engine import _ptr, _stream
    gen, B = gens['A'], 2
    assert lib.qgx_generator_size_ok(gen._h, -1, B, N) == -1 and f'N = {N}' in lib.qgx_last_error().decode()
    assert lib.qgx_generator_size_ok(gen._h, 0, B, 64) == 0
    x = torch.zeros((B, 4, N, N), dtype=torch.float32, device='cuda')
    y = torch.full((B, 2, N, N), 7.0, dtype=torch.float32, device='cuda')
    assert lib.qgx_cnn_forward(gen._h, 0, _ptr(x), _ptr(y), B, N, _stream()) == -1
    assert f'N = {N}' in lib.qgx_last_error().decode()
    torch.cuda.synchronize()
    assert (y == 7.0).all()
    with pytest.raises(ValueError, match=rf'N = {N}\b'):
        gen.cnn_forward(x)
    q0 = _eddy_like_q(np.random.RandomState(N), B, N)
    e = qa.EnsembleEngine(nx=N, n_members=B, dt=3600.)
    e.set_q(q0)
    e.step(2)
    before = [e.tc] + [e.get(f).clone() for f in (L.F_QH, L.F_Z, L.F_Q, L.F_S)]
    gen.check_size = lambda *a, **k: None            # past the facade: qgx_step itself
    try:
        for kw in (dict(sampling='AR1', nsteps_decor=2, seed=3), dict(sampling='constant', nsteps_decor=3, seed=3),
                   dict(sampling='deterministic', n_mean=4, seed=3)):
            with pytest.raises(QgxError, match=rf'N = {N}\b'):
                e.step(1, generator=gen, **kw)
    finally:
        del gen.check_size
    torch.cuda.synchronize()
    after = [e.tc] + [e.get(f).clone() for f in (L.F_QH, L.F_Z, L.F_Q, L.F_S)]
    assert before[0] == after[0] == 2
    for a, b in zip(before[1:], after[1:]):
        assert torch.equal(a, b)
    e.step(1)
    assert e.tc == 3
    if gen.noise_dtype is None:
        # an OLS net takes no latent noise, and the reference defines no predict_mean_snapshot for OLSModel: deterministic sampling
        # (M = 4) is refused for it before anything is launched, on the generic engine as on the shipped nets
        from pyqg_generative_amd._lib import QgxError
        with pytest.raises(QgxError, match='predict_mean_snapshot'):
            e.step(1, generator=gen, sampling='deterministic', n_mean=4, seed=seed)
        with pytest.raises(QgxError, match='predict_mean_snapshot'):
            gen.forward_mean(e.get(L.F_Q), 4)
        assert e.tc == 3
    e.close()
    # the handle stays usable
    xg, y64, _ = _members('A', 16, 1)
    assert _rel(gen.cnn_forward(torch.as_tensor(xg).cuda()).cpu().numpy(), y64) < GEN_TOL
