"""GPU: training of ANNModel on the device (csrc/ann_train.hip, include/qgx_train.h, tools/train_ANN.py) against the
restatement of tests/ann_training_restatement.py: stencil rows, scales, loss and gradient against float64 autograd, Adam
against torch.optim.Adam, a training trajectory through fit_ann, and the model folder it writes.  Loss and gradient run at
two batch sizes: up to 4096 rows, where every workgroup takes one tile, and above 256 x 128 rows, where workgroups add two
to four tiles into their partial sums (section 3b; tests/train_plan_restatement.py::ann_plan restates the partition).

All data follow the recipe of the restatement: band-limited images of unit variance, targets from a seeded teacher net plus
0.1 white noise, student weights from weights.synthetic_ann."""
import os

import numpy as np
import pytest
import torch

import ann_training_restatement as ar
import train_plan_restatement as tp
from redzone import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(3, [24, 24], False), (3, [24, 24], True), (5, [7, 13, 5], True), (1, [3], False), (7, [128], False)]


def _dev():
    return torch.device('cuda', 0)


# ---- 1. rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [24, 25])
@pytest.mark.parametrize('n_img', [1, 5])
def test_rows_are_bitwise_the_restatement(N, n_img):
    from pyqg_generative_amd._lib import lib, check, current_stream_ptr
    from pyqg_generative_amd.tools.train_ANN import ann_rows
    img = np.random.RandomState(N + n_img).randn(n_img, N, N).astype(np.float32)
    d = torch.as_tensor(img).cuda()
    for s in (1, 3, 5, 7):
        for step in (1, 3):
            want = ar.stencil_rows(img, s, step)
            nc = -(-N // step)
            assert want.shape == (nc * nc * n_img, s * s)
            g = guarded(want.shape, torch.float32, _dev())
            check(lib.qgx_ann_rows(d.data_ptr(), n_img, N, s, step, g.t.data_ptr(), current_stream_ptr()))
            torch.cuda.synchronize()
            g.check(written=True, what=f'rows N={N} s={s} step={step} n_img={n_img}')
            assert np.array_equal(g.t.cpu().numpy().view(np.int32), want.view(np.int32)), (N, s, step, n_img)
            assert torch.equal(ann_rows(d, s, step), g.t)


# ---- shared data ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recipe():
    """per stencil size: rows of 64 images at 24 x 24 (step 3: 4096 rows), their scales, on the host and the device"""
    out = {}
    for s, si in sorted({(s, si) for s, _, si in SHAPES}):
        q, f = ar.teacher_student_images(64, 24, 10 + s, s=s, scale_invariant=si)
        X, Y, xs, ys = ar.prepare_data([(q, f)], s)
        out[s, si] = dict(X=X, Y=Y, xs=xs, ys=ys, Xd=torch.as_tensor(X).cuda().contiguous(), Yd=torch.as_tensor(Y).cuda().contiguous())
    return out


def _student(s, hidden, si, seed=2):
    from pyqg_generative_amd import weights
    return weights.synthetic_ann(s, hidden, si, seed)


def _autograd64(net, x, y):
    m = ar.TorchANN(net, torch.float64)
    loss = m.loss(x, y)
    loss.backward()
    return float(loss.detach()), [p.grad.numpy().copy() for p in m.parameters()]


# ---- 3. loss and gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s,hidden,si', SHAPES)
def test_loss_and_gradient_match_float64_autograd(recipe, s, hidden, si):
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    r = recipe[s, si]
    net = _student(s, hidden, si)
    x64, y64 = ar.normalised(r['X'], r['Y'], r['xs'], r['ys'], torch.float64)
    # rows whose ReLU mask may legitimately differ between float32 and float64 are dropped before either side runs
    keep = np.nonzero(ar.min_abs_preactivation(net, x64.numpy()) >= 1e-4)[0]
    dropped = 1.0 - keep.size / x64.shape[0]
    print(f'\n{s} {hidden} si={si}: {dropped:.2%} of {x64.shape[0]} rows dropped')
    assert dropped <= 0.03
    t = AnnTrainer(net, device=0)
    # The single row of the n = 1 batch: its loss (yhat - y)^2 has the relative float32 error 2 eps' |yhat| / |yhat - y|
    # with eps' the forward pass's error of a few 1e-7, so a row whose output nearly equals its target cannot meet 2e-6
    # in ANY float32 evaluation (a first choice, a random row with |yhat - y| = 0.01 |yhat|, showed 1.2e-4).  The row is
    # therefore the best-conditioned one by the float64 net alone: the largest |yhat - y| / max(|yhat|, |y|).
    with torch.no_grad():
        yhat = ar.TorchANN(net, torch.float64)(x64[keep])
    ratio = ((yhat - y64[keep]).abs() / torch.maximum(yhat.abs(), y64[keep].abs())).reshape(-1).numpy()
    for n in (keep.size, 1, 257):
        idx = keep[:n] if n == keep.size else keep[np.random.RandomState(n).choice(keep.size, n, replace=False)]
        if n == 1:
            idx = keep[[int(np.argmax(ratio))]]
        loss64, g64 = _autograd64(net, x64[idx], y64[idx])
        idx_d = torch.as_tensor(idx.astype(np.int64)).cuda()
        acc = guarded((2,), torch.float64, _dev(), fill=0x00)
        t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc.t)
        g1 = t.read(_lib.TRAIN_GRAD)
        acc.check(what='loss_acc_dev')
        a = acc.t.cpu().numpy()
        assert a[1] == n
        loss = a[0] / a[1]
        err = abs(loss - loss64) / loss64
        print(f'  n = {n}: loss {loss:.6g}, relative error {err:.2e}')
        assert err <= 2e-6
        for (key, _), got, want in zip(t.shapes, t.unpack(g1).values(), g64):
            e = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
            print(f'    {key}: max gradient error {e:.2e} of max |g|')
            assert e <= 2e-6, (key, n, e)
        # a second identical call: the same bits, and the accumulator adds up
        t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc.t)
        g2 = t.read(_lib.TRAIN_GRAD)
        assert np.array_equal(g1.view(np.int32), g2.view(np.int32))
        acc.check(what='loss_acc_dev')
        assert np.array_equal(acc.t.cpu().numpy(), 2 * a)
        # on another stream: the same bits
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], None)
        st.synchronize()
        assert np.array_equal(g1.view(np.int32), t.read(_lib.TRAIN_GRAD).view(np.int32))
        # forward only: the same loss
        acc2 = guarded((2,), torch.float64, _dev(), fill=0x00)
        t.loss(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc2.t)
        torch.cuda.synchronize()
        acc2.check(what='loss_acc_dev')
        assert np.array_equal(acc2.t.cpu().numpy(), a)
    # idx = NULL: rows 0 .. n - 1
    acc3 = torch.zeros(2, dtype=torch.float64, device=_dev())
    acc4 = torch.zeros(2, dtype=torch.float64, device=_dev())
    t.loss(r['Xd'], r['Yd'], None, r['xs'], r['ys'], acc3)
    t.loss(r['Xd'], r['Yd'], torch.arange(r['Xd'].shape[0], device=_dev()), r['xs'], r['ys'], acc4)
    assert torch.equal(acc3, acc4) and float(acc3[1]) == r['Xd'].shape[0]
    t.close()


# ---- 3b. more than one tile per workgroup ----------------------------------------------------------------------------
# A gradient launch has at most 256 workgroups, and workgroup w walks the tiles w, w + 256, ... of RT <= 128 rows.  Up to
# 256 RT rows (every batch above) each workgroup runs ONE tile: the accumulation across tiles (part[o] + s[kk]), the barrier
# between tiles, and a short last tile written over the columns an earlier full tile left never run.  fit_ann's test-set
# loss and every batch of the reference's size on a small net are in that regime.
MANY_TILES_BOUND = 2e-6


@pytest.fixture(scope='module')
def dense():
    """per stencil size: the rows of 64 images at 24 x 24 at EVERY point (step 1): 36 864 rows, their scales"""
    out = {}
    for s, si in sorted({(s, si) for s, _, si in SHAPES}):
        q, f = ar.teacher_student_images(64, 24, 10 + s, s=s, scale_invariant=si)
        X, Y, xs, ys = ar.prepare_data([(q, f)], s, step=1)
        assert X.shape == (36864, s * s)
        out[s, si] = dict(X=X, Y=Y, xs=xs, ys=ys, Xd=torch.as_tensor(X).cuda().contiguous(), Yd=torch.as_tensor(Y).cuda().contiguous())
    return out


def _errors(loss, grads, loss64, g64):
    """relative error of the loss; per tensor the largest gradient error over the largest |gradient|"""
    return abs(loss - loss64) / loss64, [float(np.abs(np.asarray(g, np.float64) - w).max() / np.abs(w).max()) for g, w in zip(grads, g64)]


@pytest.mark.parametrize('s,hidden,si', SHAPES)
def test_many_tiles_per_workgroup_match_float64_autograd(dense, s, hidden, si):
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    r = dense[s, si]
    net = _student(s, hidden, si)
    x64, y64 = ar.normalised(r['X'], r['Y'], r['xs'], r['ys'], torch.float64)
    keep = np.nonzero(ar.min_abs_preactivation(net, x64.numpy()) >= 1e-4)[0]
    dropped = 1.0 - keep.size / x64.shape[0]
    assert dropped <= 0.03
    while keep.size % 4 == 0:
        keep = keep[:-1]
    n = keep.size
    # RT <= 128 for every net, so this alone means more than one tile in some workgroup; the restated plan says how many
    assert n > 256 * 128
    plan = tp.ann_plan(s, hidden, n)
    assert plan['nparts'] == 256 and plan['tiles_per_workgroup'] >= 2 and plan['last_rows'] % 4 != 0
    print(f'\n{s} {hidden} si={si}: {dropped:.2%} of {x64.shape[0]} rows dropped, {n} rows, {plan}')
    loss64, g64 = _autograd64(net, x64[keep], y64[keep])
    # the float32 torch CPU evaluation of the same rows: the yardstick the bound was chosen against
    m32 = ar.TorchANN(net, torch.float32)
    l32 = m32.loss(x64[keep].float(), y64[keep].float())
    l32.backward()
    cpu_loss, cpu_grad = _errors(float(l32.detach()), [p.grad.numpy() for p in m32.parameters()], loss64, g64)
    t = AnnTrainer(net, device=0)
    idx_d = torch.as_tensor(keep.astype(np.int64)).cuda()
    acc = guarded((2,), torch.float64, _dev(), fill=0x00)
    t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc.t)
    g1 = t.read(_lib.TRAIN_GRAD)
    acc.check(what='loss_acc_dev')
    a = acc.t.cpu().numpy()
    assert a[1] == n
    dev_loss, dev_grad = _errors(a[0] / a[1], t.unpack(g1).values(), loss64, g64)
    print(f'  loss: device {dev_loss:.2e}, float32 torch CPU {cpu_loss:.2e}')
    for (key, _), d, c in zip(t.shapes, dev_grad, cpu_grad):
        print(f'    {key}: device {d:.2e}, float32 torch CPU {c:.2e} of max |g|')
    assert dev_loss <= MANY_TILES_BOUND
    for (key, _), d in zip(t.shapes, dev_grad):
        assert d <= MANY_TILES_BOUND, (key, d)
    # a second identical call: the same bits, and the accumulator adds up
    t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc.t)
    assert np.array_equal(g1.view(np.int32), t.read(_lib.TRAIN_GRAD).view(np.int32))
    acc.check(what='loss_acc_dev')
    assert np.array_equal(acc.t.cpu().numpy(), 2 * a)
    # on another stream: the same bits
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        t.grad(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], None)
    st.synchronize()
    assert np.array_equal(g1.view(np.int32), t.read(_lib.TRAIN_GRAD).view(np.int32))
    # forward only: the same loss
    acc2 = guarded((2,), torch.float64, _dev(), fill=0x00)
    t.loss(r['Xd'], r['Yd'], idx_d, r['xs'], r['ys'], acc2.t)
    torch.cuda.synchronize()
    acc2.check(what='loss_acc_dev')
    assert np.array_equal(acc2.t.cpu().numpy(), a)
    # fit_ann's test-set path: idx = NULL over all 36 864 rows is idx = arange bit for bit, and the float64 loss of those rows
    R = r['Xd'].shape[0]
    assert tp.ann_plan(s, hidden, R)['tiles_per_workgroup'] >= 2
    acc3 = guarded((2,), torch.float64, _dev(), fill=0x00)
    acc4 = guarded((2,), torch.float64, _dev(), fill=0x00)
    t.loss(r['Xd'], r['Yd'], None, r['xs'], r['ys'], acc3.t)
    t.loss(r['Xd'], r['Yd'], torch.arange(R, device=_dev()), r['xs'], r['ys'], acc4.t)
    torch.cuda.synchronize()
    acc3.check(what='loss_acc_dev')
    acc4.check(what='loss_acc_dev')
    a3 = acc3.t.cpu().numpy()
    assert np.array_equal(a3.view(np.int64), acc4.t.cpu().numpy().view(np.int64)) and a3[1] == R
    with torch.no_grad():
        all64 = float(ar.TorchANN(net, torch.float64).loss(x64, y64))
        all32 = float(ar.TorchANN(net, torch.float32).loss(x64.float(), y64.float()))
    err = abs(a3[0] / a3[1] - all64) / all64
    print(f'  all {R} rows, idx = NULL: loss error device {err:.2e}, float32 torch CPU {abs(all32 - all64) / all64:.2e}')
    assert err <= MANY_TILES_BOUND
    t.close()


def test_zero_stencil_gives_nan_under_scale_invariance(recipe):
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    r = recipe[3, True]
    X = r['Xd'][:300].clone()
    X[7] = 0
    t = AnnTrainer(_student(3, [24, 24], True), device=0)
    acc = torch.zeros(2, dtype=torch.float64, device=_dev())
    t.grad(X, r['Yd'][:300].contiguous(), torch.arange(300, device=_dev()), r['xs'], r['ys'], acc)
    assert np.isnan(t.read(_lib.TRAIN_GRAD)).all() and np.isnan(float(acc[0]))
    t.close()


# ---- 4. Adam ----------------------------------------------------------------------------------------------------------
def _torch_adam(p0, grads, lr, dtype):
    p = torch.nn.Parameter(torch.as_tensor(p0).to(dtype))
    opt = torch.optim.Adam([p], lr=lr)
    for g in grads:
        p.grad = torch.as_tensor(g).to(dtype)
        opt.step()
    st = opt.state[p]
    return [x.detach().double().numpy() for x in (p, st['exp_avg'], st['exp_avg_sq'])]


def test_adam_matches_torch_optim_adam():
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    net = _student(3, [24, 24], False)
    t = AnnTrainer(net, device=0)
    rs = np.random.RandomState(11)
    p0 = t.read(_lib.TRAIN_PARAMS)
    grads = [(rs.randn(t.size) * 10.0 ** rs.uniform(-4, 0, t.size)).astype(np.float32) for _ in range(10)]
    lr = 1e-3
    zero = np.zeros(t.size, np.float32)
    t.write(_lib.TRAIN_M, zero)
    t.write(_lib.TRAIN_V, zero, adam_steps=0)
    for g in grads:
        t.write(_lib.TRAIN_GRAD, g)
        t.adam(lr)
    got = [t.read(w).astype(np.float64) for w in (_lib.TRAIN_PARAMS, _lib.TRAIN_M, _lib.TRAIN_V)]
    ref64 = _torch_adam(p0, grads, lr, torch.float64)
    ref32 = _torch_adam(p0, grads, lr, torch.float32)
    for name, g, r64, r32 in zip(('params', 'exp_avg', 'exp_avg_sq'), got, ref64, ref32):
        o = 0
        for key, shape in t.shapes:
            n = int(np.prod(shape))
            sl = slice(o, o + n)
            o += n
            err = np.abs(g[sl] - r64[sl]).max()
            err32 = np.abs(r32[sl] - r64[sl]).max()
            ulp = float(np.spacing(np.float32(np.abs(r64[sl]).max())))
            print(f'{name} {key}: device error {err:.3e}, torch float32 error {err32:.3e}, ulp {ulp:.3e}')
            assert err <= 4 * err32 + ulp, (name, key, err, err32, ulp)
    t.close()


def test_step_is_grad_then_adam_bitwise(recipe, dense):
    from pyqg_generative_amd import _lib
    from pyqg_generative_amd.tools.train_ANN import AnnTrainer
    for s, hidden, si in (SHAPES[0], SHAPES[2]):
        r = recipe[s, si]
        net = _student(s, hidden, si)
        a, b = AnnTrainer(net, device=0), AnnTrainer(net, device=0)
        acc_a = torch.zeros(2, dtype=torch.float64, device=_dev())
        acc_b = torch.zeros(2, dtype=torch.float64, device=_dev())
        rs = np.random.RandomState(5)
        for k, n in enumerate((1000, 129, 4096)):
            idx = torch.as_tensor(rs.permutation(r['X'].shape[0])[:n].astype(np.int64)).cuda()
            lr = 1e-3 * 0.5 ** k
            a.step(r['Xd'], r['Yd'], idx, r['xs'], r['ys'], lr, acc_a)
            b.grad(r['Xd'], r['Yd'], idx, r['xs'], r['ys'], acc_b)
            b.adam(lr)
            for what in range(4):
                assert np.array_equal(a.read(what).view(np.int32), b.read(what).view(np.int32)), (s, k, what)
            assert torch.equal(acc_a, acc_b)
        # one batch of more than 256 tiles: every workgroup's slice of the partial sums, some written over two or more tiles
        d = dense[s, si]
        n = 33001
        assert n > 32768 and tp.ann_plan(s, hidden, n)['tiles_per_workgroup'] >= 2
        idx = torch.as_tensor(rs.permutation(d['X'].shape[0])[:n].astype(np.int64)).cuda()
        a.step(d['Xd'], d['Yd'], idx, d['xs'], d['ys'], 1e-4, acc_a)
        b.grad(d['Xd'], d['Yd'], idx, d['xs'], d['ys'], acc_b)
        b.adam(1e-4)
        for what in range(4):
            assert np.array_equal(a.read(what).view(np.int32), b.read(what).view(np.int32)), (s, n, what)
        assert torch.equal(acc_a, acc_b)
        assert not np.array_equal(a.read(_lib.TRAIN_PARAMS), np.concatenate([np.r_[w.ravel(), bb] for w, bb in zip(net['w'], net['b'])]))
        a.close()
        b.close()


# ---- 2, 5, 6: through the facade -------------------------------------------------------------------------------------
E, BATCH = 4, 500


def _two_resolutions(seed):
    """24 x 24 with 48 images and 48 x 48 with 8 images: 3072 + 2048 rows, a short last batch of 120"""
    q1, f1 = ar.teacher_student_images(48, 24, seed)
    q2, f2 = ar.teacher_student_images(8, 48, seed + 50)
    return [(q1, f1), (q2, f2)]


def _perm(epoch, n):
    return np.random.RandomState(100 + epoch).permutation(n).astype(np.int64)


@pytest.fixture(scope='module')
def fitted(tmp_path_factory):
    from pyqg_generative_amd.tools.train_ANN import fit_ann
    train, test = _two_resolutions(1), _two_resolutions(2)[:1]
    folder = str(tmp_path_factory.mktemp('ann') / 'model')
    ds = lambda images: [ar.as_dataset(q, f, 2) for q, f in images]
    model = fit_ann(ds(train), ds(test), folder=folder, num_epochs=E, batch_size=BATCH, seed=4, permutations=_perm, verbose=False)
    return dict(model=model, folder=folder, train=train, test=test)


def test_scales_match_prepare_data(fitted):
    _, _, xs, ys = ar.prepare_data(fitted['train'], 3)
    m = fitted['model']
    assert isinstance(m.x_scale, float) and isinstance(m.y_scale, float)
    assert abs(m.x_scale - xs) <= float(np.spacing(np.float32(xs))) and abs(m.y_scale - ys) <= float(np.spacing(np.float32(ys)))


def test_trajectory_matches_the_restated_loop(fitted):
    from pyqg_generative_amd import weights
    X, Y, xs, ys = ar.prepare_data(fitted['train'], 3)
    Xt, Yt, _, _ = ar.prepare_data(fitted['test'], 3)
    R = X.shape[0]
    assert R == 5120 and R % BATCH != 0
    batches = [[_perm(e, R)[b:b + BATCH] for b in range(0, R, BATCH)] for e in range(E)]
    net = weights.synthetic_ann(3, [24, 24], False, 4)
    p_init = ar.TorchANN(net, torch.float64).packed()
    # the scales the device found (within an ulp of the restated ones, test above) so that both sides train on the same numbers
    m = fitted['model']
    log64, p64 = ar.train_loop(net, X, Y, Xt, Yt, m.x_scale, m.y_scale, batches, 1e-3, torch.float64)
    log32, p32 = ar.train_loop(net, X, Y, Xt, Yt, m.x_scale, m.y_scale, batches, 1e-3, torch.float32)
    sd = torch.load(os.path.join(fitted['folder'], 'net.pt'), map_location='cpu', weights_only=True)
    p = np.concatenate([sd[k].double().numpy().reshape(-1) for k in sd])
    from pyqg_generative_amd.tools.simulate import dataset_backend
    stats = dataset_backend().open_dataset(os.path.join(fitted['folder'], 'stats.nc'))
    move = np.linalg.norm(p64 - p_init)
    dev = {'parameters': np.linalg.norm(p - p64) / move}
    f32 = {'parameters': np.linalg.norm(p32 - p64) / move}
    for k in ('loss', 'loss_test'):
        got, w64, w32 = np.asarray(stats[k].values, dtype=np.float64), np.asarray(log64[k]), np.asarray(log32[k])
        dev[k] = np.abs(got / w64 - 1).max()
        f32[k] = np.abs(w32 / w64 - 1).max()
    print('\ntrajectory:', {k: f'device {dev[k]:.2e}, float32 loop {f32[k]:.2e}' for k in dev})
    for k in dev:
        bound = max(10 * f32[k], 1e-5)
        assert dev[k] <= bound, f'{k}: device deviation {dev[k]:.3e}, restated float32 loop {f32[k]:.3e}, bound {bound:.3e}'


def test_model_folder_loads_predicts_and_steps(fitted):
    from pyqg_generative_amd.models import ANNModel
    from pyqg_generative_amd.qgmodel import WeightedParameterization
    from pyqg_generative_amd.tools.simulate import dataset_backend, load_parameterization, run_simulation
    from pyqg_generative_amd.tools.parameters import EDDY_PARAMS
    folder, model = fitted['folder'], fitted['model']
    assert sorted(os.listdir(folder)) == ['model_args.json', 'net.pt', 'scale.json', 'stats.nc']
    assert isinstance(model, ANNModel) and model.folder == folder
    p = load_parameterization(folder)
    other = p.param if isinstance(p, WeightedParameterization) else p
    again = ANNModel(folder=folder)
    q, f = ar.teacher_student_images(8, 24, 9)
    ds = ar.as_dataset(q, f, 2)
    want = np.asarray(model.predict(ds)['q_forcing_advection'].values)
    assert want.shape == (2, 2, 2, 24, 24) and np.isfinite(want).all() and want.std() > 0
    for m in (other, again):
        assert (m.x_scale, m.y_scale) == (model.x_scale, model.y_scale)
        assert np.array_equal(np.asarray(m.predict(ds)['q_forcing_advection'].values), want)
    stats = dataset_backend().open_dataset(os.path.join(folder, 'stats.nc'))
    assert np.array_equal(np.asarray(stats['epoch'].values), np.arange(1, E + 1))
    for k in ('loss', 'loss_test'):
        v = np.asarray(stats[k].values)
        assert v.shape == (E,) and np.isfinite(v).all() and v[-1] < v[0], (k, v)
    N, nsteps = 32, 4
    params = EDDY_PARAMS.nx(N)._update({'tmax': 14400. * nsteps, 'log_level': 0})
    out = run_simulation(dict(params), parameterization=dict(self=p, sampling='AR1', nsteps=1), sampling_freq=14400. * 2)
    assert np.isfinite(np.asarray(out['q'].values)).all()


def test_same_seed_writes_the_same_net(tmp_path):
    from pyqg_generative_amd.tools.train_ANN import fit_ann
    q, f = ar.teacher_student_images(16, 24, 21, s=5, scale_invariant=True)
    ds = ar.as_dataset(q, f, 2)
    kw = dict(stencil_size=5, hidden_channels=[7, 13, 5], scale_invariant=True, num_epochs=2, batch_size=300, seed=6, verbose=False)
    a = fit_ann(ds, ds, folder=str(tmp_path / 'a'), **kw)
    b = fit_ann(ds, ds, folder=str(tmp_path / 'b'), **kw)
    assert open(os.path.join(a.folder, 'net.pt'), 'rb').read() == open(os.path.join(b.folder, 'net.pt'), 'rb').read()
    assert open(os.path.join(a.folder, 'stats.nc'), 'rb').read() == open(os.path.join(b.folder, 'stats.nc'), 'rb').read()
    c = fit_ann(ds, ds, folder=str(tmp_path / 'c'), **{**kw, 'seed': 7})
    assert open(os.path.join(a.folder, 'net.pt'), 'rb').read() != open(os.path.join(c.folder, 'net.pt'), 'rb').read()
    assert (a.stencil_size, a.hidden_channels, a.scale_invariant) == (5, [7, 13, 5], True)
