"""Training of ANNModel on the device (reference: models/ann_model.py:34-66 fit / save_model, tools/cnn_tools.py:373-396
prepare_data_ANN, :645-700 train, driver tools/train_ANN.py).

``fit_ann`` builds the stencil rows of the datasets on the device (csrc/ann_train.hip, qgx_ann_rows), trains the net with
the fused loss / gradient and Adam kernels of the trainer handle (include/qgx_train.h) and writes the reference's model
folder: net.pt, scale.json, model_args.json, stats.nc.  It returns ``ANNModel(folder=...)`` read back from those files.
This module holds the row builder, the trainer handle, the folder writer and the fit; what it shares with the CNN fits
(argument checks, schedule, dataset extraction, stats.nc, the epoch log, the command line) is in tools/train_common.py.

Command line:
    python -m pyqg_generative_amd.tools.train_ANN --train 'GLOB' --validate 'GLOB' [--test 'GLOB'] \\
        --model_args "{'stencil_size': 3}" --fit_args "{'num_epochs': 50}"
Every glob names netCDF files concatenated along `run`; several globs separated by commas are several datasets (the
reference trains on 48 x 48 and 96 x 96 together).  With --test, `offline-<k>.nc` (test_offline) is written per test dataset.
"""
import ctypes as C
import json
import os
from time import time

import numpy as np
import torch

from .. import _lib, weights as _weights
from .._lib import lib, check
from ..engine import Generator
from .train_common import (check_fit_args, command_line, cuda_device, learning_rates, log_epoch, print_start, save_state_dict,
                           stacked, write_log)

STEP = 3          # prepare_data_ANN keeps every third point in y and x (cnn_tools.py:384-386)


def ann_rows(img, stencil_size, step=1):
    """xarray_to_stencil on the device: img (n_img, N, N) float32 CUDA tensor -> rows (R, s * s) float32, R = ceil(N / step)^2 *
    n_img, row ((j / step) * ceil(N / step) + i / step) * n_img + img, feature dy * s + dx the wrapped neighbour"""
    if img.dim() != 3 or img.shape[-1] != img.shape[-2] or img.dtype != torch.float32 or not img.is_cuda:
        raise ValueError(f'ann_rows: (n_img, N, N) float32 device images, not {tuple(img.shape)} {img.dtype} on {img.device}')
    img = img.contiguous()
    n_img, N = int(img.shape[0]), int(img.shape[-1])
    s, step = int(stencil_size), int(step)
    if step < 1:
        raise ValueError(f'ann_rows: step = {step}')
    nc = -(-N // step)
    with torch.cuda.device(img.device):
        rows = torch.empty((nc * nc * n_img, s * s), dtype=torch.float32, device=img.device)
        check(lib.qgx_ann_rows(img.data_ptr(), n_img, N, s, step, rows.data_ptr(), _lib.current_stream_ptr()))
    return rows


class AnnTrainer:
    """The trainer handle of include/qgx_train.h: parameters, gradient and Adam's moments live on the device.  `net`: a
    weights.synthetic_ann / ann_from_state_dict dict.  Row buffers x (R, s * s), y (R, 1) and indices (int64) are CUDA
    tensors of the handle's device; index values are not checked against R by the library, so they are checked here."""

    def __init__(self, net, device=0):
        self.net = {k: net[k] for k in ('stencil_size', 'hidden', 'scale_invariant')}
        self.device = int(device)
        keep = []
        a = Generator._ann_struct(net, keep)
        self._h = C.c_void_p()
        check(lib.qgx_ann_trainer_create(C.byref(a), self.device, C.byref(self._h)))
        self.size = int(lib.qgx_ann_trainer_size(self._h))
        widths = [int(net['stencil_size']) ** 2] + [int(h) for h in net['hidden']] + [1]
        self.shapes = []
        for l in range(len(widths) - 1):
            self.shapes += [(f'layers.{2 * l}.weight', (widths[l + 1], widths[l])), (f'layers.{2 * l}.bias', (widths[l + 1],))]

    def close(self):
        if getattr(self, '_h', None):
            lib.qgx_ann_trainer_destroy(self._h)
            self._h = None

    __del__ = close

    def _batch(self, x, y, idx, n_rows=None):
        F = int(self.net['stencil_size']) ** 2
        if x.dtype != torch.float32 or y.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != F or y.numel() != x.shape[0]:
            raise ValueError(f'row buffers: x (R, {F}) and y (R) float32, not {tuple(x.shape)} {x.dtype}, {tuple(y.shape)} {y.dtype}')
        if not (x.is_cuda and y.is_cuda and x.is_contiguous() and y.is_contiguous()):
            raise ValueError('row buffers must be contiguous CUDA tensors')
        if idx is None:
            n = x.shape[0] if n_rows is None else int(n_rows)
            return n, None
        if idx.dtype != torch.int64 or not idx.is_cuda or not idx.is_contiguous() or idx.dim() != 1:
            raise ValueError('batch indices: a contiguous 1-d int64 CUDA tensor')
        return int(idx.numel()), idx.data_ptr()

    def grad(self, x, y, idx, x_scale, y_scale, loss_acc=None):
        n, ip = self._batch(x, y, idx)
        with torch.cuda.device(self.device):
            check(lib.qgx_ann_trainer_grad(self._h, x.data_ptr(), y.data_ptr(), ip, n, x_scale, y_scale,
                                           None if loss_acc is None else loss_acc.data_ptr(), _lib.current_stream_ptr()))

    def adam(self, lr):
        with torch.cuda.device(self.device):
            check(lib.qgx_ann_trainer_adam(self._h, lr, _lib.current_stream_ptr()))

    def step(self, x, y, idx, x_scale, y_scale, lr, loss_acc=None):
        n, ip = self._batch(x, y, idx)
        with torch.cuda.device(self.device):
            check(lib.qgx_ann_trainer_step(self._h, x.data_ptr(), y.data_ptr(), ip, n, x_scale, y_scale, lr,
                                           None if loss_acc is None else loss_acc.data_ptr(), _lib.current_stream_ptr()))

    def loss(self, x, y, idx, x_scale, y_scale, loss_acc):
        n, ip = self._batch(x, y, idx)
        with torch.cuda.device(self.device):
            check(lib.qgx_ann_trainer_loss(self._h, x.data_ptr(), y.data_ptr(), ip, n, x_scale, y_scale,
                                           loss_acc.data_ptr(), _lib.current_stream_ptr()))

    def read(self, what=_lib.TRAIN_PARAMS):
        out = np.empty(self.size, np.float32)
        check(lib.qgx_ann_trainer_read(self._h, int(what), out.ctypes.data))
        return out

    def write(self, what, values, adam_steps=-1):
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if v.size != self.size:
            raise ValueError(f'{v.size} values for a packed vector of {self.size}')
        check(lib.qgx_ann_trainer_write(self._h, int(what), v.ctypes.data, int(adam_steps)))

    def unpack(self, flat):
        """packed vector -> {state-dict key: array}"""
        out, o = {}, 0
        for key, shape in self.shapes:
            n = int(np.prod(shape))
            out[key] = np.asarray(flat[o:o + n]).reshape(shape).copy()
            o += n
        return out

    def state_dict(self):
        return {k: torch.from_numpy(v) for k, v in self.unpack(self.read(_lib.TRAIN_PARAMS)).items()}


def _images(ds, name):
    """stack_images (cnn_tools.py:360-371) of ds[name] with dims (run, time, lev, y, x): (n_img, N, N) float32 on the host"""
    v = stacked(ds, name, 'fit_ann')
    if v.shape[-1] != v.shape[-2]:
        raise ValueError(f'{name}: a {v.shape[-2]} x {v.shape[-1]} grid is not square')
    return np.ascontiguousarray(v.reshape((-1,) + v.shape[-2:]), dtype=np.float32)


def _check_datasets(ds):
    ds = list(ds) if isinstance(ds, (list, tuple)) else [ds]
    if not ds:
        raise ValueError('fit_ann: no dataset')
    return [(_images(d, 'q'), _images(d, 'q_forcing_advection')) for d in ds]


def device_rows(images, stencil_size, device):
    """prepare_data_ANN's X and Y (cnn_tools.py:373-389) of [(q images, forcing images), ...] on the device"""
    X, Y = [], []
    for q, f in images:
        if q.shape != f.shape:
            raise ValueError(f'q {q.shape} and q_forcing_advection {f.shape} differ in shape')
        X.append(ann_rows(torch.from_numpy(q).cuda(device), stencil_size, STEP))
        Y.append(ann_rows(torch.from_numpy(f).cuda(device), 1, STEP))
    return torch.cat(X).contiguous(), torch.cat(Y).contiguous()


def device_scales(X, Y, stencil_size):
    """x_scale, y_scale of prepare_data_ANN (cnn_tools.py:391-394): population stds in float64, cast to float32, as floats"""
    c = int(stencil_size) ** 2 // 2
    xs = X[:, c].to(torch.float64).std(unbiased=False).to(torch.float32)
    ys = Y.to(torch.float64).std(unbiased=False).to(torch.float32)
    return float(xs), float(ys)


def write_model_folder(folder, state_dict, x_scale, y_scale, stencil_size, hidden_channels, scale_invariant, log):
    """save_model (ann_model.py:54-66): net.pt (CPU float32 state dict), scale.json, model_args.json, stats.nc"""
    os.makedirs(folder, exist_ok=True)
    save_state_dict(os.path.join(folder, 'net.pt'), state_dict)
    with open(os.path.join(folder, 'scale.json'), 'w') as f:
        json.dump({'x_scale': float(x_scale), 'y_scale': float(y_scale)}, f)
    with open(os.path.join(folder, 'model_args.json'), 'w') as f:
        json.dump(dict(model='ANNModel', stencil_size=int(stencil_size), hidden_channels=[int(h) for h in hidden_channels],
                       scale_invariant=bool(scale_invariant)), f)
    write_log(os.path.join(folder, 'stats.nc'), log)


def fit_ann(ds_train, ds_test, *, stencil_size=3, hidden_channels=[24, 24], scale_invariant=False, folder='model',
            num_epochs=50, batch_size=2 ** 15, learning_rate=1e-3, seed=0, device=0, permutations=None, verbose=True):
    """Train ANNModel on the device and write its model folder; returns ANNModel(folder=folder) read from the files.

    ds_train, ds_test: a dataset or a list of datasets (of different resolutions) with q and q_forcing_advection of dims
    (run, time, lev, y, x).  permutations(epoch, n_rows), when given, returns the epoch's row order (an int64 array or
    tensor holding a permutation of 0 ... n_rows - 1) in place of torch.randperm seeded from `seed`."""
    from ..models.ann_model import ANNModel
    num_epochs, batch_size = int(num_epochs), int(batch_size)
    check_fit_args('fit_ann', num_epochs, batch_size, learning_rate)
    s, hidden = int(stencil_size), [int(h) for h in hidden_channels]
    train_img, test_img = _check_datasets(ds_train), _check_datasets(ds_test)
    net = _weights.synthetic_ann(s, hidden, bool(scale_invariant), seed)

    dev = cuda_device(device)
    with torch.cuda.device(dev):
        X, Y = device_rows(train_img, s, dev)
        Xt, Yt = device_rows(test_img, s, dev)
        x_scale, y_scale = device_scales(X, Y, s)
        R = int(X.shape[0])
        trainer = AnnTrainer(net, device=int(device))
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        lrs = learning_rates(num_epochs, learning_rate)
        acc = torch.zeros((num_epochs, 2, 2), dtype=torch.float64, device=dev)     # per epoch: train / test, (sum, rows)
        log = {}
        t_s = time()
        print_start(dev, R, verbose)
        for epoch in range(num_epochs):
            t_e = time()
            if permutations is None:
                order = torch.randperm(R, generator=gen, device=dev)
            else:
                order = torch.as_tensor(permutations(epoch, R)).to(device=dev, dtype=torch.int64).contiguous()
                if order.numel() != R or int(order.min()) < 0 or int(order.max()) >= R:
                    raise ValueError(f'permutations({epoch}, {R}) is no order of the {R} rows')
            for b0 in range(0, R, batch_size):
                trainer.step(X, Y, order[b0:b0 + batch_size], x_scale, y_scale, lrs[epoch], acc[epoch, 0])
            trainer.loss(Xt, Yt, None, x_scale, y_scale, acc[epoch, 1])
            log_epoch(log, acc[epoch].cpu().numpy(), epoch, num_epochs, t_e, t_s, verbose)      # the epoch's one host read
        if verbose:
            print(f'training took {time() - t_s:.2f} seconds')
        sd = trainer.state_dict()
        trainer.close()
    write_model_folder(folder, sd, x_scale, y_scale, s, hidden, scale_invariant, log)
    return ANNModel(scale_invariant=bool(scale_invariant), stencil_size=s, hidden_channels=hidden, folder=folder, device=device)


def main(argv=None):
    return command_line('train ANNModel on the device and write its model folder', {'ANNModel': fit_ann}, argv,
                        several=True, ignore=('read',))


if __name__ == '__main__':
    main()
