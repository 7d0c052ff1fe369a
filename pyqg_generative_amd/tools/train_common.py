"""What every fit_* of tools/train_ANN.py and tools/train_CNN.py shares: the checks of the fit arguments, the reference's
learning-rate schedule, the extraction of a dataset's variable, the device argument, the files of a model folder that do
not depend on the model (state dicts, stats*.nc), the per-epoch log and progress line, and the command line.  A new fit_*
adds a net, a loss and a folder writer to its own module; nothing here knows a model.
"""
import math
import os
from time import time

import numpy as np
import torch

DIMS = ('run', 'time', 'lev', 'y', 'x')


def check_fit_args(who, num_epochs, batch_size, learning_rate):
    if batch_size < 1:
        raise ValueError(f'{who}: batch_size = {batch_size}')
    if num_epochs < 1:
        raise ValueError(f'{who}: num_epochs = {num_epochs}')
    if not (math.isfinite(learning_rate) and learning_rate >= 0):
        raise ValueError(f'{who}: learning_rate = {learning_rate}')


def learning_rates(num_epochs, learning_rate):
    """the learning rate of every epoch under train()'s schedule (cnn_tools.py:670-672, :692): MultiStepLR with milestones
    int(E / 2), int(3 E / 4), int(7 E / 8), gamma 0.1, stepped after each epoch — torch's class on a dummy optimizer, so that
    repeated and zero milestones of a small E behave as torch's do"""
    E = int(num_epochs)
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=float(learning_rate))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[int(E / 2), int(E * 3 / 4), int(E * 7 / 8)], gamma=0.1)
    out = []
    for _ in range(E):
        out.append(float(opt.param_groups[0]['lr']))
        opt.step()
        sched.step()
    return out


def stacked(ds, key, who):
    """the values of ds[key] as (run, time, lev, y, x), whatever the order of its dims; `who` is the fit that asks"""
    if key not in ds:
        raise ValueError(f'{who} needs {key!r} in every dataset')
    a = ds[key]
    dims = tuple(a.dims)
    if dims != DIMS:
        if set(dims) != set(DIMS):
            raise ValueError(f'{key}: dims {dims}, expected (run, time, lev, y, x)')
        a = a.transpose(*DIMS)
    return np.asarray(a.values)


def cuda_device(device):
    """an index or a torch.device -> torch.device"""
    return device if isinstance(device, torch.device) else torch.device('cuda', int(device))


def save_state_dict(path, state_dict):
    """torch.save of a detached CPU copy; values that are no tensors (the ANN trainer's numpy arrays) are stored as float32"""
    torch.save({k: v.detach().cpu().clone() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32)).clone()
                for k, v in state_dict.items()}, path)


def write_log(path, log):
    """log_to_xarray(log).to_netcdf(path): one variable per key over `epoch`; a file already there is replaced"""
    from .simulate import dataset_backend
    xr = dataset_backend()
    E = len(next(iter(log.values())))
    stats = xr.Dataset({k: (['epoch'], np.asarray(v, dtype=np.float64)) for k, v in log.items()},
                       coords={'epoch': np.arange(1, E + 1)})
    if os.path.exists(path):
        os.remove(path)
    stats.to_netcdf(path)


def print_start(dev, n, verbose):
    if verbose:
        print(f'Training starts on device {torch.cuda.get_device_name(dev)}, number of samples {n}')


def log_epoch(log, a, epoch, E, t_e, t_s, verbose):
    """a (2, 2) float64 on the host, [train, test] x [sum of loss * n, n] of epoch `epoch` of E, which began at t_e (the fit
    at t_s): the means are appended to log['loss'] and log['loss_test'], and the reference's progress line is printed"""
    log.setdefault('loss', []).append(float(a[0, 0] / a[0, 1]))
    log.setdefault('loss_test', []).append(float(a[1, 0] / a[1, 1]))
    if verbose:
        t = time()
        print('[%d/%d] [%.2f/%.2f] Loss: [%.3f, %.3f]' % (epoch + 1, E, t - t_e, (t - t_s) * (E / (epoch + 1) - 1),
                                                          log['loss'][-1], log['loss_test'][-1]))


def open_datasets(pattern, several):
    """the netCDF files of a glob, concatenated along run; with `several`, a list of them, one per comma-separated glob"""
    from .simulate import dataset_backend
    xr = dataset_backend()
    one = lambda p: xr.open_mfdataset(p.strip(), combine='nested', concat_dim='run')
    return [one(p) for p in pattern.split(',') if p.strip()] if several else one(pattern)


def command_line(description, fit_of, argv, several=False, ignore=()):
    """The command line of a training module.  fit_of: {model name: fit(ds_train, ds_test, **model_args, **fit_args)}; with
    more than one, --model chooses (default: the first).  several: comma-separated globs are several datasets, handed to the
    fit as lists, and --test writes offline-<k>.nc per test dataset in place of offline.nc.  ignore: keys of --model_args
    that the reference's constructor takes and a fit does not.  Returns the fitted model."""
    import argparse
    import ast
    names = list(fit_of)
    many = '; several, comma-separated: several datasets' if several else ''
    parser = argparse.ArgumentParser(description=description)
    if len(names) > 1:
        parser.add_argument('--model', type=str, default=names[0], choices=names)
    parser.add_argument('--train', type=str, required=True, help='glob of training files, concatenated along run' + many)
    parser.add_argument('--validate', type=str, required=True)
    parser.add_argument('--test', type=str, default=None, help='glob of files for test_offline' + many)
    parser.add_argument('--model_args', type=str, default=str({}))
    parser.add_argument('--fit_args', type=str, default=str({}))
    args = parser.parse_args(argv)
    print(args)
    model_args, fit_args = ast.literal_eval(args.model_args), ast.literal_eval(args.fit_args)
    if not isinstance(model_args, dict) or not isinstance(fit_args, dict):
        raise ValueError('--model_args and --fit_args are dict literals')
    for key in ignore:
        model_args.pop(key, None)
    fit = fit_of[args.model if len(names) > 1 else names[0]]
    model = fit(open_datasets(args.train, several), open_datasets(args.validate, several), **model_args, **fit_args)
    if args.test:
        sets = open_datasets(args.test, several)
        for name, ds in ([(f'offline-{k}.nc', d) for k, d in enumerate(sets)] if several else [('offline.nc', sets)]):
            model.test_offline(ds).to_netcdf(os.path.join(model.folder, name))
    return model
