"""Online metrics of a run against a reference run, and the statistics of a run, computed on the GPU (reference:
pyqg_generative/tools/comparison_tools.py:16-54 DISTRIB_KEYS / SPECTRAL_KEYS / distrib_score / spectral_score, :56-115
coarsegrain_reference_dataset, :116-195 diagnostic_differences_Perezhogin, :197-271 dataset_statistics, :273-410
cache_path / dataset_smart_read, :412-436 the command line).

The distributional errors are 1-Wasserstein distances between the pooled values (runs x last T snapshots x space) of
q, u, v, KE = u^2 + v^2 and Ens = curl(u, v)^2 per layer.  They are exact — the value of
``scipy.stats.wasserstein_distance`` — and deterministic, and run in libqgx.so: a key pass over the strided snapshots,
a radix sort of both samples and a merge-path sum (csrc/metrics.hip; qgx_w1_keys / qgx_w1_sorted).  The curl is
spectral on the fields' own grid (qgx_rfft2, qgx_spec_curl, qgx_irfft2).  The spectral errors bin a few thousand
time-averaged numbers per dataset and stay in host numpy (tools/spectral_tools.py::calc_ispec).

The derived flow fields of dataset_statistics / dataset_smart_read — omega = curl(u, v), KE, Ens, Vabs and the plane sums
behind KE_time — come from ONE entry point, qgx_flow_features (csrc/flow.hip): u and v are read once.  Their PDFs are
qgx_histogram counts of the device arrays; the isotropic spectra of the sixteen time-averaged diagnostics are host numpy.

Datasets are those of ``run_simulation`` / ``concat_in_time`` on either backend (xarray or tools/xr_lite.py), with or
without a 'run' dimension; files are read through the backend (xr_lite reads the classic netCDF its ``to_netcdf`` writes).
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from .. import _lib
from .._lib import lib, check
from ..engine import _ptr, _stream
from .operators import Dev, ave_lev
from .parameters import AVERAGE_SLICE_ANDREW
from .simulate import dataset_backend
from .spectral_tools import _Grid, calc_ispec, twothirds_nyquist

DISTRIB_KEYS = [
    'distrib_diff_q1',
    'distrib_diff_q2',
    'distrib_diff_u1',
    'distrib_diff_u2',
    'distrib_diff_v1',
    'distrib_diff_v2',
    'distrib_diff_KE1',
    'distrib_diff_KE2',
    'distrib_diff_Ens1',
    'distrib_diff_Ens2'
]

SPECTRAL_KEYS = [
    'spectral_diff_KEspec1',
    'spectral_diff_KEspec2',
    'spectral_diff_KEflux',
    'spectral_diff_APEflux',
    'spectral_diff_APEgenspec',
    'spectral_diff_KEfrictionspec',
    'spectral_diff_Eflux'
]

CHUNK = 512      # fields per transform in the curl and the coarse-graining operators
SPECTRA = ['KEspec', 'KEflux', 'APEflux', 'APEgenspec', 'KEfrictionspec']


def distrib_score(similarity_instance):
    l = [v for k, v in similarity_instance.items() if k in DISTRIB_KEYS]
    return np.mean(l) if len(l) > 0 else np.nan


def spectral_score(similarity_instance):
    l = [v for k, v in similarity_instance.items() if k in SPECTRAL_KEYS]
    return np.mean(l) if len(l) > 0 else np.nan


# ---- the exact 1-Wasserstein distance ---------------------------------------------------------------------------
class _Sample:
    """keys of one sample (qgx_w1_keys) and its statistics [sum of feature^2, non-finite count], on the device"""

    def __init__(self, x, y, feature, key_bits, R, T, P, stride_r, stride_t, offset=0):
        self.n, self.key_bits, dev = R * T * P, key_bits, x.device
        self.keys = torch.empty(self.n, dtype=torch.int32 if key_bits == 32 else torch.int64, device=dev)
        self.stats = torch.empty(2, dtype=torch.float64, device=dev)
        partials = torch.empty(2 * _lib.W1_PARTIALS, dtype=torch.float64, device=dev)
        off = offset * x.element_size()
        check(lib.qgx_w1_keys(C.c_void_p(x.data_ptr() + off), C.c_void_p(y.data_ptr() + off if y is not None else 0),
                              int(x.dtype == torch.float64), feature, key_bits, R, T, P, stride_r, stride_t,
                              _ptr(self.keys), _ptr(partials), _ptr(self.stats), _stream()))

    def scale(self):
        """sqrt(mean(feature^2)): the reference's normalisation"""
        return float(np.sqrt(self.stats[0].item() / self.n))


def _w1(a, b):
    """W1 of two _Samples (their keys are sorted in place) -> 0-d float64 device tensor"""
    nbytes = C.c_size_t()
    check(lib.qgx_w1_workspace(a.n, b.n, a.key_bits, C.byref(nbytes)))
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=a.keys.device)
    out = torch.empty(1, dtype=torch.float64, device=a.keys.device)
    check(lib.qgx_w1_sorted(_ptr(a.keys), a.n, _ptr(a.stats), _ptr(b.keys), b.n, _ptr(b.stats), a.key_bits,
                            _ptr(work), nbytes.value, _ptr(out), _stream()))
    return out[0]


def _flat_device(x, device):
    """-> flat float32 / float64 tensor on the GPU; device tensors stay where they are"""
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(f'cuda:{device}')
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(f'cuda:{device}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.reshape(-1)


def wasserstein_distance(u_values, v_values, device=0):
    """scipy.stats.wasserstein_distance(u_values, v_values) (unweighted) on the GPU: numpy arrays or torch tensors of
    any shape, flattened.  Exact, and bitwise the same for every order of either input.  NaN if either holds a NaN or
    an infinity.  -> float"""
    for x in (u_values, v_values):
        if (x.numel() if isinstance(x, torch.Tensor) else np.size(x)) == 0:
            raise ValueError('Distribution can\'t be empty.')
    u = _flat_device(u_values, device)
    v = _flat_device(v_values, u.device.index)
    if v.device != u.device:
        v = v.to(u.device)
    with torch.cuda.device(u.device):
        bits = 32 if u.dtype == v.dtype == torch.float32 else 64
        a = _Sample(u, None, _lib.W1_IDENTITY, bits, 1, 1, u.numel(), 0, 0)
        b = _Sample(v, None, _lib.W1_IDENTITY, bits, 1, 1, v.numel(), 0, 0)
        return float(_w1(a, b).item())


# ---- datasets -----------------------------------------------------------------------------------------------------
def _spatial(da):
    """DataArray (run, time, lev, y, x) in that order -> numpy"""
    return np.asarray(da.transpose('run', 'time', 'lev', 'y', 'x').values)


class _Snapshots:
    """q, u, v of the last T snapshots of a dataset with a 'run' dimension, (R, T, 2, N, N) on the device as stored"""

    def __init__(self, ds, T, device):
        self.f = {}
        for name in ('q', 'u', 'v'):
            a = _spatial(ds[name])[:, -T:]
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float64)
            self.f[name] = torch.from_numpy(np.ascontiguousarray(a)).to(f'cuda:{device}')
        self.R, self.T, _, self.N, _ = self.f['q'].shape

    def view(self, z):
        """(R, T, P, stride_r, stride_t, offset) of layer z"""
        P = self.N * self.N
        return self.R, self.T, P, self.T * 2 * P, 2 * P, z * P

    def sample(self, label, z, key_bits):
        if label in ('q', 'u', 'v'):
            return _Sample(self.f[label], None, _lib.W1_IDENTITY, key_bits, *self.view(z))
        if label == 'KE':
            return _Sample(self.f['u'], self.f['v'], _lib.W1_SUMSQ2, 64, *self.view(z))
        c = self.curl(z)
        return _Sample(c, None, _lib.W1_SQUARE, 64, 1, 1, c.numel(), 0, 0)

    def curl(self, z):
        """curl(u, v) = ddx(v) - ddy(u) of layer z, spectral on the fields' grid: (R*T, N, N) float64"""
        N = self.N
        u, v = (self.f[k].reshape(-1, 2, N, N) for k in ('u', 'v'))
        out = torch.empty((u.shape[0], N, N), dtype=torch.float64, device=u.device)
        for s in range(0, u.shape[0], CHUNK):
            uh = Dev.rfft2(u[s:s + CHUNK, z].to(torch.float64).contiguous())
            vh = Dev.rfft2(v[s:s + CHUNK, z].to(torch.float64).contiguous())
            ch = torch.empty_like(uh)
            check(lib.qgx_spec_curl(_ptr(uh), _ptr(vh), _ptr(ch), ch.shape[0], N, Dev.L, _stream()))
            out[s:s + CHUNK] = Dev.irfft2(ch)
        return out


def _spectral_rmse(spec1, spec2):
    spec1, spec2 = np.asarray(spec1), np.asarray(spec2)
    m1, m2 = _Grid(spec1.shape[-2]), _Grid(spec2.shape[-2])
    kr1, ispec1 = calc_ispec(m1, spec1)
    kr2, ispec2 = calc_ispec(m2, spec2)
    kmax = min(twothirds_nyquist(m1), twothirds_nyquist(m2))
    nk = (kr1 < kmax).sum()
    return np.sqrt(np.mean((ispec1[:nk].astype('float64') - ispec2[:nk].astype('float64')) ** 2)), \
        np.sqrt(np.mean((ispec2[:nk].astype('float64')) ** 2))


def diagnostic_differences_Perezhogin(ds1, ds2, T=128, device=0):
    """Distributional and spectral differences of ds1 from the target ds2, normalised by ds2's scales.
    -> (normalized_differences, differences, scales), dicts keyed as in the reference"""
    if 'run' not in ds1.dims:
        ds1 = ds1.expand_dims('run')
    if 'run' not in ds2.dims:
        ds2 = ds2.expand_dims('run')

    differences, scales = {}, {}
    with torch.cuda.device(device):
        s1, s2 = _Snapshots(ds1, T, device), _Snapshots(ds2, T, device)
        bits = 32 if s1.f['q'].dtype == s2.f['q'].dtype == torch.float32 else 64
        for label in ('q', 'u', 'v', 'KE', 'Ens'):
            for z in (0, 1):
                a, b = s1.sample(label, z, bits), s2.sample(label, z, bits)
                key = f'distrib_diff_{label}{z + 1}'
                differences[key] = float(_w1(a, b).item())
                scales[key] = b.scale()
                del a, b
        del s1, s2

    for spec in ['KEspec']:
        for z in [0, 1]:
            spec1 = ds1[spec].isel(lev=z).mean('run').values
            spec2 = ds2[spec].isel(lev=z).mean('run').values
            differences[f'spectral_diff_{spec}{z + 1}'], scales[f'spectral_diff_{spec}{z + 1}'] = \
                _spectral_rmse(spec1, spec2)

    def compute_Eflux(ds):
        out = 0
        for spec in ['KEflux', 'APEflux', 'paramspec_KEflux', 'paramspec_APEflux']:
            if spec in ds.data_vars:
                out = out + np.asarray(ds[spec].mean('run').values)
        return out

    differences['spectral_diff_Eflux'], scales['spectral_diff_Eflux'] = \
        _spectral_rmse(compute_Eflux(ds1), compute_Eflux(ds2))
    differences['spectral_diff_APEgenspec'], scales['spectral_diff_APEgenspec'] = \
        _spectral_rmse(ds1['APEgenspec'].mean('run').values, ds2['APEgenspec'].mean('run').values)

    normalized_differences = {key: differences[key] / scales[key] for key in differences}
    return normalized_differences, differences, scales


# ---- coarse-grained reference -------------------------------------------------------------------------------------
_OPERATORS = {'Operator1': Dev.Operator1, 'Operator2': Dev.Operator2, 'Operator4': Dev.Operator4,
              'Operator5': Dev.Operator5}


def coarsegrain_spectrum(array, resolution, operator):
    """a spectral statistic (..., N, N/2+1) of a high-resolution run on the coarse grid's (l, k) half plane, times the
    squared transfer function of the filter: filtr^2 for Operator1, the Gaussian of width 2 dx squared for Operator2,
    nothing for Operator4 / Operator5 (comparison_tools.py:89-114)"""
    if operator not in _OPERATORS:
        raise ValueError('operator must be Operator1 or Operator2')
    n = resolution // 2
    a = np.asarray(array)
    out = np.concatenate((a[..., :n, :n + 1], a[..., -n:, :n + 1]), axis=-2)
    m = _Grid(resolution)
    if operator == 'Operator1':
        out = out * m.filtr * m.filtr
    elif operator == 'Operator2':
        filtr = np.exp(-(m.k ** 2 + m.l ** 2) * (2 * m.dx) ** 2 / 24)
        out = out * filtr * filtr
    return out


def coarsegrain_reference_dataset(ds, resolution, operator, device=0):
    """Snapshots q, u, v, psi of a high-resolution dataset through the coarse-graining operator on the GPU, and its
    spectra KEspec, KEflux, APEflux, APEgenspec, KEfrictionspec through coarsegrain_spectrum.
    operator: 'Operator1', 'Operator2', 'Operator4' or 'Operator5'"""
    if operator not in _OPERATORS:
        raise ValueError('operator must be Operator1 or Operator2')
    op = _OPERATORS[operator]
    xr = dataset_backend()
    if 'run' not in ds.dims:
        ds = ds.expand_dims('run')
    dsf = xr.Dataset()
    with torch.cuda.device(device):
        for var in ['q', 'u', 'v', 'psi']:
            da = ds[var]
            a = np.asarray(da.values)
            flat = a.reshape((-1,) + a.shape[-2:])
            out = np.empty((flat.shape[0], resolution, resolution))
            for s in range(0, flat.shape[0], CHUNK):
                x = torch.from_numpy(np.ascontiguousarray(flat[s:s + CHUNK], dtype=np.float64)).to(f'cuda:{device}')
                out[s:s + CHUNK] = op(x, resolution).cpu().numpy()
            dsf[var] = xr.DataArray(out.reshape(a.shape[:-2] + (resolution, resolution)), dims=da.dims)

    for var in SPECTRA:
        a = np.asarray(ds[var].values)
        if a.ndim == 3:
            dims = ['run', 'l', 'k']
        elif a.ndim == 4:
            dims = ['run', 'lev', 'l', 'k']
        else:
            raise ValueError('var must be 3 or 4 dimensional')
        dsf[var] = xr.DataArray(coarsegrain_spectrum(a, resolution, operator), dims=dims)
    m = _Grid(resolution)
    dsf['k'] = xr.DataArray(m.kk, dims=['k'])
    dsf['l'] = xr.DataArray(m.ll, dims=['l'])
    return dsf


# ---- the derived flow fields --------------------------------------------------------------------------------------
FLOW_FEATURES = ('omega', 'KE', 'Ens', 'Vabs', 'KE_sum')
DIAGNOSTICS = ['APEflux', 'APEgenspec', 'Dissspec', 'ENSDissspec', 'ENSflux', 'ENSfrictionspec', 'ENSgenspec',
               'ENSparamspec', 'Ensspec', 'KEflux', 'KEfrictionspec', 'KEspec', 'entspec', 'paramspec', 'paramspec_APEflux',
               'paramspec_KEflux']
_LARGE_PLAN_POINTS = 1 << 21     # grid points per chunk of the batched path: 32 planes at 256 x 256


def _field_device(x, device):
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(f'cuda:{device}')
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(f'cuda:{device}')
    return t.contiguous()


def flow_features(u, v, device=0, want=FLOW_FEATURES):
    """The derived fields of velocity snapshots u, v (..., 2, N, N): numpy arrays or torch tensors, float32 or float64 (a
    pair of different dtypes is promoted to float64).  -> dict of device tensors, the names in ``want``:
      'omega'  (..., 2, N, N) float64      curl(u, v) = ddx(v) - ddy(u), spectral on the fields' grid
      'KE'     (..., 2, N, N) input dtype  (u^2 + v^2) / 2
      'Ens'    (..., 2, N, N) float64      omega^2 / 2
      'Vabs'   (..., 2, N, N) input dtype  sqrt(u^2 + v^2)
      'KE_sum' (..., 2)       float64      the sum of KE over each plane, of the float64 values
    All arithmetic is float64, in one pass over u and v (qgx_flow_features); a name left out is not computed.  KE and Ens
    carry the factor 1/2 that the features of diagnostic_differences_Perezhogin do not."""
    want = tuple(want)
    unknown = [w for w in want if w not in FLOW_FEATURES]
    if unknown or not want:
        raise ValueError(f'flow_features: want must name some of {FLOW_FEATURES}, got {want}')
    ud = _field_device(u, device)
    vd = _field_device(v, ud.device.index)
    if ud.shape != vd.shape or ud.dim() < 3 or ud.shape[-3] != 2 or ud.shape[-1] != ud.shape[-2]:
        raise ValueError(f'flow_features needs u, v of one shape (..., 2, N, N), got {tuple(ud.shape)} and {tuple(vd.shape)}')
    if ud.dtype != vd.dtype or ud.dtype not in (torch.float32, torch.float64):
        ud, vd = ud.to(torch.float64), vd.to(torch.float64)
    if ud.numel() == 0:
        raise ValueError('flow_features of empty fields')
    N, lead = ud.shape[-1], tuple(ud.shape[:-3])
    S = ud.numel() // (2 * N * N)
    dev = ud.device
    with torch.cuda.device(dev):
        members = 1 if N <= 96 else max(1, min(2 * S, _LARGE_PLAN_POINTS // (N * N)))
        plan = Dev.plan(N, 2 * members, dev.index)
        out = {}
        for name in want:
            shape = lead + ((2,) if name == 'KE_sum' else (2, N, N))
            out[name] = torch.empty(shape, dtype=ud.dtype if name in ('KE', 'Vabs') else torch.float64, device=dev)
        nbytes = C.c_size_t()
        check(lib.qgx_flow_features_workspace(plan._h, S, C.byref(nbytes)))
        work = torch.empty(nbytes.value, dtype=torch.uint8, device=dev) if nbytes.value else None
        check(lib.qgx_flow_features(plan._h, _ptr(ud), _ptr(vd), int(ud.dtype == torch.float64), S, _ptr(out.get('omega')),
                                    _ptr(out.get('KE')), _ptr(out.get('Ens')), _ptr(out.get('Vabs')), _ptr(out.get('KE_sum')),
                                    _ptr(work), nbytes.value, _stream()))
    return out


# ---- dataset_statistics / dataset_smart_read ------------------------------------------------------------------------
def _coord(xr, x, name):
    return xr.DataArray(x, attrs={'long_name': name})


def _years(ds):
    """time in days -> years, as the reference does it: its test looks for the KEY 'years' among the attributes, which no
    dataset has, so the division is always made"""
    if 'years' not in ds['time'].attrs:
        t = ds['time'] / 360
        t.attrs = {'long_name': 'time [$years$]'}
        ds['time'] = t
    return ds


_CANON = ('run', 'time', 'lev', 'y', 'x')


def _canonical(ds, name):
    """-> (values (R, T, 2, N, N) as stored, with axes of length one for a missing run / time; the order of dims they
    are in; the variable's own dims)"""
    da = ds[name]
    order = [d for d in _CANON if d in da.dims]
    if len(order) != len(da.dims) or order[-3:] != ['lev', 'y', 'x']:
        raise ValueError(f'{name} has dims {tuple(da.dims)}; expected ([run,] [time,] lev, y, x) in some order')
    a = np.asarray(da.transpose(*order).values)
    return a.reshape([a.shape[order.index(d)] if d in order else 1 for d in _CANON]), order, tuple(da.dims)


def _like_q(xr, t, order, dims):
    """device tensor (R, T, 2, N, N) -> DataArray with the dims of q"""
    a = t.cpu().numpy()
    a = a.reshape([n for n, d in zip(a.shape, _CANON) if d in order])
    return xr.DataArray(a, dims=order).transpose(*dims)


def _ispec_statistics(xr, ds, stats, delta, **kw_ispec):
    """the isotropic spectra ...r / ...r_mean of the time-averaged diagnostics, Energysumr and Efluxr"""
    m = _Grid(len(ds['x']))
    for key in DIAGNOSTICS:
        if key not in ds.keys():
            continue
        var = ds[key].astype('float64')      # (the run mean of the stored float32 spectra in float64; the reference's is float32)
        if 'run' in var.dims:
            var = var.mean(dim='run')
        if 'lev' in var.dims:
            sps = []
            for z in [0, 1]:
                k, sp = calc_ispec(m, np.asarray(var.isel(lev=z).values), **kw_ispec)
                sps.append(sp)
            sp = np.stack(sps, axis=0)
            stats[key + 'r'] = xr.DataArray(sp, dims=['lev', 'kr'], coords=[[1, 2], _coord(xr, k, 'wavenumber, $m^{-1}$')])
            var_mean = ave_lev(var, delta)
            k, sp = calc_ispec(m, np.asarray(var_mean), **kw_ispec)
            stats[key + 'r_mean'] = xr.DataArray(sp, dims=['kr'], coords=[_coord(xr, k, 'wavenumber, $m^{-1}$')])
        else:
            k, sp = calc_ispec(m, np.asarray(var.values), **kw_ispec)
            stats[key + 'r'] = xr.DataArray(sp, dims=['kr'], coords=[_coord(xr, k, 'wavenumber, $m^{-1}$')])

    budget_sum = 0
    for key in ['KEfluxr', 'APEfluxr', 'APEgenspecr', 'KEfrictionspecr', 'paramspec_APEfluxr', 'paramspec_KEfluxr']:
        if key in stats.keys():
            budget_sum = budget_sum + stats[key]
    stats['Energysumr'] = budget_sum

    Eflux = 0
    for key in ['KEfluxr', 'APEfluxr', 'paramspec_KEfluxr', 'paramspec_APEfluxr']:
        if key in stats.keys():
            Eflux = Eflux + stats[key]
    stats['Efluxr'] = Eflux


def _ke_time(xr, ds, ke_sum, delta, N):
    """ave_lev(KE, delta).mean(([run,] x, y)) from the plane sums (R, T, 2) of the device: the layer weights and the
    division by R N^2 are all that runs here"""
    w = np.array([delta / (1 + delta), 1 / (1 + delta)])
    s = ke_sum.cpu().numpy()
    values = (s.sum(axis=0) * w).sum(axis=-1) / (s.shape[0] * N * N)
    return xr.DataArray(values, dims=['time'], coords=[ds['time']])


def dataset_statistics(ds, delta=0.25, device=0, **kw_ispec):
    """If a path (a glob pattern) is given, the dataset is returned as is, its files concatenated along 'run' and time in
    years.  If a dataset is given — with or without a 'run' dimension — its statistics are computed:
      <diagnostic>r [, <diagnostic>r_mean]   isotropic spectra of the run-mean time-averaged diagnostics (calc_ispec with
                                             **kw_ispec): per layer (lev, kr) and of the depth average (kr), or (kr) alone
      Energysumr, Efluxr                     the energy budget's sum and the total spectral energy flux
      KE_time (time)                         depth-, run- and area-mean kinetic energy; time in years
    (reference: comparison_tools.py:197-271)"""
    xr = dataset_backend()
    if isinstance(ds, str):
        return _years(xr.open_mfdataset(ds, combine='nested', concat_dim='run', decode_times=False))
    stats = xr.Dataset()
    _ispec_statistics(xr, ds, stats, delta, **kw_ispec)
    u, _, _ = _canonical(ds, 'u')
    v, _, _ = _canonical(ds, 'v')
    f = flow_features(u, v, device, want=('KE_sum',))
    stats['KE_time'] = _ke_time(xr, ds, f['KE_sum'], delta, u.shape[-1])
    return _years(stats)


def cache_path(path):
    dir = os.path.dirname(path)
    files = os.path.basename(path)
    cachename = files.encode('utf-8').hex() + '.cache_netcdf'
    return os.path.join(dir, cachename)


_PDF_XMAX = {('Ens', 0): 1e-10, ('Ens', 1): 1.5e-12, ('KE', 0): 1.5e-2, ('KE', 1): 5e-4}


def _smart_statistics(xr, ds, delta, compute_all, device):
    from .computational_tools import PDF_histogram
    stats = xr.Dataset()
    fields = {name: _canonical(ds, name) for name in ('q', 'u', 'v')}
    _, order, dims = fields['q']
    T = fields['q'][0].shape[1]
    # the PDFs' time window: AVERAGE_SLICE_ANDREW, or the last snapshot alone
    t0 = AVERAGE_SLICE_ANDREW.indices(T)[0] if compute_all else max(T - 1, 0)
    with torch.cuda.device(device):
        dev = {name: _field_device(a if compute_all or name == 'q' else a[:, -1:], device) for name, (a, _, _) in fields.items()}
        f = flow_features(dev['u'], dev['v'], device, want=FLOW_FEATURES if compute_all else ('KE',))
        if compute_all:
            for name in ('omega', 'KE', 'Ens', 'Vabs'):
                stats[name] = _like_q(xr, f[name], order, dims)
            ke_sum = f['KE_sum']
        else:
            ke_sum = flow_features(fields['u'][0], fields['v'][0], device, want=('KE_sum',))['KE_sum']
        for var in ['q', 'u', 'v', 'KE', 'Ens'] if compute_all else ['q', 'u', 'v', 'KE']:
            x = f[var] if var in f else dev[var]
            first = t0 if x.shape[1] == T else 0          # (compute_all=False: u, v and KE hold the last snapshot only)
            for lev in [0, 1]:
                values = x[:, first:, lev].contiguous()
                if values.numel() == 0:
                    raise ValueError(f'dataset_smart_read: no snapshot at time index >= {t0} for the PDFs')
                xmin = 0 if var in ['KE', 'Ens'] else None
                points, density = PDF_histogram(values, xmin=xmin, xmax=_PDF_XMAX.get((var, lev)))
                stats[f'PDF_{var}{lev + 1}'] = xr.DataArray(density, dims=f'{var}_{lev}', coords=[points])
    _ispec_statistics(xr, ds, stats, delta)
    stats['KE_time'] = _ke_time(xr, ds, ke_sum, delta, fields['u'][0].shape[-1])
    return stats


def dataset_smart_read(path, delta=0.25, read_cache=True, compute_all=True, device=0):
    """The files of ``path`` (a glob pattern) concatenated along 'run', time in years, merged with their statistics:
      omega, KE, Ens, Vabs                   with the dims of q (compute_all only)
      PDF_{q,u,v,KE,Ens}{1,2}                30-bin densities per layer over time index >= 44 on dimension {var}_{lev}: q, u, v
                                             over mean -+ 4 sigma, KE and Ens from 0 to a fixed maximum per layer
                                             (compute_all=False: q, u, v, KE of the last snapshot alone)
      the spectra of dataset_statistics, Energysumr, Efluxr, KE_time
    The statistics are cached beside the files (cache_path): read from there unless read_cache is False, which deletes the
    cache and computes them anew.  A dataset in place of a path is used as it is (with or without 'run', its time
    coordinate untouched); nothing is read or cached.  (reference: comparison_tools.py:273-410)"""
    xr = dataset_backend()
    if not isinstance(path, str):
        return xr.merge([path, _smart_statistics(xr, path, delta, compute_all, device)])
    cache = cache_path(path)
    if os.path.exists(cache) and read_cache:
        ds1 = xr.open_mfdataset(path, combine='nested', concat_dim='run', decode_times=False)
        ds2 = xr.open_dataset(cache)
        t = ds1['time'] / 360
        t.attrs = {'long_name': 'time [$years$]'}
        ds1['time'] = t
        ds2['time'] = ds1['time']       # make sure time is the same
        return xr.merge([ds1, ds2])
    if os.path.exists(cache) and not read_cache:
        os.remove(cache)

    ds = xr.open_mfdataset(path, combine='nested', concat_dim='run', decode_times=False)
    t = ds['time'] / 360
    t.attrs = {'long_name': 'time [$years$]'}
    ds['time'] = t
    stats = _smart_statistics(xr, ds, delta, compute_all, device)
    stats.to_netcdf(cache)
    return xr.merge([ds, stats])


# ---- command line ---------------------------------------------------------------------------------------------------
def main(argv=None):
    """--model_path (a glob pattern: one file per run) --target_path --save_file --key: the normalised differences of the
    model's runs from the target, with the key, as JSON (reference: comparison_tools.py:412-436)"""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--model_path', type=str)
    parser.add_argument('--target_path', type=str)
    parser.add_argument('--save_file', type=str)
    parser.add_argument('--key', type=str)
    args = parser.parse_args(argv)
    print(args)

    xr = dataset_backend()
    model = xr.open_mfdataset(args.model_path, combine='nested', concat_dim='run')
    print('model loaded')
    target = xr.open_dataset(args.target_path)
    print('target loaded')
    difference, _, _ = diagnostic_differences_Perezhogin(model, target, T=128)
    print('difference calculated')
    difference['key'] = args.key
    with open(args.save_file, 'w') as file:
        json.dump(difference, file)
    print('json file closed')
    return difference


if __name__ == '__main__':
    main()
