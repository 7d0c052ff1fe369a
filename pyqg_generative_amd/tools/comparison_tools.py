"""Online metrics of a run against a reference run, computed on the GPU (reference: pyqg_generative/tools/
comparison_tools.py:16-54 DISTRIB_KEYS / SPECTRAL_KEYS / distrib_score / spectral_score, :56-115
coarsegrain_reference_dataset, :116-195 diagnostic_differences_Perezhogin).

The distributional errors are 1-Wasserstein distances between the pooled values (runs x last T snapshots x space) of
q, u, v, KE = u^2 + v^2 and Ens = curl(u, v)^2 per layer.  They are exact — the value of
``scipy.stats.wasserstein_distance`` — and deterministic, and run in libqgx.so: a key pass over the strided snapshots,
a radix sort of both samples and a merge-path sum (csrc/metrics.hip; qgx_w1_keys / qgx_w1_sorted).  The curl is
spectral on the fields' own grid (qgx_rfft2, qgx_spec_curl, qgx_irfft2).  The spectral errors bin a few thousand
time-averaged numbers per dataset and stay in host numpy (tools/spectral_tools.py::calc_ispec).

Datasets are those of ``run_simulation`` / ``concat_in_time`` on either backend (xarray or tools/xr_lite.py), with or
without a 'run' dimension.  The reference module's file-reading command line (comparison_tools.py:412-436) is not
provided.
"""
import ctypes as C
import numpy as np
import torch

from .. import _lib
from .._lib import lib, check
from ..engine import _ptr, _stream
from .operators import Dev
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
