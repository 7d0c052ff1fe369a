"""Offline metrics of a parameterization, computed on the GPU (reference: pyqg_generative/tools/computational_tools.py:5-36
PDF_histogram, :38-84 subgrid_scores; models/parameterization.py:36-168 Parameterization.test_offline, which calls
``offline_dataset`` here).

Every reduction over the (run, time, lev, y, x) fields runs in libqgx.so (csrc/offline.hip):
  * spectra: ``qgx_rfft2`` of truth, sample, mean and psi in chunks of ``CHUNK`` snapshots, then
    ``qgx_offline_spectra`` sums the power, cospectrum and cross-layer planes per time window (t < 44, t >= 44);
  * moments: ``qgx_offline_moments``, the two-pass grouped sums behind mse / nmse / skill / correlation / var_ratio over
    (run, time), (run, y, x) and (run, time, y, x);
  * PDFs: ``qgx_histogram``, np.histogram's uniform bins on x / std in float64, with the view's population std.
Ratios, clipping, square roots and the isotropic binning (``spectrum.isotropize`` / ``calc_ispec``, a few thousand
numbers) stay on the host.

Deviations from the reference, both deliberate:
  * non-finite input gives NaN (metrics, spectra and PDF densities), where xarray's reductions skip NaN;
  * the PDFs divide in float64 by a float64 std, where the reference divides a float32 field by a float32 std: a value
    within about 1e-7 of a bin edge may land in the neighbouring bin.
"""
import ctypes as C
import time as _time

import numpy as np
import torch

from .. import _lib
from .._lib import lib, check
from ..engine import _ptr, _stream
from .operators import Dev
from .parameters import AVERAGE_SLICE_ANDREW
from .simulate import dataset_backend
from .spectral_tools import spectrum

CHUNK = 256               # snapshots per transform chunk of the spectra (512 fields per qgx_rfft2)
T0 = AVERAGE_SLICE_ANDREW.start
FIELDS = ('', '_gen', '_mean', '_res', '_gen_res')      # the planes' field order f: T, G, M, R = T - M, GR = G - M
DIMS = ('run', 'time', 'lev', 'y', 'x')


# ---- device helpers -----------------------------------------------------------------------------------------------
def _device(x, device=0):
    """numpy array / torch tensor -> contiguous float32 / float64 tensor on the GPU"""
    if isinstance(x, torch.Tensor):
        t = x if x.is_cuda else x.to(f'cuda:{device}')
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(f'cuda:{device}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.contiguous()


def _work(which, R=0, T=0, N=0, nbins=0, device=None):
    n = C.c_size_t()
    check(lib.qgx_offline_workspace(which, R, T, N, nbins, C.byref(n)))
    return torch.empty(max(n.value, 1), dtype=torch.uint8, device=device)


def _supported_grid(N):
    n = N
    for p in (2, 3):
        while n % p == 0:
            n //= p
    return 8 <= N <= 512 and N % 2 == 0 and n == 1


def check_fields(*arrays):
    """(run, time, lev, y, x) arrays with 2 layers and a square grid the transforms support; ValueError otherwise"""
    shape = None
    for a in arrays:
        s = tuple(np.shape(a))
        if len(s) != 5:
            raise ValueError(f'offline metrics need 5-D (run, time, lev, y, x) fields, got shape {s}')
        if s[2] != 2:
            raise ValueError(f'offline metrics need 2 layers, got {s[2]}')
        if s[3] != s[4] or not _supported_grid(s[4]):
            raise ValueError(f'offline metrics need a square N x N grid with N even, 8 <= N <= 512, N = 2^a 3^b; got '
                             f'{s[3]} x {s[4]}')
        if min(s) < 1:
            raise ValueError(f'empty field of shape {s}')
        if shape is not None and s != shape:
            raise ValueError(f'fields of different shapes {shape} and {s}')
        shape = s
    return shape


class _Timer:
    """wall time per phase; synchronises the device at each phase boundary when enabled"""

    def __init__(self, out):
        self.out = out
        self.t = _time.perf_counter()

    def __call__(self, name):
        if self.out is None:
            return
        torch.cuda.synchronize()
        now = _time.perf_counter()
        self.out[name] = self.out.get(name, 0.) + now - self.t
        self.t = now


def spectra_sums(t, m, g, psi=None, t0=T0, timer=None):
    """(R, T, 2, N, N) device fields -> (2 windows, 22 planes, N, N/2+1) host float64 sums over the snapshots of each
    window (window 1: time index >= t0); plane order of qgx_offline_spectra"""
    R, T, _, N, _ = t.shape
    S = R * T
    acc = _work(_lib.WORK_SPECTRA, N=N, device=t.device).view(torch.float64)
    flat = [None if x is None else x.reshape(S, 2, N, N) for x in (t, g, m, psi)]
    for s0 in range(0, S, CHUNK):
        hats = [None if x is None else Dev.rfft2(x[s0:s0 + CHUNK].reshape(-1, N, N).to(torch.float64)) for x in flat]
        if timer:
            timer('transforms')
        check(lib.qgx_offline_spectra(*(_ptr(h) for h in hats), min(CHUNK, S - s0), N, s0, T, t0, int(s0 > 0),
                                      _ptr(acc), _stream()))
        if timer:
            timer('densities')
    out = torch.empty((2, _lib.OFFLINE_PLANES, N, N // 2 + 1), dtype=torch.float64, device=t.device)
    check(lib.qgx_offline_spectra_finish(_ptr(acc), N, _ptr(out), _stream()))
    res = out.cpu().numpy()
    if timer:
        timer('densities')
    return res


def moment_sums(t, m, g):
    """(R, T, 2, N, N) device fields -> dict of host float64 sums, quantities q = [(t-m)^2, t^2, (t-t')^2, (m-m')^2,
    (t-t')(m-m'), (g-m)^2] with t', m' the group means: 'spatial' (6, 2, N, N), 'temporal' (6, T, 2), 'global' (6, 2)"""
    R, T, _, N, _ = t.shape
    work = _work(_lib.WORK_MOMENTS, R, T, N, device=t.device)
    out = torch.empty(6 * (2 * N * N + 2 * T + 2), dtype=torch.float64, device=t.device)
    dtypes = sum(int(x.dtype == torch.float64) << i for i, x in enumerate((t, m, g)))
    check(lib.qgx_offline_moments(_ptr(t), _ptr(m), _ptr(g), dtypes, R, T, N, _ptr(work), work.numel(), _ptr(out),
                                  _stream()))
    o = out.cpu().numpy()
    a, b = 6 * 2 * N * N, 6 * 2 * N * N + 6 * T * 2
    return {'spatial': o[:a].reshape(6, 2, N, N), 'temporal': o[a:b].reshape(6, T, 2), 'global': o[b:].reshape(6, 2)}


def histogram(x, edges, z=0, t0=0, scale=None, shape=None):
    """counts of np.histogram(x / scale, bins=edges) over layer z, time index >= t0 of a (R, T, nlev, P) device array
    (``shape``; default: x flat as one row).  scale=None: the view's population std.  -> (int64 counts, stats) with
    stats = [mean, std, non-finite count, scale used] (mean and std only when scale is None)"""
    R, T, nlev, P = shape if shape is not None else (1, 1, 1, x.numel())
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    ed = torch.from_numpy(edges).to(x.device)
    work = _work(_lib.WORK_HISTOGRAM, nbins=nb, device=x.device)
    counts = torch.empty(max(nb, 1), dtype=torch.int64, device=x.device)
    stats = torch.full((4,), np.nan, dtype=torch.float64, device=x.device)
    flags = _lib.HIST_STATS | _lib.HIST_SCALE_STD if scale is None else 0
    check(lib.qgx_histogram(_ptr(x), int(x.dtype == torch.float64), R, T, nlev, P, z, t0, _ptr(ed), nb, flags,
                            float(scale if scale is not None else 1.0), _ptr(work), work.numel(), _ptr(counts),
                            _ptr(stats), _stream()))
    return counts[:nb].cpu().numpy(), stats.cpu().numpy()


def _stats(x, shape=None):
    """[mean, population std, non-finite count] of a flat device array"""
    R, T, nlev, P = shape if shape is not None else (1, 1, 1, x.numel())
    work = _work(_lib.WORK_HISTOGRAM, device=x.device)
    stats = torch.full((4,), np.nan, dtype=torch.float64, device=x.device)
    check(lib.qgx_histogram(_ptr(x), int(x.dtype == torch.float64), R, T, nlev, P, 0, 0, None, 0, _lib.HIST_STATS, 1.0,
                            _ptr(work), work.numel(), None, _ptr(stats), _stream()))
    return stats.cpu().numpy()


# ---- the reference's functions ------------------------------------------------------------------------------------
def PDF_histogram(x, xmin=None, xmax=None, Nbins=30):
    """x: numpy array or torch tensor (flattened).  Default range mean -+ 4 sigma.  -> (bin centres, density) with
    density = counts / x.size / bandwidth (x.size counts values outside the range too); NaN densities if x holds a
    non-finite value"""
    n = x.numel() if isinstance(x, torch.Tensor) else np.size(x)
    if n == 0:
        raise ValueError('PDF_histogram of an empty array')
    if int(Nbins) < 1 or int(Nbins) > _lib.HIST_MAX_BINS:
        raise ValueError(f'Nbins must be in [1, {_lib.HIST_MAX_BINS}]')
    Nbins = int(Nbins)
    xd = _device(x).reshape(-1)
    with torch.cuda.device(xd.device):
        if xmin is None or xmax is None:
            mean, sigma, bad = _stats(xd)[:3]
            xmin = mean - 4 * sigma if xmin is None else xmin
            xmax = mean + 4 * sigma if xmax is None else xmax
        first, last = float(xmin) + 0.0, float(xmax) + 0.0
        if first > last:
            raise ValueError('max must be larger than min in range parameter.')
        if first == last:                        # np.histogram's widening of an empty range
            first, last = first - 0.5, last + 0.5
        bandwidth = (float(xmax) - float(xmin)) / Nbins
        edges = np.linspace(first, last, Nbins + 1)
        points = (edges[:-1] + edges[1:]) * 0.5
        if not (np.isfinite(first) and np.isfinite(last)):
            return points, np.full(Nbins, np.nan)
        counts, stats = histogram(xd, edges, scale=1.0)
    density = counts / n / bandwidth
    if stats[2] != 0:
        density = np.full(Nbins, np.nan)
    return points, density


def _values(da):
    dims = getattr(da, 'dims', None)
    if dims is not None and set(dims) == set(DIMS) and tuple(dims) != DIMS:
        da = da.transpose(*DIMS)
    return np.asarray(da.values if hasattr(da, 'values') else da)


def _sp_da(sp, af2, N, name, description, units):
    return sp.isotropize(af2, np.empty((0, N)), name=name, description=description, units=units)


def _R2(x, xt):
    return float((1 - ((x - xt) ** 2).mean(-1) / xt.var(-1)).mean())


def _L2(x, xt):
    return float(((((x - xt) ** 2).mean(-1) / (xt ** 2).mean(-1)) ** 0.5).mean())


class OfflineStats:
    """Every device reduction of the offline metrics for truth t, mean m, sample g [and psi]: (run, time, lev, y, x)
    arrays (numpy or torch).  timings: optional dict that receives wall seconds per phase (with device syncs)."""

    def __init__(self, t, m, g, psi=None, device=0, pdfs=False, res=None, gen_res=None, timings=None):
        self.shape = check_fields(*[a for a in (t, m, g, psi) if a is not None])
        R, T, _, N, _ = self.shape
        self.R, self.T, self.N = R, T, N
        timer = _Timer(timings)
        with torch.cuda.device(device):
            dev = [None if a is None else _device(a, device) for a in (t, m, g, psi)]
            timer('upload')
            self.spec = spectra_sums(*dev, t0=T0, timer=timer if timings is not None else None)
            self.mom = moment_sums(*dev[:3])
            timer('moments')
            self.pdf = self._pdfs(dev, res, gen_res, device, timer) if pdfs else None
            timer('histograms')

    def _pdfs(self, dev, res, gen_res, device, timer):
        """PDF{,_gen,_mean}{0,1} in units of the truth's std and PDF{_res,_gen_res}{0,1} in units of the truth
        residual's std over time index >= 44: 70 bins on [-5, 5]"""
        R, T, _, N, _ = self.shape
        edges = np.linspace(-5.0, 5.0, 71)
        out = {'points': (edges[:-1] + edges[1:]) * 0.5}
        tw = max(T - T0, 0)
        rd = [_device(a, device) for a in (res, gen_res)]
        groups = ((('', dev[0]), ('_gen', dev[2]), ('_mean', dev[1])), (('_res', rd[0]), ('_gen_res', rd[1])))
        for group in groups:
            for lev in (0, 1):
                if tw == 0:
                    for suffix, _ in group:
                        out[suffix + str(lev)] = np.full(70, np.nan)
                    continue
                scale = None
                for suffix, x in group:
                    counts, stats = histogram(x, edges, z=lev, t0=T0, scale=scale, shape=(R, T, 2, N * N))
                    if scale is None:
                        scale = float(stats[1])
                    dens = counts / (R * tw * N * N) / (10. / 70)
                    out[suffix + str(lev)] = dens if stats[2] == 0 and np.isfinite(scale) else np.full(70, np.nan)
        return out

    # ---- derived quantities ----
    def power(self, f, window):
        """(lev, N, N/2+1) time/run-mean power of field f (index into FIELDS); window 'all' or 'late' (t >= 44)"""
        return self._mean(self.spec[:, 2 * f:2 * f + 2], window)

    def cospectrum(self, f, window='late'):
        return self._mean(self.spec[:, 10 + 2 * f:12 + 2 * f], window)

    def cross(self, c, window='late'):
        return self._mean(self.spec[:, 20 + c], window)

    def _mean(self, planes, window):
        n_late = self.R * max(self.T - T0, 0)
        with np.errstate(invalid='ignore', divide='ignore'):
            if window == 'all':
                return (planes[0] + planes[1]) / (self.R * self.T)
            return planes[1] / n_late if n_late else np.full(planes[1].shape, np.nan)


def _scores(st):
    """the 0-d and spectral variables of subgrid_scores from an OfflineStats"""
    xr = dataset_backend()
    g = st.mom['global']
    sp = spectrum(time=slice(None, None))
    kw = dict(name='', description='', units='')
    ds = xr.Dataset()
    with np.errstate(invalid='ignore', divide='ignore'):
        ds['R2_mean'] = float((1 - g[0] / g[2]).mean())
        ds['L2_mean'] = float(np.sqrt(g[0] / g[1]).mean())
        ds['sp_true'] = _sp_da(sp, st.power(0, 'all'), st.N, **kw)
        ds['sp_gen'] = _sp_da(sp, st.power(1, 'all'), st.N, **kw)
        ds['R2_total'] = _R2(np.asarray(ds['sp_gen'].values), np.asarray(ds['sp_true'].values))
        ds['L2_total'] = _L2(np.asarray(ds['sp_gen'].values), np.asarray(ds['sp_true'].values))
        ds['sp_true_res'] = _sp_da(sp, st.power(3, 'all'), st.N, **kw)
        ds['sp_gen_res'] = _sp_da(sp, st.power(4, 'all'), st.N, **kw)
        ds['R2_residual'] = _R2(np.asarray(ds['sp_gen_res'].values), np.asarray(ds['sp_true_res'].values))
        ds['L2_residual'] = _L2(np.asarray(ds['sp_gen_res'].values), np.asarray(ds['sp_true_res'].values))
        ds['var_ratio'] = xr.DataArray(g[5] / g[0], dims=['lev'])
    return ds


def subgrid_scores(true, mean, gen, device=0):
    """Scalar scores of the mean, of one generated sample and of its residual for DataArrays (run, time, lev, y, x) of
    either backend: R2_* / L2_* (0-d), sp_true, sp_gen, sp_true_res, sp_gen_res (lev, k; full time window) and
    var_ratio (lev)"""
    t, m, g = (_values(a) for a in (true, mean, gen))
    return _scores(OfflineStats(t, m, g, device=device))


def offline_dataset(ds, preds, device=0, timings=None):
    """The dataset of the reference's Parameterization.test_offline from the input dataset ds (q, q_forcing_advection,
    psi) and predict's output preds (q_forcing_advection: one sample, _mean, _var).  timings: optional dict of wall
    seconds per phase."""
    xr = dataset_backend()
    target = 'q_forcing_advection'
    t0w = _time.perf_counter()
    true = _values(ds[target])
    gen, mean, var = (_values(preds[target + s]) for s in ('', '_mean', '_var'))
    psi = _values(ds['psi'])
    check_fields(true, gen, mean, var, psi)
    res = true.astype(np.float64) - mean
    gen_res = gen - mean
    host0 = _time.perf_counter() - t0w
    st = OfflineStats(true, mean, gen, psi, device=device, pdfs=True, res=res, gen_res=gen_res, timings=timings)
    t1 = _time.perf_counter()

    out = xr.Dataset(attrs=dict(ds.attrs))
    out[target] = xr.DataArray(true, dims=DIMS)
    out[target + '_mean'] = xr.DataArray(mean, dims=DIMS)
    out[target + '_var'] = xr.DataArray(var, dims=DIMS)
    out['q'] = xr.DataArray(_values(ds['q']), dims=DIMS)
    out[target + '_gen'] = xr.DataArray(gen, dims=DIMS)
    out[target + '_std'] = xr.DataArray(var ** 0.5, dims=DIMS)
    out[target + '_res'] = xr.DataArray(res, dims=DIMS)
    out[target + '_gen_res'] = xr.DataArray(gen_res, dims=DIMS)

    scores = _scores(st)
    for k in ('R2_mean', 'R2_total', 'R2_residual', 'L2_mean', 'L2_total', 'L2_residual'):
        out[k] = scores[k]

    R, T, _, N, _ = st.shape
    n = {'spatial': R * T, 'temporal': R * N * N, 'global': R * T * N * N}
    dims = {'spatial': ['lev', 'y', 'x'], 'temporal': ['time', 'lev'], 'global': ['lev']}
    prefix = {'spatial': 'spatial_', 'temporal': 'temporal_', 'global': ''}

    def limits(x):
        return np.minimum(np.maximum(x, -10), 1)

    with np.errstate(invalid='ignore', divide='ignore'):
        fld = {}
        for grp in ('spatial', 'temporal', 'global'):
            sdd, stt, ctt, cmm, ctm, sgg = (st.mom[grp][q] / n[grp] for q in range(6))
            fld[grp] = dict(mse=sdd, nmse=sdd / stt, skill=limits(1 - sdd / ctt),
                            correlation=ctm / (np.sqrt(ctt) * np.sqrt(cmm)), sgs_ms=stt, var_ratio=sgg / sdd)
        order = [('spatial', 'mse'), ('temporal', 'mse'), ('global', 'mse'), ('temporal', 'sgs_ms'),
                 ('spatial', 'nmse'), ('temporal', 'nmse'), ('global', 'nmse'),
                 ('spatial', 'skill'), ('temporal', 'skill'), ('global', 'skill'),
                 ('spatial', 'correlation'), ('temporal', 'correlation'), ('global', 'correlation'),
                 ('temporal', 'var_ratio'), ('global', 'var_ratio')]
        for grp, q in order:
            out[prefix[grp] + q] = xr.DataArray(fld[grp][q], dims=dims[grp])

        sp = spectrum()
        for f, suffix in ((0, ''), (1, '_gen'), (3, '_res'), (4, '_gen_res'), (2, '_mean')):
            out['PSD' + suffix] = _sp_da(sp, st.power(f, 'late'), N, name='Power spectral density of $dq/dt$',
                                         units='$m/s^4$', description='Power spectrum of subgrid forcing')
        sp = spectrum(type='cospectrum')
        for f, suffix in ((0, ''), (1, '_gen'), (3, '_res'), (4, '_gen_res'), (2, '_mean')):
            out['Eflux' + suffix] = -_sp_da(sp, st.cospectrum(f), N, name='Energy contribution', units='$m^3/s^3$',
                                            description='Energy contribution of subgrid forcing')

        def L2(x, x_true):
            x, x_true = np.asarray(x.values), np.asarray(x_true.values)
            return xr.DataArray((((x - x_true) ** 2).mean(-1) / (x_true ** 2).mean(-1)) ** 0.5, dims=['lev'])
        out['L2_PSD'] = L2(out['PSD_gen'], out['PSD'])
        out['L2_Eflux'] = L2(out['Eflux_gen'], out['Eflux'])

        sp = spectrum(type='cross_layer')
        for c, suffix in ((0, '_res'), (1, '_gen_res')):
            out['CSD' + suffix] = _sp_da(sp, st.cross(c), N, name='Cross layer covariance', units='$m/s^4$',
                                         description='Cross layer covariance of subgrid forcing')

    for names, dim in ((('', '_gen', '_mean'), 'q_'), (('_res', '_gen_res'), 'dq_')):
        for lev in (0, 1):
            c = xr.DataArray(st.pdf['points'], dims=[dim + str(lev)], attrs={'long_name': 'RMS units'})
            for suffix in names:
                out['PDF' + suffix + str(lev)] = xr.DataArray(st.pdf[suffix + str(lev)], dims=[dim + str(lev)],
                                                              coords={dim + str(lev): c})
    if 'time' in ds:
        out['time'] = ds['time'].copy(deep=True)
    out = out.astype('float32')
    if timings is not None:
        timings['host'] = timings.get('host', 0.) + host0 + _time.perf_counter() - t1
    return out
