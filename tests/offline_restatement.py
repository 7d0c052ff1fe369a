"""Test-side numpy restatement of the reference's offline metrics, written from their formulas
(pyqg_generative/models/parameterization.py:36-168 test_offline, tools/computational_tools.py:5-84 PDF_histogram and
subgrid_scores, tools/spectral_tools.py:7-101 spectrum): plain arrays (run, time, lev, N, N) in, a dict of numpy arrays
out.  It follows the product's conventions where the two differ from the reference by design: residuals are formed in
float64, and the PDFs divide a float64 field by a float64 population std.
"""
import numpy as np

from oracle.qg_ref import QGModelRef
from oracle.spectral_ref import calc_ispec

T0 = 44                    # AVERAGE_SLICE_ANDREW = slice(44, None)
NBINS = 70


def uniform_histogram(x, first, last, nbins):
    """np.histogram(x, bins=nbins, range=(first, last)) for float64 x, value by value: edges from np.linspace, the bin
    from ((v - first) / (last - first)) * nbins truncated, moved down one if v lies below its left edge, up one if it
    lies on or above its right edge (except in the last bin, which is closed)"""
    edges = np.linspace(first, last, nbins + 1)
    counts = np.zeros(nbins, dtype=np.int64)
    for v in np.asarray(x, dtype=np.float64).ravel():
        if not (first <= v <= last):
            continue
        i = min(int(((v - first) / (last - first)) * nbins), nbins - 1)
        if v < edges[i]:
            i -= 1
        if i != nbins - 1 and v >= edges[i + 1]:
            i += 1
        counts[i] += 1
    return counts


def pdf(x, xmin=None, xmax=None, nbins=30):
    """PDF_histogram: (bin centres, counts / x.size / bandwidth); default range mean -+ 4 population std"""
    x = np.asarray(x, dtype=np.float64).ravel()
    xmin = x.mean() - 4 * x.std() if xmin is None else xmin
    xmax = x.mean() + 4 * x.std() if xmax is None else xmax
    counts, edges = np.histogram(x, bins=nbins, range=(xmin, xmax))
    return (edges[:-1] + edges[1:]) / 2, counts / x.size / ((xmax - xmin) / nbins)


def _fft(x):
    x = np.asarray(x, dtype=np.float64)
    return np.fft.rfftn(x, axes=(-2, -1)) / (x.shape[-1] * x.shape[-2])


def iso(af2):
    """spectrum()'s binning (averaging=False, truncate=False) of (..., N, N/2+1) densities -> (k, (..., nk))"""
    g = QGModelRef(nx=af2.shape[-2])
    lead = af2.shape[:-2]
    flat = af2.reshape((-1,) + af2.shape[-2:])
    out = [calc_ispec(g, a, averaging=False, truncate=False) for a in flat]
    return out[0][0], np.stack([o[1] for o in out]).reshape(lead + (-1,))


def power(x, t0=0):
    """run/time-mean isotropic power per lev of x (run, time, lev, N, N) over time index >= t0"""
    return iso((np.abs(_fft(x[:, t0:])) ** 2).mean(axis=(0, 1)))[1]


def cospectrum(a, b, t0=T0):
    return iso(np.real(np.conj(_fft(a[:, t0:])) * _fft(b[:, t0:])).mean(axis=(0, 1)))[1]


def cross_layer(x, t0=T0):
    f = _fft(x[:, t0:])
    return iso(np.real(np.conj(f[:, :, 0]) * f[:, :, 1]).mean(axis=(0, 1)))[1]


def subgrid_scores(true, mean, gen):
    true, mean, gen = (np.asarray(a, dtype=np.float64) for a in (true, mean, gen))
    ax = (0, 1, 3, 4)

    def R2(x, xt, axes):
        return float((1 - ((x - xt) ** 2).mean(axes) / xt.var(axes)).mean())

    def L2(x, xt, axes):
        return float(np.sqrt(((x - xt) ** 2).mean(axes) / (xt ** 2).mean(axes)).mean())
    out = {'R2_mean': R2(mean, true, ax), 'L2_mean': L2(mean, true, ax)}
    out['sp_true'], out['sp_gen'] = power(true), power(gen)
    out['sp_true_res'], out['sp_gen_res'] = power(true - mean), power(gen - mean)
    for name, a, b in (('total', 'sp_gen', 'sp_true'), ('residual', 'sp_gen_res', 'sp_true_res')):
        out['R2_' + name] = R2(out[a], out[b], -1)
        out['L2_' + name] = L2(out[a], out[b], -1)
    out['var_ratio'] = ((gen - mean) ** 2).mean(ax) / ((true - mean) ** 2).mean(ax)
    return out


def test_offline(true, mean, gen, psi):
    """every computed variable of Parameterization.test_offline, float64, before the final float32 cast"""
    true, mean, gen, psi = (np.asarray(a, dtype=np.float64) for a in (true, mean, gen, psi))
    res, gen_res = true - mean, gen - mean
    out = {k: v for k, v in subgrid_scores(true, mean, gen).items() if k[:2] in ('R2', 'L2')}
    err = (true - mean) ** 2
    for prefix, axes in (('spatial_', (0, 1)), ('temporal_', (0, 3, 4)), ('', (0, 1, 3, 4))):
        tm = true.mean(axes, keepdims=True)
        pm = mean.mean(axes, keepdims=True)
        mse = err.mean(axes)
        var_t = ((true - tm) ** 2).mean(axes)
        var_p = ((mean - pm) ** 2).mean(axes)
        cov = ((true - tm) * (mean - pm)).mean(axes)
        out[prefix + 'mse'] = mse
        out[prefix + 'nmse'] = mse / (true ** 2).mean(axes)
        out[prefix + 'skill'] = np.clip(1 - mse / var_t, -10, 1)
        out[prefix + 'correlation'] = cov / np.sqrt(var_t * var_p)
    out['temporal_sgs_ms'] = (true ** 2).mean((0, 3, 4))
    out['temporal_var_ratio'] = (gen_res ** 2).mean((0, 3, 4)) / (res ** 2).mean((0, 3, 4))
    out['var_ratio'] = (gen_res ** 2).mean((0, 1, 3, 4)) / (res ** 2).mean((0, 1, 3, 4))
    fields = {'': true, '_gen': gen, '_res': res, '_gen_res': gen_res, '_mean': mean}
    for s, x in fields.items():
        out['PSD' + s] = power(x, T0)
        out['Eflux' + s] = -cospectrum(psi, x)
    for name in ('PSD', 'Eflux'):
        out['L2_' + name] = np.sqrt(((out[name + '_gen'] - out[name]) ** 2).mean(-1) / (out[name] ** 2).mean(-1))
    out['CSD_res'], out['CSD_gen_res'] = cross_layer(res), cross_layer(gen_res)
    edges = np.linspace(-5, 5, NBINS + 1)
    out['points'] = (edges[:-1] + edges[1:]) / 2
    for group in (('', '_gen', '_mean'), ('_res', '_gen_res')):
        for lev in (0, 1):
            std = fields[group[0]][:, T0:, lev].std()
            for s in group:
                x = fields[s][:, T0:, lev].ravel() / std
                out['PDF' + s + str(lev)] = pdf(x, -5, 5, NBINS)[1]
    return out
