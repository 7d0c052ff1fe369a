"""Test-side float64 numpy restatement of the reference's run statistics, written from their formulas
(pyqg_generative/tools/comparison_tools.py:197-271 dataset_statistics, :273-410 dataset_smart_read): plain arrays in, a
dict of numpy arrays out.  A run is a dict with
  u, v [, q]         (R, T, 2, N, N)   snapshots
  time               (T)               in days
  <diagnostic>       (R, 2, N, N/2+1) or (R, N, N/2+1)   time-averaged spectra, any of DIAGNOSTICS
The curl is oracle.metrics_ref._curl, the binning oracle.spectral_ref.calc_ispec, the PDFs offline_restatement.pdf.
"""
import numpy as np

from oracle.metrics_ref import _curl
from oracle.qg_ref import QGModelRef
from oracle.spectral_ref import calc_ispec
from offline_restatement import pdf

DIAGNOSTICS = ['APEflux', 'APEgenspec', 'Dissspec', 'ENSDissspec', 'ENSflux', 'ENSfrictionspec', 'ENSgenspec',
               'ENSparamspec', 'Ensspec', 'KEflux', 'KEfrictionspec', 'KEspec', 'entspec', 'paramspec', 'paramspec_APEflux',
               'paramspec_KEflux']
T0 = 44                    # AVERAGE_SLICE_ANDREW = slice(44, None)
PDF_XMAX = {('Ens', 0): 1e-10, ('Ens', 1): 1.5e-12, ('KE', 0): 1.5e-2, ('KE', 1): 5e-4}


def flow_features(u, v):
    """u, v (..., N, N) -> omega = ddx(v) - ddy(u), KE = (u^2 + v^2) / 2, Ens = omega^2 / 2, Vabs = sqrt(2 KE) and KE_sum,
    the sum of KE over the last two axes"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    omega = _curl(u, v)
    ke = (u ** 2 + v ** 2) * 0.5
    return {'omega': omega, 'KE': ke, 'Ens': 0.5 * omega ** 2, 'Vabs': np.sqrt(2 * ke), 'KE_sum': ke.sum(axis=(-2, -1))}


def layer_weights(delta):
    return np.array([delta / (1 + delta), 1 / (1 + delta)])


def ke_time(u, v, delta):
    """ave_lev(KE, delta).mean(('run', 'x', 'y')) of (R, T, 2, N, N) fields -> (T)"""
    ke = flow_features(u, v)['KE']
    return (ke * layer_weights(delta)[:, None, None]).sum(axis=2).mean(axis=(0, 2, 3))


def spectra(run, delta, **kw_ispec):
    """the ...r / ...r_mean variables, Energysumr and Efluxr"""
    out = {}
    g = QGModelRef(nx=np.asarray(run['u']).shape[-1])
    for key in DIAGNOSTICS:
        if key not in run:
            continue
        var = np.asarray(run[key], dtype=np.float64).mean(axis=0)
        if var.ndim == 3:
            per_layer = [calc_ispec(g, var[z], **kw_ispec) for z in (0, 1)]
            out['kr'] = per_layer[0][0]
            out[key + 'r'] = np.stack([sp for _, sp in per_layer])
            w = layer_weights(delta)
            out[key + 'r_mean'] = calc_ispec(g, w[0] * var[0] + w[1] * var[1], **kw_ispec)[1]
        else:
            out['kr'], out[key + 'r'] = calc_ispec(g, var, **kw_ispec)
    out['Energysumr'] = sum(out[k] for k in ('KEfluxr', 'APEfluxr', 'APEgenspecr', 'KEfrictionspecr', 'paramspec_APEfluxr',
                                             'paramspec_KEfluxr') if k in out)
    out['Efluxr'] = sum(out[k] for k in ('KEfluxr', 'APEfluxr', 'paramspec_KEfluxr', 'paramspec_APEfluxr') if k in out)
    return out


def dataset_statistics(run, delta=0.25, **kw_ispec):
    out = spectra(run, delta, **kw_ispec)
    out['KE_time'] = ke_time(run['u'], run['v'], delta)
    out['time'] = np.asarray(run['time'], dtype=np.float64) / 360       # ('years' is never a KEY of the attributes)
    return out


def dataset_smart_read(run, delta=0.25, compute_all=True):
    out = spectra(run, delta)
    f = flow_features(run['u'], run['v'])
    if compute_all:
        out.update({k: f[k] for k in ('omega', 'KE', 'Ens', 'Vabs')})
    window = slice(T0, None) if compute_all else slice(-1, None)
    fields = {'q': run['q'], 'u': run['u'], 'v': run['v'], 'KE': f['KE'], 'Ens': f['Ens']}
    for var in ('q', 'u', 'v', 'KE', 'Ens') if compute_all else ('q', 'u', 'v', 'KE'):
        for lev in (0, 1):
            x = np.asarray(fields[var], dtype=np.float64)[:, window, lev]
            out[f'{var}_{lev}'], out[f'PDF_{var}{lev + 1}'] = pdf(x, 0 if var in ('KE', 'Ens') else None,
                                                                  PDF_XMAX.get((var, lev)), 30)
    out['KE_time'] = ke_time(run['u'], run['v'], delta)
    out['time'] = np.asarray(run['time'], dtype=np.float64) / 360
    return out
