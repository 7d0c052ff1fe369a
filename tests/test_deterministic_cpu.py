"""CPU: the ABI of sampling='deterministic' (QGX_SAMPLING_DETERMINISTIC, qgx_param.n_mean, qgx_generator_forward_mean's
argument checks, which run before any device call) and the Philox key of its realisations
(parameterization.py:27-28 -> predict_mean_snapshot, cgan_regression.py:164-171)."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from oracle import samplers_ref

QGX_ERR_INVALID = -1


def test_sampling_enum_and_param_layout():
    from pyqg_generative_amd import _lib
    assert (_lib.SAMPLING_AR1, _lib.SAMPLING_CONSTANT, _lib.SAMPLING_DETERMINISTIC) == (0, 1, 2)
    header = open(os.path.join(ROOT, 'include', 'qgx.h')).read()
    assert re.search(r'QGX_SAMPLING_DETERMINISTIC\s*=\s*2\b', header)
    # n_mean took the place of the reserved word: the last int32 of a 64-byte struct, every other field where it was
    assert C.sizeof(_lib.qgx_param) == 64
    assert _lib.qgx_param.n_mean.offset == 60 and _lib.qgx_param.n_mean.size == 4
    assert _lib.qgx_param.demean.offset == 56 and _lib.qgx_param.forcing_dev.offset == 48
    assert not hasattr(_lib.qgx_param, 'reserved')
    assert re.search(r'int32_t\s+n_mean;', header) and not re.search(r'int32_t\s+reserved;', header)
    p = _lib.qgx_param()
    p.n_mean = 100
    assert bytes(p)[60:64] == (100).to_bytes(4, 'little')


def test_forward_mean_refuses_bad_arguments_without_a_device():
    """null pointers, M < 1, M > 65536, step >= 2^32 and 0 < chunk < B are QGX_ERR_INVALID before the handle is read or any
    HIP call is made: the 'handle' and the 'device pointers' here are host memory that is never dereferenced"""
    from pyqg_generative_amd._lib import lib
    fake = C.create_string_buffer(1 << 16)
    h, q, S = (C.c_void_p(C.addressof(fake) + o) for o in (0, 4096, 8192))
    null = C.c_void_p(0)
    B, N = 4, 48
    good = dict(M=5, chunk=0, step=0)

    def call(g=h, q=q, S=S, **kw):
        a = dict(good, **kw)
        return lib.qgx_generator_forward_mean(g, q, S, B, N, a['M'], a['chunk'], 1, 7, 0, a['step'], null)
    for kw, word in ((dict(g=null), 'null'), (dict(q=null), 'null'), (dict(S=null), 'null'),
                     (dict(M=0), 'M = 0'), (dict(M=-3), 'M = -3'), (dict(M=65537), 'M = 65537'),
                     (dict(step=1 << 32), '2^32'), (dict(step=(1 << 40) + 1), '2^32'),
                     (dict(chunk=1), 'chunk = 1'), (dict(chunk=B - 1), f'chunk = {B - 1}')):
        assert call(**kw) == QGX_ERR_INVALID, kw
        assert word in lib.qgx_last_error().decode(), (kw, lib.qgx_last_error())


def test_realisation_key_is_a_stream_of_its_own():
    """realisation j of key-step t draws (seed, member, t | (j + 1) << 32): the high word of the step, which no AR1 /
    constant draw ever sets, so the stream differs from (seed, member, t), from every other realisation's and from the
    next step's — integer-exact, on the raw Philox words"""
    seed, member, t, n = 21, 7, 3, 256
    base, raw_base = samplers_ref.philox_normal(seed, member, t, n)
    raws = [raw_base]
    for j in range(4):
        x, raw = samplers_ref.philox_normal(seed, member, t | (j + 1) << 32, n)
        assert x.dtype == np.float32 and np.isfinite(x).all()
        raws.append(raw)
    raws.append(samplers_ref.philox_normal(seed, member, (t + 1) | 1 << 32, n)[1])
    for i in range(len(raws)):
        for k in range(i + 1, len(raws)):
            # independent 32-bit words agree with probability 2^-32 each: no agreement in 256 words
            assert (raws[i] == raws[k]).sum() == 0, (i, k)
    # the low word alone keys the AR1 / constant streams: t + (j + 1) << 32 and t | (j + 1) << 32 are the same key for t < 2^32
    assert (t + (1 << 32)) == (t | 1 << 32)
