"""CPU: every entry point of include/qgx.h that writes a caller's device buffer has a guard-band test.

The list is computed from `_lib.SYMBOLS` (every symbol with a `void *` argument: device pointers, handles and streams
all travel as one), minus the exclusions below, each with its reason; what is left must be called in
tests/test_gpu_abi_bounds.py.  A new entry point therefore needs a bounds test or a stated reason."""
import ctypes as C
import os
import re

import pytest

pytest.importorskip('torch')

HERE = os.path.dirname(os.path.abspath(__file__))

# symbols with a void * argument that take NO caller-supplied device output or workspace
EXCLUDED = {
    # the void * is the handle (and a stream) only; what they write is the handle's own state
    'qgx_destroy': 'handle only',
    'qgx_invert': 'handle and stream: writes ph, u, v of the model',
    'qgx_step': 'handle and stream: writes the model state (its device inputs z_external_dev / forcing_dev are read-only)',
    'qgx_step_streams': 'handle only, a query',
    'qgx_step_count': 'handle only, a query',
    'qgx_run_kernel_state': 'handle only, a query',
    'qgx_reset_time': 'handle only',
    'qgx_set_option': 'handle only',
    'qgx_diag_config': 'handle only',
    'qgx_diag_count': 'handle only, a query',
    'qgx_diag_reset': 'handle only',
    'qgx_generator_destroy': 'handle only',
    'qgx_generator_set_option': 'handle only',
    'qgx_generator_size_ok': 'handle only, no device call',
    'qgx_generator_layer2_kernel': 'handle only; its output is a host int',
    'qgx_generator_profile': 'handle only',
    'qgx_generator_profile_read': 'handle only; host outputs',
    'qgx_generator_info': 'handle only; host outputs',
    'qgx_generator_wino_info': 'handle only; host outputs',
    'qgx_generator_wino_info_n': 'handle only; host outputs',
    'qgx_generator_range_read': 'handle and stream; host outputs',
    # device INPUTS only (copied into the model)
    'qgx_set_q': 'device input only',
    'qgx_set_qh': 'device input only',
    # host pointers
    'qgx_get_table': 'writes a HOST buffer (tests/test_gpu_parity.py compares every table)',
    'qgx_set_viscosity': 'host input, stream',
    'qgx_get_viscosity': 'host outputs',
    'qgx_set_backscatter': 'host inputs, stream',
    'qgx_get_backscatter': 'host outputs',
    'qgx_field_bytes': 'a size query (its answers are what the bounds tests size their buffers by)',
}


def _with_void_pointer():
    from pyqg_generative_amd._lib import SYMBOLS
    return [name for name, _, args in SYMBOLS if C.c_void_p in args]


def test_every_writing_entry_point_has_a_bounds_test():
    names = _with_void_pointer()
    assert set(EXCLUDED) <= set(names), sorted(set(EXCLUDED) - set(names))      # no stale exclusions
    must = [n for n in names if n not in EXCLUDED]
    text = open(os.path.join(HERE, 'test_gpu_abi_bounds.py')).read()
    missing = [n for n in must if not re.search(rf'\blib\.{n}\(', text)]
    assert not missing, f'no guard-band test calls {missing}: add one to tests/test_gpu_abi_bounds.py (or a reasoned exclusion)'
    # the list itself, so that a change of it is seen in review
    assert sorted(must) == sorted([
        'qgx_get', 'qgx_backscatter_forcing', 'qgx_status_ke_cfl', 'qgx_diag_get', 'qgx_generator_forward',
        'qgx_generator_forward_mean', 'qgx_cnn_forward', 'qgx_rfft2', 'qgx_irfft2', 'qgx_spec_regrid', 'qgx_spec_div',
        'qgx_real_fma', 'qgx_moments_accumulate', 'qgx_noise_normal', 'qgx_w1_keys', 'qgx_w1_sorted', 'qgx_spec_curl',
        'qgx_offline_spectra', 'qgx_offline_spectra_finish', 'qgx_offline_moments', 'qgx_histogram'])


def test_symbols_without_any_pointer_are_queries():
    """what the computation above cannot see: symbols with no void * at all — they take no device memory"""
    from pyqg_generative_amd._lib import SYMBOLS
    rest = sorted(name for name, _, args in SYMBOLS if C.c_void_p not in args)
    assert rest == ['qgx_create', 'qgx_generator_create', 'qgx_generator_create_ann', 'qgx_generator_create_unet',
                    'qgx_last_error', 'qgx_offline_workspace', 'qgx_version', 'qgx_w1_workspace']
