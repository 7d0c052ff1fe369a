"""ctypes binding of the C-ABI library ``libqgx.so`` (include/qgx.h).

The HIP library is the product: there is NO CPU fallback.  Importing this
module without the built library raises ``ImportError`` loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('QGX_LIB') or os.path.join(_HERE, 'libqgx.so')   # QGX_LIB: developer builds only


class QgxError(RuntimeError):
    pass


class qgx_config(C.Structure):
    _fields_ = [('nx', C.c_int32), ('n_members', C.c_int32), ('device', C.c_int32),
                ('plan_only', C.c_int32),
                ('L', C.c_double), ('dt', C.c_double), ('rek', C.c_double), ('delta', C.c_double),
                ('beta', C.c_double), ('rd', C.c_double), ('U1', C.c_double), ('U2', C.c_double),
                ('H1', C.c_double), ('filterfac', C.c_double)]


class qgx_param(C.Structure):
    _fields_ = [('gen', C.c_void_p), ('sampling', C.c_int32), ('nsteps', C.c_int32),
                ('weight', C.c_double), ('seed', C.c_uint64), ('member_offset', C.c_uint64),
                ('z_external_dev', C.c_void_p), ('forcing_dev', C.c_void_p),
                ('demean', C.c_int32), ('n_mean', C.c_int32)]


class qgx_cnn_weights(C.Structure):
    _fields_ = [('n_in', C.c_int32), ('n_out', C.c_int32),
                ('conv_w', C.c_void_p * 8), ('conv_b', C.c_void_p * 8),
                ('bn_gamma', C.c_void_p * 7), ('bn_beta', C.c_void_p * 7),
                ('bn_mean', C.c_void_p * 7), ('bn_var', C.c_void_p * 7),
                ('bn_eps', C.c_float)]


class qgx_cnn_arch(C.Structure):
    _fields_ = [('n_layers', C.c_int32), ('channels', C.c_int32 * 9), ('ksize', C.c_int32 * 8),
                ('batch_norm', C.c_int32), ('bias', C.c_int32), ('force_generic', C.c_int32),
                ('conv_w', C.c_void_p * 8), ('conv_b', C.c_void_p * 8),
                ('bn_gamma', C.c_void_p * 7), ('bn_beta', C.c_void_p * 7),
                ('bn_mean', C.c_void_p * 7), ('bn_var', C.c_void_p * 7),
                ('bn_eps', C.c_float)]


class qgx_unet_res(C.Structure):
    _fields_ = [('bn_gamma', C.c_void_p), ('bn_beta', C.c_void_p), ('bn_mean', C.c_void_p), ('bn_var', C.c_void_p),
                ('conv_a_w', C.c_void_p), ('conv_a_b', C.c_void_p),
                ('bn2_gamma', C.c_void_p), ('bn2_beta', C.c_void_p), ('bn2_mean', C.c_void_p), ('bn2_var', C.c_void_p),
                ('conv_b_w', C.c_void_p), ('conv_b_b', C.c_void_p), ('skip_w', C.c_void_p), ('skip_b', C.c_void_p)]


class qgx_unet_weights(C.Structure):
    _fields_ = [('conv32_w', C.c_void_p), ('conv32_b', C.c_void_p), ('res', qgx_unet_res * 11),
                ('up_w', C.c_void_p * 4), ('up_b', C.c_void_p * 4),
                ('conv_end_w', C.c_void_p), ('conv_end_b', C.c_void_p), ('bn_eps', C.c_float)]


class qgx_ann_weights(C.Structure):
    _fields_ = [('stencil_size', C.c_int32), ('n_hidden', C.c_int32), ('hidden', C.c_int32 * 4),
                ('scale_invariant', C.c_int32), ('w', C.c_void_p * 5), ('b', C.c_void_p * 5)]


# enum mirrors (include/qgx.h)
F_Q, F_QH, F_PH, F_U, F_V, F_DQHDT, F_DQHDT_P, F_DQHDT_PP, F_S, F_Z, F_P = range(11)
T_FILTR, T_WV2, T_A, T_KK, T_LL = range(5)
SAMPLING_AR1, SAMPLING_CONSTANT, SAMPLING_DETERMINISTIC = 0, 1, 2
DIAGS = ['KEspec', 'Ensspec', 'entspec', 'APEflux', 'KEflux', 'APEgenspec', 'KEfrictionspec', 'paramspec',
         'paramspec_APEflux', 'paramspec_KEflux', 'Dissspec', 'ENSDissspec', 'ENSflux', 'ENSgenspec', 'ENSfrictionspec',
         'ENSparamspec']
GEN_GAN, GEN_VAE, GEN_GZ, GEN_OLS = 0, 1, 2, 3
GEN_ANN = 4          # enum qgx_gen_kind_ann: handles of qgx_generator_create_ann only
W1_IDENTITY, W1_SUMSQ2, W1_SQUARE = 0, 1, 2
W1_PARTIALS = 1024
OFFLINE_PLANES, OFFLINE_SPEC_GROUPS, HIST_MAX_BINS = 22, 32, 4096
WORK_SPECTRA, WORK_MOMENTS, WORK_HISTOGRAM = 0, 1, 2
HIST_STATS, HIST_SCALE_STD = 1, 2

# every symbol include/qgx.h declares: (name, restype, argtypes)
SYMBOLS = [
    ('qgx_create', C.c_int, [C.POINTER(qgx_config), C.POINTER(C.c_void_p)]),
    ('qgx_destroy', C.c_int, [C.c_void_p]),
    ('qgx_set_q', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_set_qh', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_get', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_get_table', C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ('qgx_field_bytes', C.c_size_t, [C.c_void_p, C.c_int]),
    ('qgx_invert', C.c_int, [C.c_void_p, C.c_void_p]),
    ('qgx_step', C.c_int, [C.c_void_p, C.c_int, C.POINTER(qgx_param), C.c_int, C.c_void_p]),
    ('qgx_step_streams', C.c_int, [C.c_void_p, C.POINTER(qgx_param)]),
    ('qgx_step_count', C.c_int64, [C.c_void_p]),
    ('qgx_run_kernel_state', C.c_int, [C.c_void_p]),
    ('qgx_reset_time', C.c_int, [C.c_void_p]),
    ('qgx_set_option', C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ('qgx_set_viscosity', C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p]),
    ('qgx_get_viscosity', C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ('qgx_set_backscatter', C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_void_p]),
    ('qgx_get_backscatter', C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ('qgx_backscatter_forcing', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_status_ke_cfl', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_diag_config', C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    ('qgx_diag_get', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_diag_count', C.c_int64, [C.c_void_p]),
    ('qgx_diag_reset', C.c_int, [C.c_void_p]),
    ('qgx_generator_create', C.c_int, [C.c_int, C.POINTER(qgx_cnn_weights), C.c_int,
                                       C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                       C.POINTER(C.c_void_p)]),
    ('qgx_generator_create_unet', C.c_int, [C.POINTER(qgx_unet_weights), C.POINTER(qgx_cnn_weights),
                                            C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_void_p)]),
    ('qgx_generator_create_ann', C.c_int, [C.POINTER(qgx_ann_weights), C.c_float, C.c_float, C.c_int,
                                           C.POINTER(C.c_void_p)]),
    ('qgx_generator_destroy', C.c_int, [C.c_void_p]),
    ('qgx_generator_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int, C.c_void_p]),
    ('qgx_generator_forward_mean', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]),
    ('qgx_cnn_forward', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p]),
    ('qgx_rfft2', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_irfft2', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_spec_regrid', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                  C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_spec_div', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    ('qgx_real_fma', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p,
                               C.c_double, C.c_void_p]),
    ('qgx_moments_accumulate', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ('qgx_generator_set_option', C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ('qgx_generator_range_read', C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_float), C.c_void_p]),
    ('qgx_generator_info', C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_float)]),
    ('qgx_generator_wino_info', C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    ('qgx_generator_wino_info_n', C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    ('qgx_generator_size_ok', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    ('qgx_generator_layer2_kernel', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    ('qgx_generator_profile', C.c_int, [C.c_void_p, C.c_int]),
    ('qgx_generator_profile_read', C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ('qgx_noise_normal', C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                   C.c_uint64, C.c_double, C.c_double, C.c_void_p]),
    ('qgx_w1_workspace', C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)]),
    ('qgx_w1_keys', C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                              C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('qgx_w1_sorted', C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ('qgx_spec_curl', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]),
    ('qgx_offline_workspace', C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    ('qgx_offline_spectra', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64,
                                      C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_offline_spectra_finish', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_offline_moments', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int,
                                      C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ('qgx_histogram', C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    ('qgx_last_error', C.c_char_p, []),
    ('qgx_version', C.c_char_p, []),
]
# what include/qgx_arch.h declares (SYMBOLS mirrors qgx.h itself): creators that take host descriptors and no caller's device buffer
ARCH_SYMBOLS = [
    ('qgx_generator_create_arch', C.c_int, [C.c_int, C.POINTER(qgx_cnn_arch), C.c_int,
                                            C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int,
                                            C.POINTER(C.c_void_p)]),
]
# what include/qgx_stats.h declares: the derived flow fields behind dataset_statistics / dataset_smart_read
STATS_SYMBOLS = [
    ('qgx_flow_features_workspace', C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_size_t)]),
    ('qgx_flow_features', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
]
# what include/qgx_train.h declares: stencil rows and the trainer of ANNModel's network (tools/train_ANN.py)
TRAIN_PARAMS, TRAIN_GRAD, TRAIN_M, TRAIN_V = range(4)
_BATCH = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float]   # t, x, y, idx, n, scales
TRAIN_SYMBOLS = [
    ('qgx_ann_rows', C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ('qgx_ann_trainer_create', C.c_int, [C.POINTER(qgx_ann_weights), C.c_int, C.POINTER(C.c_void_p)]),
    ('qgx_ann_trainer_destroy', C.c_int, [C.c_void_p]),
    ('qgx_ann_trainer_size', C.c_int64, [C.c_void_p]),
    ('qgx_ann_trainer_grad', C.c_int, _BATCH + [C.c_void_p, C.c_void_p]),
    ('qgx_ann_trainer_adam', C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    ('qgx_ann_trainer_step', C.c_int, _BATCH + [C.c_double, C.c_void_p, C.c_void_p]),
    ('qgx_ann_trainer_loss', C.c_int, _BATCH + [C.c_void_p, C.c_void_p]),
    ('qgx_ann_trainer_read', C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    ('qgx_ann_trainer_write', C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
]

# what include/qgx_conv_train.h declares: the circular convolution and its two gradients (tools/train_ops.py)
_CONV = [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]                                       # B, N, cin, cout, k
_CONV_WORK = [C.c_void_p, C.c_size_t, C.c_void_p]                                             # work, work_bytes, stream
CONV_TRAIN_SYMBOLS = [
    ('qgx_conv2d_workspace', C.c_int, _CONV + [C.POINTER(C.c_size_t)]),
    ('qgx_conv2d_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
    ('qgx_conv2d_backward_data', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
    ('qgx_conv2d_backward_weight', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
]

# what include/qgx_head_train.h declares: the batch gather and the loss head of a net's training step (tools/train_ops.py)
HEAD_MSE, HEAD_SOFTPLUS_MSE = 0, 1
_HEAD = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]                                         # y, t, idx, mode
_HEAD_SHAPE = [C.c_int64, C.c_int, C.c_int, C.c_int64]                                        # B, N, C, n
HEAD_TRAIN_SYMBOLS = [
    ('qgx_batch_gather', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    ('qgx_head_workspace', C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    ('qgx_head_loss', C.c_int, _HEAD + [C.c_void_p] + _HEAD_SHAPE + [C.c_void_p, C.c_size_t, C.c_void_p]),
    ('qgx_head_grad', C.c_int, _HEAD + [C.c_void_p, C.c_void_p] + _HEAD_SHAPE + [C.c_void_p]),
    ('qgx_head_apply', C.c_int, _HEAD + [C.c_void_p] + _HEAD_SHAPE + [C.c_void_p]),
]

# what include/qgx_flux_train.h declares: 10000 divergence(F) of a flux-form net and its adjoint (tools/train_ops.py)
FLUX_PLANAR, FLUX_ENGINE = 0, 1
_FLUX = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]                     # in, out, B, N, layout, stream
FLUX_TRAIN_SYMBOLS = [
    ('qgx_fluxdiv_forward', C.c_int, _FLUX),
    ('qgx_fluxdiv_backward', C.c_int, _FLUX),
]

# what include/qgx_latent_train.h declares: the latent step of a conditional VAE's training (tools/train_ops.py)
_DRAW = [C.c_uint64, C.c_uint64]                                                              # seed, step
LATENT_TRAIN_SYMBOLS = [
    ('qgx_latent_workspace', C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_size_t)]),
    ('qgx_latent_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + _DRAW + [C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    ('qgx_latent_backward', C.c_int, [C.c_void_p, C.c_void_p] + _DRAW + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                      C.c_void_p]),
]

# what include/qgx_dconv_train.h declares: the discriminator's stride-2 convolution and its two gradients (tools/train_ops.py)
_DCONV = [C.c_int64, C.c_int, C.c_int, C.c_int]                                               # B, N, cin, cout
DCONV_TRAIN_SYMBOLS = [
    ('qgx_dconv2d_workspace', C.c_int, _DCONV + [C.POINTER(C.c_size_t)]),
    ('qgx_dconv2d_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _DCONV + _CONV_WORK),
    ('qgx_dconv2d_backward_data', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _DCONV + _CONV_WORK),
    ('qgx_dconv2d_backward_weight', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _DCONV + _CONV_WORK),
]

# what include/qgx_uconv_train.h declares: the U-Net's circular 3 x 3 / 1 x 1 convolution and its two gradients (tools/train_ops.py)
UCONV_TRAIN_SYMBOLS = [
    ('qgx_uconv2d_workspace', C.c_int, _CONV + [C.POINTER(C.c_size_t)]),
    ('qgx_uconv2d_forward', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
    ('qgx_uconv2d_backward_data', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
    ('qgx_uconv2d_backward_weight', C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + _CONV + _CONV_WORK),
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: the HIP extension is not built. Run '
            '`python -c "import __graft_entry__ as g; g.build()"` (or `make -C '
            'pyqg_generative_amd/csrc`). There is no CPU fallback.')
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so) with the same soname as
    # /opt/rocm's, and this library links against that soname: whichever is loaded first serves both.
    # Load torch's first — torch finds no GPU when it is handed the other runtime.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, res, args in (SYMBOLS + ARCH_SYMBOLS + STATS_SYMBOLS + TRAIN_SYMBOLS + CONV_TRAIN_SYMBOLS + HEAD_TRAIN_SYMBOLS
                            + FLUX_TRAIN_SYMBOLS + LATENT_TRAIN_SYMBOLS + DCONV_TRAIN_SYMBOLS + UCONV_TRAIN_SYMBOLS):
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc):
    if rc != 0:
        raise QgxError(f'qgx error {rc}: {lib.qgx_last_error().decode()}')


def current_stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
