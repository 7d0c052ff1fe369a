/* qgx_arch.h — the architecture-generic AndrewCNN creator of the qgx C ABI.  Included by qgx.h (which declares qgx_generator,
 * the generator kinds and every entry point such a handle serves); not meant to be included on its own. */
#ifndef QGX_ARCH_H
#define QGX_ARCH_H

/* AndrewCNN nets of any architecture the reference's AndrewCNN(n_in, n_out, batch_norm, bias, div, hidden_channels) builds
 * (cnn_tools.py:125-176): n_layers = len(hidden_channels) + 1 convolutions, 2 ... 8; channels[0] = n_in, channels[1 ..
 * n_layers - 1] the hidden widths, each 1 ... 256 and free of any multiple (the engine pads: K to 8, output tiles to 32),
 * channels[n_layers] = 2, or 4 for a flux-form net (div=True, see above); ksize[l] = 5 or 3 for convolution l (the
 * reference: 5, 5, 3, 3, ...; the last one 3).  batch_norm = 0: the blocks are Conv -> ReLU (state-dict keys conv.{2l}.*),
 * the bn_* pointers are not read; bias = 0: Conv2d(bias=False), conv_b is not read.  With a flag set, every pointer it
 * governs must be non-NULL for l < n_layers (BatchNorm: l < n_layers - 1).  force_generic != 0 (A/B measurements and
 * tests): the generic engine even for the shipped architecture.
 * kind, n_nets, channels[0] and flux form per kind are those of qgx_generator_create; each net is described on its own (the
 * reference builds a GAN's / VAE's net_mean with the default widths whatever hidden_channels says, cgan_regression.py:60).
 * Every out-of-range field and every NULL pointer a flag requires is refused with QGX_ERR_INVALID and a message naming
 * the field, before any allocation or device call.
 * If every net is the shipped architecture ([128, 64, 32, 32, 32, 32, 32], kernels 5, 5, 3, ..., BatchNorm, bias) the handle
 * is the one qgx_generator_create makes: same kernels, calibration, f16x3 and Winograd included, bitwise equal outputs.
 * Otherwise the nets of another architecture run the generic engine (conv_generic.hip: exact-f32 MFMA kernels with run-time
 * channel counts, float32-class as precision 0), shipped-architecture nets beside them the exact-f32 kernels, and the handle
 * is exact f32 only, as a U-Net handle: qgx_generator_info reports precision 0, _wino_info off, and
 * qgx_generator_set_option refuses everything but precision 0.  It serves every entry point a qgx_generator_create handle
 * serves (qgx_generator_forward, _forward_mean, qgx_cnn_forward, qgx_step with every sampling), at N = 16, 32, 48, 64, 96,
 * 128 and every member count; other N are refused as above. */
typedef struct qgx_cnn_arch {         /* host pointers, float32, PyTorch layouts */
    int32_t n_layers;                 /* convolutions, 2 ... 8                                        */
    int32_t channels[9];              /* [0] n_in (2 | 4), [n_layers] 2, or 4: flux form              */
    int32_t ksize[8];                 /* 5 | 3                                                        */
    int32_t batch_norm, bias;         /* 0 | 1                                                        */
    int32_t force_generic;            /* 0; != 0: the generic engine for the shipped architecture too */
    const float *conv_w[8];           /* (channels[l + 1], channels[l], k, k)                         */
    const float *conv_b[8];           /* (channels[l + 1]); bias = 0: not read                        */
    const float *bn_gamma[7], *bn_beta[7], *bn_mean[7], *bn_var[7];   /* batch_norm = 0: not read     */
    float bn_eps;                     /* 1e-5                                                         */
} qgx_cnn_arch;
int qgx_generator_create_arch(int kind, const qgx_cnn_arch *nets, int n_nets, const float x_std[2],
                              const float y_std[2], int device, qgx_generator **out);

#endif
