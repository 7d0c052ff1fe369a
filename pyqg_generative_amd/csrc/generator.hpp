// The generator handle and the seam between its two translation units (private to csrc/).
//
// generator.hip owns the handle: lifecycle, workspaces, the model-independent kernels around a net (input assembly,
// output scaling, range words, moments), generator_forward's dispatch over the model kinds, and the C ABI that is not
// AndrewCNN-specific.  conv.hip owns the AndrewCNN engine: kernels, weight packers, launchers, cnn_forward, the range
// and Winograd calibration, the kernel-selection options (every opt_* field below; the variants that lost
// their measurements are no longer carried: DESIGN.md 3.2), the per-layer profiler, and the C
// ABI that only makes sense for AndrewCNN nets.  Between them: the functions declared at the end of this file.
// The U-Net and the ANN are opaque back ends of the same kind (common.hpp: UNet, Ann).
#pragma once
#include "common.hpp"

namespace qgx {

struct LastWeights { float w[3 * 3 * 32 * 2]; };   // [tap][c][2], passed BY VALUE: kernarg -> scalar loads

struct LayerHost {
    int cin, cout, ks, coutp, cc, ngroups;
    // generic engine (conv_generic.hip): K per tap = the input channels padded to 8 (the NHWC pixel stride of the layer's
    // input; 8 for the planar first layer), and the channels stored per output pixel (cout padded to 8; the last layer: cout)
    int cinp = 0, cstore = 0;
    LastWeights wv_host[2];   // last layer, VALU kernel layout (kernel argument): output channels (0, 1), and (2, 3) of a flux-form net
    float *wl16 = nullptr;                   // k_conv3 layout [chunk][tap][g8][h][coutp][4], 16-channel chunks
    float *w = nullptr, *w32 = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr;   // w: 16-ch chunks (or planar), w32: 32-ch chunks
    void *wh = nullptr;                      // conv_half.hpp layout: f16 hi/lo
    float wh_unscale = 1.f;                  // 2^-s of the power-of-two weight pre-scale
    // layer 2 with layer 1's BatchNorm folded in (W' = W alpha[c_in], b' = b + sum W beta'[c_in]; exact under circular
    // padding): layer 1 then stores ReLU output, half of which is exactly zero -> a sparser MFMA operand
    void *whF = nullptr; float whF_unscale = 1.f; float *biasF = nullptr;
    // layer 2 as a 1-D Winograd convolution F(4, 5) along x (conv_wino.hpp): transformed weights, [0] plain, [1] with layer
    // 1's BatchNorm folded in; per-position 2^-s of the power-of-two pre-scale
    void *ww[2] = {nullptr, nullptr};
    float ww_unscale[2][8] = {{1, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 1}};
    float *ones = nullptr, *zeros = nullptr; // layer 1: identity BatchNorm for the folded variant
    void *whf = nullptr;                     // first layer, f16x3: [step][part][h][128][8] f16
    float whf_unscale = 1.f;
    // every device allocation of a layer: a packer that adds a layout adds its pointer here
    void free_device() {
        void *ptrs[] = {w, w32, wl16, bias, scale, shift, wh, whF, biasF, ww[0], ww[1], ones, zeros, whf};
        for (void *p : ptrs) if (p) (void)hipFree(p);
    }
};
struct NetHost {
    int n_in, n_out;       // n_out = 4: a flux-form net (AndrewCNN(n_in, 2, div=True)): the last convolution writes four fluxes
    LayerHost L[8];
    // qgx_generator_create_arch: any other architecture than the shipped one with BatchNorm and bias runs the generic engine
    // (conv_generic.hip) on L[0 .. n_layers - 1]; the shipped one keeps generic = false and every layout cnn_pack_net makes
    bool generic = false;
    int n_layers = 8, batch_norm = 1, bias = 1;
    // channels per pixel of the widest activation this net stores in actA (which = 0: layers 1, 3, ...) / actB (layers 2, 4, ...)
    int act_width(int which) const {
        if (!generic) return which ? 64 : 128;
        int w = 8;
        for (int l = which; l < n_layers - 1; l += 2) w = L[l].cstore > w ? L[l].cstore : w;
        return w;
    }
    bool flux() const { return n_out == 4; }
    int y_channels() const { return flux() ? 2 : n_out; }     // channels of AndrewCNN.forward's output
};

// activation buffers of one ensemble (or half-ensemble), grown on demand, outside any captured region
struct Workspace {
    size_t cap_elems = 0;          // capacity in units of B*N*N pixels
    float *actA = nullptr, *actB = nullptr, *X = nullptr, *Y0 = nullptr, *Y1 = nullptr;
    float *F = nullptr;            // fluxes (B, 4, N, N) of a flux-form net, between its last convolution and the divergence;
                                   // allocated only for handles that hold such a net
    float *part = nullptr;         // split-K partial sums of the small-ensemble path
    size_t part_elems = 0;
    void free_activations() {      // everything generator_reserve allocates
        for (float **p : {&actA, &actB, &X, &Y0, &Y1, &F}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        cap_elems = 0;
    }
    double *mean_acc = nullptr;    // deterministic sampling: float64 sum over realisations (B, 2, N, N), kept across the chunks
    size_t mean_elems = 0;
    void free_mean() {
        if (mean_acc) (void)hipFree(mean_acc);
        mean_acc = nullptr; mean_elems = 0;
    }
    void free_part() {
        if (part) (void)hipFree(part);
        part = nullptr; part_elems = 0;
    }
};

}  // namespace qgx

struct qgx_generator {
    int kind, device, n_nets;
    int generic = 0;               // qgx_generator_create_arch with a net of the generic engine: exact f32 only, as unet / ann
    int actw[2] = {128, 64};       // channels per pixel of actA / actB: the widest layer of the handle's nets (generator_reserve)
    qgx::UNet *unet = nullptr;     // qgx_generator_create_unet: net 0 is the DeepInversion U-Net (unet.hip), its workspace is actA
    qgx::Ann *ann = nullptr;       // qgx_generator_create_ann: the pointwise stencil network (ann.hip); its only workspace is Y0
    qgx::NetHost nets[2];
    float x_std[2], y_std[2];
    // ws[1]: the other half of an ensemble stepped in halves on two streams (model.hip::qgx_step);
    // generator_select_workspace chooses the active one
    qgx::Workspace ws[2];
    int ws_active = 0;
    qgx::Workspace &work() { return ws[ws_active]; }
    // f16x3 range guard (conv_half.hpp::range_guard): [0] sticky flags — bit l: layer l stored a value beyond the f16
    // range, bit 31: non-finite forcing; [1] bits of the largest |network input| seen
    unsigned *range_dev = nullptr;

    // ---- AndrewCNN state: read and written by conv.hip only ----
    // kernel variant selection (qgx_generator_set_option; defaults = fastest measured)
    int opt_cc = 32, opt_last_valu = 1, opt_first_split = 2, opt_v3 = -1, opt_small = 1;
    unsigned long long *stamps = nullptr;   // diagnostic builds only
    int stamp_layer = -1;
    int opt_h2_tw32 = 0;           // 5x5 layer at 64 x 64: 16-row x 32-column tiles instead of 8 full rows
    int opt_h2_x96 = 1;            // 3x3 layers at 96 x 96 as 8-wave workgroups on 16-row x 32-column tiles (-1.4 % of the step at 32 members, -3.6 % at 64)
    int opt_h2_w8_min96 = 1024;    // 5x5 layer at 96 x 96: minimum tile count for the 8-wave x-tiled kernel
    int opt_h2_w8 = 3;             // k_convh2 as one 8-wave workgroup per CU: bit 0 the 5x5 layer, bit 1 the 3x3 layers (64 x 64)
    int opt_prio_alt = 1;          // k_convh2 with two workgroups per CU: alternate their wave priority per tile
    int opt_h2_grid = 0;           // k_convh2: persistent workgroups per launch (0 = one or two per CU by LDS size)
    int opt_wino = 2;              // f16x3: the 5x5 layer as a 1-D Winograd convolution F(4, 5) along x (k_convw): 0 never, 1 on every
                                   //   specialised grid, 2 = per grid size, where calibrate_wino() admitted it
    int auto_wino_n[5] = {0, 0, 0, 0, 0};            //   ... what calibrate_wino() decided for N = 32, 48, 64, 96, 128 and the errors it measured
    float wino_err_n[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int opt_wino2 = 1;             //   ... as k_convw2 (conv_wino2.hpp: transform under the MFMAs, bit-identical) where that kernel exists; 0 = k_convw
    int opt_h2_rows96 = 0;         // 3x3 layers at 96 x 96: tile rows, 0 = by tile-count quantisation, 12 (6 waves), 16 (8 waves)
    int opt_wino_rows64 = 0;       //   ... its tile shape at 64 x 64, 128 x 128 and 32 x 32: 0 = by tile-count quantisation, 4 = the half-height
                                   //   shape (4 x 64 tiles; 8 x 32 at 32 x 32), 8 = the full one
    int opt_wino_rows96 = 0;       //   ... its tile rows at 96 x 96: 0 = by tile-count quantisation (wino_rows), 12, 16
    int opt_wino_min_tiles = 48;   //   ... from this many full-height tiles on (measured crossovers, bench_tools/ab_conv.py: with the half-height
                                   //   shapes the Winograd kernel is ahead of the 25-tap kernels from 6 members at 64 x 64, 4 at 96 x 96, 24 at 32 x 32)
    int opt_fold = 1;              // f16x3: layer 1 stores ReLU output, its BatchNorm is folded into layer 2's weights
    int opt_part_max_tiles = 96;   // f16x3: split K on the wide layers below this many quarter-height tiles (crossover against the Winograd
                                   //   layer's half-height shape: 6 members at 64 x 64 — forward 166.8 -> 158.0 us —, 4 at 96 x 96: 217.5 -> 184.3)
    int opt_last_rows = 0;         // VALU last layer: rows per workgroup (0 = automatic)
    int opt_half_min_tiles = 1;
    int opt_tiny_pairs = 7;        // tiny ensembles at 64 x 64 (split-K path): bit 0 layers (7, 8), bit 1 layers (5, 6), bit 2 layers (3, 4) as ONE fused launch on 2-row strips
    int opt_small_tiles = 1;       // 64 x 64, at most 4 members: half-height tiles (small_tiles())
    int opt_fuse96 = 2;            // ... at 96 x 96 (4-row strips): bit 0 (5,6), 1 (7,8)
    int opt_fuse = 3;              // f16x3, 64x64: 3x3 layers fused pairwise (k_convh_pair): bit 0 (5,6), 1 (7,8), 2 (3,4)
    int opt_pair = 1;              // 3x3 k_convh2: fetch both 64-byte halves of a pixel's 128-byte line together
    int opt_member_chunk = 0;      // 16-bit path: members per sub-batch (0 = whole ensemble)
    int opt_first_h = 1;           // f16x3 path: first layer on the 16-bit cores too (0: exact-f32 MFMA first layer)
    int opt_precision = 3;         // 0 = exact f32 MFMA, 3 = f16x3 split (f32-class accuracy; the default on the grids
                                   // k_convh2 is specialised for, see half_path_ok)
    float opt_ascale = 1.f;        // power-of-two pre-scale of stored 16-bit activations (chosen by calibrate())
    unsigned *calib_dev = nullptr; // calibration only: per-layer max |activation| of the exact-f32 evaluation
    float calib_max[10] = {0};     // [0..6] stored (post-BatchNorm) activations, [8] layer 1 before its BatchNorm
    int auto_precision = 3, auto_fold = 1, auto_ascale_log2 = 0;   // what calibrate() decided
    // optional per-layer timing with HIP events on the launch stream (bench.py roofline leg)
    int prof_layer = -1;
    int prof_every = 1;                 // bracket every n-th launch of the profiled layer ("prof_every" option)
    long prof_seen = 0;
    std::vector<hipEvent_t> prof_ev;    // pairs (start, stop)
    size_t prof_used = 0;
};

namespace qgx {

// ---- conv.hip, called by generator.hip ----
int cnn_pack_net(NetHost &net, const qgx_cnn_weights *w);    // shapes of the eight layers and every weight layout, on the device
void cnn_free_net(NetHost &net);
int cnn_calibrate(qgx_generator *g);          // range calibration, then the Winograd layer's per grid size (once, at creation)
void cnn_exact_f32_only(qgx_generator *g);    // U-Net and ANN handles: a net_mean beside them takes the exact-f32 kernels
// AndrewCNN.forward: x planar (B,n_in,N,N) -> y planar (B,2,N,N); a flux-form net's fluxes go through the workspace's F and
// the divergence kernel (fluxdiv.hip), so that every caller sees the one output shape
int cnn_forward(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N, hipStream_t st);
// whether cnn_forward's launchers take B members at N x N under the options in force (no HIP call)
bool cnn_size_ok(const qgx_generator *g, const NetHost &net, int B, int N);

// ---- conv_generic.hip: AndrewCNN nets of any admitted architecture (qgx_cnn_arch), exact-f32 MFMA kernels with run-time
// channel counts; called by generator.hip (check, pack) and conv.hip (the dispatch of cnn_forward / cnn_size_ok)
int cnn_arch_check(const qgx_cnn_arch *a, int inet);          // every field and required pointer; no HIP call, no allocation
bool cnn_arch_is_shipped(const qgx_cnn_arch *a);              // [128, 64, 32 x 5], kernels 5, 5, 3 ..., BatchNorm, bias, not forced
void cnn_arch_to_weights(const qgx_cnn_arch *a, qgx_cnn_weights *w);     // ... such a descriptor as cnn_pack_net takes it
int cnn_pack_net_arch(NetHost &net, const qgx_cnn_arch *a);
int cnng_convs(qgx_generator *g, const NetHost &net, const float *x, float *y, int B, int N, hipStream_t st);
bool cnng_size_ok(const NetHost &net, int B, int N);
// ... one convolution with the bias alone, NHWC in and out, outside any handle: the layer operation of conv_train.hip
bool convg_linear_ok(int64_t B, int N, int coutp, int ks);       // no HIP call
int launch_convg_linear(const float *in, float *out, const float *w, const float *bias, int B, int N, int cinp, int coutp,
                        int cstore, int ks, hipStream_t st);
// conv.hip helpers the generic launchers share
int ensure_dynamic_lds(const void *kern, int bytes);
int choose_rows(int N);

// One launch of a conv-family kernel (conv.hip, conv_generic.hip, conv_wino2.hip): raises the kernel's dynamic-LDS cap
// (ensure_dynamic_lds: once per kernel, device and host thread), launches, and reports a refused launch.  Tile shapes,
// argument structs and ProfScope stay with the launchers.
template <typename... Params, typename... Args>
int launch_conv_kernel(void (*kern)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
    if (lds > 0) { if (const int rc = ensure_dynamic_lds((const void *)kern, (int)lds)) return rc; }
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    QGX_HIP(hipGetLastError());
    return QGX_OK;
}
// at most `cap` persistent workgroups, never more than total_tiles
inline int persistent_grid(int cap, int total_tiles) { return cap < total_tiles ? cap : total_tiles; }

// The profiler's bracket around one launcher: begin() records the start event of a pair when `layer` is the profiled one,
// and the stop event is recorded when the scope is left on ANY path, so that qgx_generator_profile_read never meets a
// start event whose stop event was not recorded.
struct ProfScope {
    hipEvent_t stop = nullptr;
    hipStream_t st = nullptr;
    int begin(qgx_generator *g, int layer, hipStream_t stream) {
        if (g->prof_layer != layer) return QGX_OK;
        // an event pair costs ~6 us of idle GPU on each side of the kernel: bracket every prof_every-th launch only
        if (g->prof_every > 1 && (g->prof_seen++ % g->prof_every) != 0) return QGX_OK;
        if (g->prof_used + 2 > g->prof_ev.size()) {
            for (int i = 0; i < 2; ++i) {
                hipEvent_t e;
                QGX_HIP(hipEventCreate(&e));
                g->prof_ev.push_back(e);
            }
        }
        QGX_HIP(hipEventRecord(g->prof_ev[g->prof_used], stream));
        stop = g->prof_ev[g->prof_used + 1];
        st = stream;
        g->prof_used += 2;
        return QGX_OK;
    }
    ~ProfScope() { if (stop) (void)hipEventRecord(stop, st); }
};

// ---- fluxdiv.hip: y (B,2,N,N) = 10000 div F, F (B,4,N,N) = [fx1, fx2, fy1, fy2], float32 spectral, one kernel ----
bool fluxdiv_size_ok(int N);
int fluxdiv_prepare();                         // once per handle with a flux-form net, outside any captured region
int fluxdiv_forward(const float *F, float *y, int B, int N, hipStream_t st);

// ---- generator.hip, called by conv.hip ----
int generator_reserve(qgx_generator *g, int B, int N);       // the active workspace's activation buffers for B members at N x N
int generator_reserve_part(qgx_generator *g, size_t elems);  // ... and its split-K buffer (floats)
// the running maximum of |x| (a NaN counts as infinity) into range[1], as float bits
void launch_absmax(const float *x, size_t n, unsigned *range, hipStream_t st);

// largest |x| of a tensor: non-negative floats order like their bit patterns
__device__ __forceinline__ float abs_or_inf(float x) { return x != x ? __uint_as_float(0x7f800000u) : fabsf(x); }

}  // namespace qgx
