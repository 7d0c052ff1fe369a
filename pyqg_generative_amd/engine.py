"""Thin object wrappers over the C ABI (include/qgx.h).

PyTorch tensors are used as device-memory containers and for the stream only;
all arithmetic happens inside libqgx.so.
"""
import ctypes as C
import numpy as np
import torch

from . import _lib
from ._lib import lib, check

PYQG_DEFAULTS = dict(L=1e6, dt=7200., rek=5.787e-7, delta=0.25, beta=1.5e-11, rd=15000.0,
                     U1=0.025, U2=0.0, H1=500., filterfac=23.6)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Generator:
    """Device-resident generator (CGAN G / CVAE decoder, each optionally with the regression net `net_mean` as a second
    net / GZ mean+var nets / OLSModel's one deterministic net, which takes no latent noise)."""
    KINDS = {'gan': _lib.GEN_GAN, 'vae': _lib.GEN_VAE, 'gz': _lib.GEN_GZ, 'ols': _lib.GEN_OLS, 'ann': _lib.GEN_ANN}
    NOISE_FREE = ('ols', 'ann')

    def __init__(self, kind, nets, x_std, y_std, device=0, force_generic=False):
        """nets: list of dicts with float32 numpy arrays
        conv_w[8], conv_b[8], bn_g[7], bn_b[7], bn_m[7], bn_v[7] (PyTorch layouts).  kind 'gan' also takes the DeepInversion
        U-Net as nets[0] (a weights.unet_from_state_dict / weights.synthetic_unet dict), optionally followed by net_mean.
        A net of another architecture than the shipped one (weights.net_from_state_dict_arch / synthetic_arch: other
        hidden_channels, no BatchNorm, no bias) sends the handle through qgx_generator_create_arch: such nets run the generic
        engine, and the handle is exact f32 only.  force_generic (measurements, tests): the generic engine for every net."""
        from .weights import is_unet, is_shipped_arch
        self.kind = kind
        self.device = device
        self._h = C.c_void_p(0)
        keep = []
        xs = (C.c_float * 2)(*[float(v) for v in np.asarray(x_std, np.float32).reshape(-1)])
        ys = (C.c_float * 2)(*[float(v) for v in np.asarray(y_std, np.float32).reshape(-1)])
        self.x_std = np.asarray(x_std, np.float32).reshape(-1)
        self.y_std = np.asarray(y_std, np.float32).reshape(-1)
        self.unet = bool(nets) and is_unet(nets[0])
        self.n_nets = len(nets)
        if kind == 'ann':
            # ANNModel's stencil network: nets = [weights.ann_from_state_dict dict], x_std / y_std the scalars x_scale, y_scale
            if len(nets) != 1 or self.x_std.size != 1 or self.y_std.size != 1:
                raise ValueError("the 'ann' generator takes one ANN and the scalars x_scale, y_scale")
            a = self._ann_struct(nets[0], keep)
            check(lib.qgx_generator_create_ann(C.byref(a), float(self.x_std[0]), float(self.y_std[0]), device,
                                               C.byref(self._h)))
            self.n_in = 1
            return
        if self.unet:
            if kind != 'gan' or len(nets) > 2:
                raise ValueError("the U-Net generator is a CGAN generator ('gan'), optionally with one regression net")
            u = self._unet_struct(nets[0], keep)
            mean = None
            if len(nets) == 2:
                mean = _lib.qgx_cnn_weights()
                self._cnn_struct(nets[1], mean, keep)
            check(lib.qgx_generator_create_unet(C.byref(u), C.byref(mean) if mean is not None else None, xs, ys, device,
                                                C.byref(self._h)))
        elif force_generic or not all(is_shipped_arch(net) for net in nets):
            arr = (_lib.qgx_cnn_arch * len(nets))()
            for n, net in enumerate(nets):
                self._arch_struct(net, arr[n], keep, force_generic)
            check(lib.qgx_generator_create_arch(self.KINDS[kind], arr, len(nets), xs, ys, device, C.byref(self._h)))
        else:
            arr = (_lib.qgx_cnn_weights * len(nets))()
            for n, net in enumerate(nets):
                self._cnn_struct(net, arr[n], keep)
            check(lib.qgx_generator_create(self.KINDS[kind], arr, len(nets), xs, ys, device, C.byref(self._h)))
        self.n_in = 2 if kind in ('gz', 'ols') else 4

    @staticmethod
    def _arch_struct(net, a, keep, force_generic=False):
        """AndrewCNN dict of any architecture -> qgx_cnn_arch (host pointers into `keep`); absent biases / BatchNorm stay NULL"""
        from .weights import net_arch
        arch = net_arch(net)
        n = len(net['conv_w'])
        if not 2 <= n <= 8:
            raise ValueError(f'an AndrewCNN has 2 ... 8 convolutions, not {n}')
        a.n_layers = n
        a.channels[0] = int(net['conv_w'][0].shape[1])
        for l in range(n):
            a.channels[l + 1] = int(net['conv_w'][l].shape[0])
            a.ksize[l] = int(net['conv_w'][l].shape[-1])
        a.batch_norm, a.bias, a.force_generic = int(bool(arch['batch_norm'])), int(bool(arch['bias'])), int(bool(force_generic))
        a.bn_eps = 1e-5
        for l in range(n):
            cw = np.ascontiguousarray(net['conv_w'][l], dtype=np.float32)
            want = (a.channels[l + 1], a.channels[l], a.ksize[l], a.ksize[l])
            if cw.shape != want:
                raise ValueError(f'conv_w[{l}] has shape {cw.shape}, the layers around it make it {want}')
            keep.append(cw)
            a.conv_w[l] = cw.ctypes.data
            if arch['bias']:
                cb = np.ascontiguousarray(net['conv_b'][l], dtype=np.float32).reshape(a.channels[l + 1])
                keep.append(cb)
                a.conv_b[l] = cb.ctypes.data
        if arch['batch_norm']:
            for l in range(n - 1):
                for field, key in (('bn_gamma', 'bn_g'), ('bn_beta', 'bn_b'), ('bn_mean', 'bn_m'), ('bn_var', 'bn_v')):
                    v = np.ascontiguousarray(net[key][l], dtype=np.float32).reshape(a.channels[l + 1])
                    keep.append(v)
                    getattr(a, field)[l] = v.ctypes.data

    @staticmethod
    def _cnn_struct(net, w, keep):
        w.n_in = int(net['conv_w'][0].shape[1])
        w.n_out = int(net['conv_w'][7].shape[0])
        w.bn_eps = 1e-5
        for i in range(8):
            cw = np.ascontiguousarray(net['conv_w'][i], dtype=np.float32)
            cb = np.ascontiguousarray(net['conv_b'][i], dtype=np.float32)
            keep += [cw, cb]
            w.conv_w[i] = cw.ctypes.data
            w.conv_b[i] = cb.ctypes.data
        for i in range(7):
            for field, key in (('bn_gamma', 'bn_g'), ('bn_beta', 'bn_b'),
                               ('bn_mean', 'bn_m'), ('bn_var', 'bn_v')):
                a = np.ascontiguousarray(net[key][i], dtype=np.float32)
                keep.append(a)
                getattr(w, field)[i] = a.ctypes.data

    @staticmethod
    def _ann_struct(net, keep):
        """weights.ann_from_state_dict dict -> qgx_ann_weights (host pointers into `keep`)"""
        a = _lib.qgx_ann_weights()
        hidden = list(net['hidden'])
        a.stencil_size, a.n_hidden, a.scale_invariant = int(net['stencil_size']), len(hidden), int(bool(net['scale_invariant']))
        for l, h in enumerate(hidden[:4]):
            a.hidden[l] = int(h)
        for l in range(min(len(hidden) + 1, 5)):
            w = np.ascontiguousarray(net['w'][l], dtype=np.float32)
            b = np.ascontiguousarray(net['b'][l], dtype=np.float32)
            keep += [w, b]
            a.w[l], a.b[l] = w.ctypes.data, b.ctypes.data
        return a

    @staticmethod
    def _unet_struct(net, keep):
        """flat DeepInversionGenerator(4, 2) state dict -> qgx_unet_weights (host pointers into `keep`)"""
        from .weights import UNET_UNITS, UNET_UPS

        def ptr(key):
            a = np.ascontiguousarray(net[key], dtype=np.float32)
            keep.append(a)
            return a.ctypes.data
        u = _lib.qgx_unet_weights()
        u.conv32_w, u.conv32_b = ptr('conv32.weight'), ptr('conv32.bias')
        for i, (p, _, _, bn) in enumerate(UNET_UNITS):
            r = u.res[i]
            if bn:
                r.bn_gamma, r.bn_beta = ptr(f'{p}.bn.weight'), ptr(f'{p}.bn.bias')
                r.bn_mean, r.bn_var = ptr(f'{p}.bn.running_mean'), ptr(f'{p}.bn.running_var')
                r.bn2_gamma, r.bn2_beta = ptr(f'{p}.conv.2.weight'), ptr(f'{p}.conv.2.bias')
                r.bn2_mean, r.bn2_var = ptr(f'{p}.conv.2.running_mean'), ptr(f'{p}.conv.2.running_var')
            r.conv_a_w, r.conv_a_b = ptr(f'{p}.conv.1.weight'), ptr(f'{p}.conv.1.bias')
            r.conv_b_w, r.conv_b_b = ptr(f'{p}.conv.4.weight'), ptr(f'{p}.conv.4.bias')
            r.skip_w, r.skip_b = ptr(f'{p}.conv1.weight'), ptr(f'{p}.conv1.bias')
        for i, (p, _) in enumerate(UNET_UPS):
            u.up_w[i], u.up_b[i] = ptr(f'{p}.upsampling.weight'), ptr(f'{p}.upsampling.bias')
        u.conv_end_w, u.conv_end_b = ptr('conv_end.weight'), ptr('conv_end.bias')
        u.bn_eps = 1e-5
        return u

    @property
    def noise_dtype(self):
        """element type of the latent noise z; None for 'ols' and 'ann' (no noise)"""
        if self.kind in self.NOISE_FREE:
            return None
        return torch.float64 if self.kind == 'gz' else torch.float32

    # ---- f16x3 range guard ---------------------------------------------------------------------
    def info(self):
        """What the calibration at construction decided: dict(precision 0|3, ascale_log2, fold, layer_absmax)."""
        p, e, f = C.c_int(0), C.c_int(0), C.c_int(0)
        mx = (C.c_float * 10)()
        check(lib.qgx_generator_info(self._h, C.byref(p), C.byref(e), C.byref(f), mx))
        return dict(precision=p.value, ascale_log2=e.value, fold=f.value, layer_absmax=list(mx))

    def wino_info(self, N=None):
        """the 5x5 layer's 1-D Winograd form: dict(enabled, chosen_by_calibration, calibration_error, N) — at a grid size it
        is the default only if its outputs on calibration inputs OF THAT SIZE stayed within 1e-5 of the exact-f32 kernels' at
        construction (measured at each of 32, 48, 64, 96, 128).  N = None: the 64 x 64 entry"""
        en, au, err = C.c_int(0), C.c_int(0), C.c_float(0)
        if N is None:
            check(lib.qgx_generator_wino_info(self._h, C.byref(en), C.byref(au), C.byref(err)))
        else:
            check(lib.qgx_generator_wino_info_n(self._h, int(N), C.byref(en), C.byref(au), C.byref(err)))
        return dict(enabled=bool(en.value), chosen_by_calibration=bool(au.value), calibration_error=err.value, N=64 if N is None else int(N))

    LAYER2_KERNELS = ('exact-f32', '25-tap', '25-tap split-K', 'winograd', 'winograd, transform under the MFMAs')

    def layer2_kernel(self, B, N, inet=0):
        """index into LAYER2_KERNELS of the kernel the 5x5 layer takes for B members at N x N under the options in force"""
        k = C.c_int(0)
        check(lib.qgx_generator_layer2_kernel(self._h, int(inet), int(B), int(N), C.byref(k)))
        return k.value

    def range_read(self):
        """Synchronise and return (flags, input_absmax) of the range guard since the last read; clears them.
        flags bit l: conv layer l+1 stored an activation beyond the f16 range; bit 31: non-finite forcing."""
        fl, mx = C.c_uint(0), C.c_float(0)
        check(lib.qgx_generator_range_read(self._h, C.byref(fl), C.byref(mx), _stream()))
        return fl.value, mx.value

    def range_ok(self):
        """-> None if every value stayed inside the 16-bit window since the last check, else a description."""
        if self.precision == 0:          # exact-f32 kernels store no 16-bit activations: nothing to read, no synchronisation
            return None
        flags, in_max = self.range_read()
        if flags == 0 and in_max <= 65504.:
            return None
        layers = [l + 1 for l in range(8) if flags >> l & 1]
        return (f'f16x3 generator arithmetic left its range: overflow in conv layer(s) {layers}, '
                f'non-finite forcing: {bool(flags >> 31)}, largest |network input| {in_max:g}')

    def _guarded(self, launch):
        """Run `launch()`; if the 16-bit window was left, switch this generator to the exact-f32 kernels for good
        and run it again.  What the caller receives is inside the 2e-5 (of max|y|) the golden vectors are held to: float32
        error class (1-2e-6) from the 25-tap and exact-f32 kernels, 3-9e-6 where the Winograd form of the 5x5 layer was
        admitted by its calibration at this grid size (bound 1e-5, `wino_info(N)`; `set_option('wino', 0)` turns it off)."""
        out = launch()
        if self.check_range:
            why = self.range_ok()
            if why is not None:
                import warnings
                warnings.warn(why + '; switching this generator to the exact-f32 kernels', RuntimeWarning)
                self.set_option('precision', 0)
                out = launch()
        return out

    check_range = True

    def guarded_loop(self, body):
        """Run `body()` — a loop of many forward launches (Monte-Carlo sampling, minibatches) — with ONE range check
        after it instead of a device-to-host read and a stream synchronisation per launch; if the 16-bit window was left
        anywhere in the loop, switch to the exact-f32 kernels for good and run the whole loop again."""
        if not self.check_range:
            return body()
        self.check_range = False
        try:
            out = body()
            why = self.range_ok()
            if why is not None:
                import warnings
                warnings.warn(why + '; switching this generator to the exact-f32 kernels', RuntimeWarning)
                self.set_option('precision', 0)
                out = body()
        finally:
            del self.check_range            # back to the class default
        return out

    def check_size(self, B, N, inet=-1):
        """ValueError for a grid the kernels of this handle (inet >= 0: of that net alone) do not run — the library's own
        rule (qgx_generator_size_ok: the AndrewCNN kernels take 16, 32, 48, 64, 96, 128 with the shipped options, the U-Net
        32 ... 128), asked here before any buffer is allocated"""
        if inet not in range(-1, self.n_nets) or B < 1:
            return                          # not a question of the grid: the call itself refuses it (QgxError)
        if lib.qgx_generator_size_ok(self._h, int(inet), int(B), int(N)) != 0:
            raise ValueError(lib.qgx_last_error().decode())

    @staticmethod
    def _check_q_out(q, out):
        """ValueError unless q is a contiguous float64 CUDA tensor (B,2,N,N) and `out` (if given) one of the same shape on
        the same device: the library takes raw pointers and no capacities, so a float32 or short `out` would be overrun"""
        if not (isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.is_contiguous()):
            raise ValueError('q must be a contiguous float64 CUDA tensor')
        if q.dim() != 4 or q.shape[0] < 1 or q.shape[1] != 2 or q.shape[2] != q.shape[3]:
            raise ValueError(f'q must be (B, 2, N, N) with a square grid, got {tuple(q.shape)}')
        if out is None:
            return
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == q.device):
            raise ValueError("out must be a CUDA tensor on q's device")
        if out.dtype != torch.float64:
            raise ValueError(f'out must be float64, got {out.dtype}')
        if tuple(out.shape) != tuple(q.shape):
            raise ValueError(f"out must have q's shape {tuple(q.shape)}, got {tuple(out.shape)}")
        if not out.is_contiguous():
            raise ValueError('out must be contiguous')

    def forward(self, q, z=None, demean=True, out=None):
        """q: (B,2,N,N) float64 cuda; z: (B,2,N,N) float32 (float64 for gz; 'ols' and 'ann' take none) -> S (B,2,N,N) float64.
        out: a contiguous float64 CUDA tensor of q's shape to write S into (ValueError otherwise, before anything runs)."""
        self._check_q_out(q, out)
        B, _, N, _ = q.shape
        if self.kind in self.NOISE_FREE:
            if z is not None:
                raise ValueError(f"the {self.kind!r} generator takes no latent noise")
        else:
            assert z is not None and z.is_cuda and z.dtype == self.noise_dtype and z.is_contiguous()
            assert z.numel() == q.numel()
        self.check_size(B, N)
        S = out if out is not None else torch.empty_like(q)

        def launch():
            check(lib.qgx_generator_forward(self._h, _ptr(q), _ptr(z), _ptr(S), B, N, int(bool(demean)), _stream()))
            return S
        return self._guarded(launch)

    def forward_mean(self, q, M, seed=0, member_offset=0, step=0, demean=True, chunk=0, out=None):
        """Deterministic sampling (predict_mean_snapshot for every member): q (B,2,N,N) float64 cuda -> S (B,2,N,N) float64,
        y_std * (mean of M realisations of the generator [+ net_mean]); 'gz': y_std * net_mean, no draws.  Realisation j of
        member b draws the Philox stream (seed, member_offset + b, step + ((j + 1) << 32)) on the device.  chunk: pseudo-members
        (member x realisation) per launch of the generator, 0 = automatic, else at least B.  'ols' and 'ann' have no such
        mode (QgxError).  out: as in forward."""
        self._check_q_out(q, out)
        B, _, N, _ = q.shape
        S = out if out is not None else torch.empty_like(q)

        def launch():
            check(lib.qgx_generator_forward_mean(self._h, _ptr(q), _ptr(S), B, N, int(M), int(chunk), int(bool(demean)),
                                                 int(seed), int(member_offset), int(step), _stream()))
            return S
        return self._guarded(launch)

    def cnn_forward(self, x, inet=0):
        """Raw net forward: x (B,n_in,N,N) float32 -> (B,2,N,N) float32 (net 0: the AndrewCNN or U-Net generator, 4 channels;
        'gz' / 'ols': 2 channels; 'ann': the stencil network on (B,1,N,N) images normalised by x_scale -> (B,1,N,N))."""
        n_in = 2 if (self.kind in ('gz', 'ols') or inet == 1) else 4   # net 1 of a GAN / VAE generator: the regression net
        n_in, n_out = (1, 1) if self.kind == 'ann' else (n_in, 2)
        B, _, N, _ = x.shape
        self.check_size(B, N, inet)
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == n_in
        B, _, N, _ = x.shape
        y = torch.empty((B, n_out, N, N), dtype=torch.float32, device=x.device)

        def launch():
            check(lib.qgx_cnn_forward(self._h, inet, _ptr(x), _ptr(y), B, N, _stream()))
            return y
        return self._guarded(launch)

    def set_option(self, name, value):
        check(lib.qgx_generator_set_option(self._h, name.encode(), int(value)))
        if name in ('precision', 'auto'):
            self._precision = None

    @property
    def precision(self):
        """arithmetic of the kernels in use: 0 exact f32, 3 f16x3 (cached: asked after every guarded launch)"""
        if getattr(self, '_precision', None) is None:
            self._precision = self.info()['precision']
        return self._precision

    def profile(self, layer):
        """Bracket every launch of conv layer `layer` (0..7; -1 = off) with HIP events."""
        check(lib.qgx_generator_profile(self._h, int(layer)))

    def profile_read(self):
        """-> (summed kernel milliseconds, launches) since the last read."""
        ms, n = C.c_double(0), C.c_int64(0)
        check(lib.qgx_generator_profile_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self._h:
            lib.qgx_generator_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EnsembleEngine:
    """B independent two-layer QG members resident on one GPU."""

    def __init__(self, nx=64, n_members=1, device=0, plan_only=False, **params):
        """plan_only: an FFT plan of the grid for rfft2 / irfft2 (tools/operators.py::Dev) — tables and work space, no
        model state, a tenth of the device memory and of the creation time of a model"""
        cfg = _lib.qgx_config()
        cfg.plan_only = int(bool(plan_only))
        p = dict(PYQG_DEFAULTS)
        for k, v in params.items():
            if k not in p:
                raise TypeError(f'unknown model parameter {k!r}')
            p[k] = v
        cfg.nx, cfg.n_members, cfg.device = int(nx), int(n_members), int(device)
        for k, v in p.items():
            setattr(cfg, k, float(v))
        self.params = p
        self.N, self.NK, self.B = int(nx), int(nx) // 2 + 1, int(n_members)
        self.device = torch.device('cuda', device)
        self._h = C.c_void_p(0)
        self._generators = []           # generators used by step(): their range guard is read at status time
        self.step_calls = 0             # qgx_step calls made through step() (a fused run makes few, a host plug-in one per step)
        check(lib.qgx_create(C.byref(cfg), C.byref(self._h)))

    # ---- tables -------------------------------------------------------------------
    def table(self, which):
        N, NK = self.N, self.NK
        shape = {_lib.T_FILTR: (N, NK), _lib.T_WV2: (N, NK), _lib.T_A: (2, 2, N, NK),
                 _lib.T_KK: (NK,), _lib.T_LL: (N,)}[which]
        out = np.empty(shape, dtype=np.float64)
        check(lib.qgx_get_table(self._h, which, out.ctypes.data_as(C.c_void_p)))
        return out

    # ---- state --------------------------------------------------------------------
    def _real(self):
        return torch.empty((self.B, 2, self.N, self.N), dtype=torch.float64, device=self.device)

    def _spec(self):
        return torch.empty((self.B, 2, self.N, self.NK), dtype=torch.complex128, device=self.device)

    def get(self, field, noise_dtype=None):
        """copy of a state field.  F_Z (the latent noise) has the element type of the generator last stepped with — float32
        for GAN / VAE, float64 for GZ — which the library reports (qgx_field_bytes); a `noise_dtype` that contradicts it is
        refused rather than handed a buffer of the wrong size"""
        if field in (_lib.F_Q, _lib.F_U, _lib.F_V, _lib.F_S, _lib.F_P):
            out = self._real()
        elif field == _lib.F_Z:
            nbytes = int(lib.qgx_field_bytes(self._h, field))
            dtype = torch.float64 if nbytes == self.B * 2 * self.N * self.N * 8 else torch.float32
            if noise_dtype is not None and noise_dtype != dtype:
                raise ValueError(f'the latent noise of this model is {dtype}, not {noise_dtype}')
            out = torch.empty((self.B, 2, self.N, self.N), dtype=dtype, device=self.device)
        else:
            out = self._spec()
        # qgx_get takes no capacity: the buffer must be exactly what the library will write
        nbytes = int(lib.qgx_field_bytes(self._h, field))
        assert out.numel() * out.element_size() == nbytes, (field, out.numel() * out.element_size(), nbytes)
        check(lib.qgx_get(self._h, field, _ptr(out), _stream()))
        return out

    def set_q(self, q):
        q = torch.as_tensor(q, dtype=torch.float64, device=self.device).contiguous()
        assert tuple(q.shape) == (self.B, 2, self.N, self.N), q.shape
        check(lib.qgx_set_q(self._h, _ptr(q), _stream()))
        torch.cuda.current_stream().synchronize()     # q may be a temporary

    def set_qh(self, qh):
        qh = torch.as_tensor(qh, dtype=torch.complex128, device=self.device).contiguous()
        assert tuple(qh.shape) == (self.B, 2, self.N, self.NK), qh.shape
        check(lib.qgx_set_qh(self._h, _ptr(qh), _stream()))
        torch.cuda.current_stream().synchronize()

    def invert(self):
        check(lib.qgx_invert(self._h, _stream()))

    @property
    def tc(self):
        return int(lib.qgx_step_count(self._h))

    @property
    def run_kernel_state(self):
        """256 x 256 grids: 1 = unparameterized runs of steps execute as single persistent launches, -1 = not on this
        device (three launches per step), 0 = not decided yet / other grid"""
        return int(lib.qgx_run_kernel_state(self._h))

    def reset_time(self):
        check(lib.qgx_reset_time(self._h))

    def set_option(self, name, value):
        """kernel-path switch of this model (include/qgx.h::qgx_set_option): same results, different fusion / tiling"""
        check(lib.qgx_set_option(self._h, name.encode(), int(value)))

    # ---- molecular viscosity (the reference's Laplace(nu, PV), tools/simulate.py:207-225) ----
    def set_viscosity(self, nu, PV=False):
        """nu lap zeta (PV=False) or nu lap q (PV=True) as a term of every later step's tendency, evaluated inside the step
        kernels (qgx_set_viscosity).  nu: a scalar for all members, or one value per member (a viscosity sweep is one
        ensemble); None switches the term off.  Takes effect at the next step; the AB history is kept."""
        if nu is None:
            check(lib.qgx_set_viscosity(self._h, None, 0, _stream()))
            return
        a = np.asarray(nu, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(self.B, float(a))
        if a.shape != (self.B,):
            raise ValueError(f'nu must be a scalar or one value per member ({self.B}), got shape {a.shape}')
        a = np.ascontiguousarray(a)
        check(lib.qgx_set_viscosity(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), int(bool(PV)), _stream()))

    @property
    def viscosity(self):
        """None while the term is off, else (nu per member as a numpy array, PV)"""
        a = np.zeros(self.B, dtype=np.float64)
        pv = C.c_int(0)
        n = lib.qgx_get_viscosity(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), C.byref(pv))
        if n < 0:
            check(n)
        return (a, bool(pv.value)) if n > 0 else None

    # ---- Jansen-Held backscatter closure (pyqg's BackscatterBiharmonic; the reference's physical parameterizations) ----
    def _per_member(self, x, name):
        a = np.asarray(x, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(self.B, float(a))
        if a.shape != (self.B,):
            raise ValueError(f'{name} must be a scalar or one value per member ({self.B}), got shape {a.shape}')
        return np.ascontiguousarray(a)

    def set_backscatter(self, smag, back=None, eps=1e-32):
        """BackscatterBiharmonic(smag, back, eps) as the q-parameterization of every later plain step, evaluated on the
        device from the current state (qgx_set_backscatter).  smag, back: scalars for all members, or one value per member
        (a (C_S, C_B) sweep is one ensemble); smag None switches the closure off.  Takes effect at the next step."""
        if smag is None:
            check(lib.qgx_set_backscatter(self._h, None, None, 0.0, _stream()))
            return
        if back is None:
            raise ValueError('set_backscatter needs back_constant with smag_constant')
        cs, cb = self._per_member(smag, 'smag'), self._per_member(back, 'back')
        dp = C.POINTER(C.c_double)
        check(lib.qgx_set_backscatter(self._h, cs.ctypes.data_as(dp), cb.ctypes.data_as(dp), float(eps), _stream()))

    @property
    def backscatter(self):
        """None while the closure is off, else (smag per member, back per member, eps)"""
        cs, cb = np.zeros(self.B, dtype=np.float64), np.zeros(self.B, dtype=np.float64)
        eps = C.c_double(0.0)
        dp = C.POINTER(C.c_double)
        n = lib.qgx_get_backscatter(self._h, cs.ctypes.data_as(dp), cb.ctypes.data_as(dp), C.byref(eps))
        if n < 0:
            check(n)
        return (cs, cb, eps.value) if n > 0 else None

    def backscatter_forcing(self, ratio=False):
        """The closure of the current state: S (B,2,N,N) float64 device tensor; ratio=True: (S, R) with the energy ratio
        R (B).  Changes no state (qgx_backscatter_forcing)."""
        S = self._real()
        R = torch.empty((self.B,), dtype=torch.float64, device=self.device) if ratio else None
        # S has the layout of a real field: the library's own count for one (qgx_field_bytes), not this class's arithmetic
        assert S.numel() * S.element_size() == int(lib.qgx_field_bytes(self._h, _lib.F_Q)) and (R is None or R.numel() == self.B)
        check(lib.qgx_backscatter_forcing(self._h, _ptr(S), _ptr(R), _stream()))
        return (S, R) if ratio else S

    def status(self):
        """-> (KE[B], CFL[B]) as pyqg's _print_status computes them (from the last inversion)."""
        out = torch.empty((self.B, 2), dtype=torch.float64, device=self.device)
        # out_dev[2*b + 0] = KE, [2*b + 1] = CFL: two doubles per member of the handle (the library exports no size query
        # for this; the line states the contract next to the allocation, it cannot fail by itself)
        assert out.numel() == 2 * self.B
        check(lib.qgx_status_ke_cfl(self._h, _ptr(out), _stream()))
        out = out.cpu().numpy()
        self.check_generators()
        return out[:, 0], out[:, 1]

    def check_generators(self):
        """The fused step cannot re-run a forcing after the fact: a generator that left its 16-bit window since the
        last check has corrupted the members' state, so this raises (status / snapshot cadence of the run loop)."""
        self._generators = [g for g in self._generators if g._h]        # a closed generator has nothing left to report
        for g in self._generators:
            why = g.range_ok() if g.check_range else None
            if why is not None:
                raise FloatingPointError(why + "; re-run with Generator.set_option('precision', 0)")

    # ---- time-averaged diagnostics --------------------------------------------------
    def diag_config(self, start_step, every):
        check(lib.qgx_diag_config(self._h, int(start_step), int(every)))

    @property
    def diag_count(self):
        return int(lib.qgx_diag_count(self._h))

    def diag_reset(self):
        check(lib.qgx_diag_reset(self._h))

    def diag(self, name):
        """time mean of diagnostic `name` per member: (B,2,N,NK) for KEspec/Ensspec else (B,N,NK) (device tensor)"""
        i = _lib.DIAGS.index(name)
        shape = (self.B, 2, self.N, self.NK) if i < 2 else (self.B, self.N, self.NK)
        out = torch.empty(shape, dtype=torch.float64, device=self.device)
        # enum qgx_diag: (B,2,N,N/2+1) real for the first two, (B,N,N/2+1) for the rest, i.e. as many doubles as a spectral
        # field has complex values, or half of that, by the library's own count of a spectral field
        nspec = int(lib.qgx_field_bytes(self._h, _lib.F_QH)) // 16
        assert out.numel() == (nspec if i < 2 else nspec // 2), (name, out.numel(), nspec)
        check(lib.qgx_diag_get(self._h, i, _ptr(out), _stream()))
        return out

    # ---- stepping -----------------------------------------------------------------
    SAMPLINGS = {'AR1': _lib.SAMPLING_AR1, 'constant': _lib.SAMPLING_CONSTANT, 'deterministic': _lib.SAMPLING_DETERMINISTIC}

    def step(self, nsteps=1, generator=None, sampling='AR1', nsteps_decor=1, weight=1.0, seed=0,
             member_offset=0, z_external=None, forcing=None, demean=None, refresh_diag=True, n_mean=100):
        """sampling='deterministic': every step applies the mean of `n_mean` generator realisations for the current PV
        (nsteps_decor is not used; the latent noise and the sampler state stay as they are)"""
        p = None
        keep = []
        if generator is not None or forcing is not None:
            p = _lib.qgx_param()
            p.gen = generator._h if generator is not None else None
            if generator is not None:
                generator.check_size(self.B, self.N)
            if generator is not None and generator not in self._generators:
                self._generators.append(generator)
            p.sampling = self.SAMPLINGS[sampling]
            p.nsteps = int(nsteps_decor)
            p.n_mean = int(n_mean)
            p.weight = float(weight)
            p.seed = int(seed)
            p.member_offset = int(member_offset)
            if z_external is not None:
                assert z_external.is_cuda and z_external.is_contiguous()
                keep.append(z_external)
                p.z_external_dev = z_external.data_ptr()
            if forcing is not None:
                assert forcing.is_cuda and forcing.dtype == torch.float64 and forcing.is_contiguous()
                keep.append(forcing)
                p.forcing_dev = forcing.data_ptr()
            if demean is None:
                demean = generator is not None
            p.demean = int(bool(demean))
        check(lib.qgx_step(self._h, int(nsteps), C.byref(p) if p is not None else None,
                           int(bool(refresh_diag)), _stream()))
        self.step_calls += 1
        if keep:
            torch.cuda.current_stream().synchronize()

    def step_streams(self, generator=None, sampling='AR1'):
        """1 or 2: the internal streams `step` advances this ensemble on with `generator` attached (qgx_step_streams)"""
        if generator is None:
            return 1
        p = _lib.qgx_param()
        p.gen = generator._h
        p.sampling = self.SAMPLINGS[sampling]
        return int(lib.qgx_step_streams(self._h, C.byref(p)))

    def close(self):
        if self._h:
            lib.qgx_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
