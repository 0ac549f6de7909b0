"""Host runtime over the C ABI: one Context per GPU, torch-ROCm tensors as device-memory containers.

Nothing here computes: every numeric operation is a call into libsr355.so on the tensor's device
and the current torch stream.  Errors coming back over the ABI are raised as the exception types
the reference raises at the same call sites (ValueError / RuntimeError / KeyError / MemoryError).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


class Sr355Error(RuntimeError):
    pass


_EXC = {L.SR_ERR_INVALID: ValueError, L.SR_ERR_HIP: Sr355Error, L.SR_ERR_OOM: MemoryError,
        L.SR_ERR_STATE: RuntimeError, L.SR_ERR_NAME: KeyError, L.SR_ERR_CAPACITY: ValueError}

_TORCH2DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.uint8: L.DTYPE_U8}
_DT2TORCH = {v: k for k, v in _TORCH2DT.items()}


def dtype_code(dt):
    if isinstance(dt, str):
        dt = {"f32": torch.float32, "float32": torch.float32, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16,
              "u8": torch.uint8}[dt]
    return _TORCH2DT[dt]


def _fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _np32(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _check_tensor(ctx, t, name, dtypes=(torch.float32,)):
    """The kernels read raw device pointers: a tensor handed over the ABI must live on the context's GPU, be dense and have
    a dtype the entry point understands.  Anything else raises ValueError here instead of reading out of bounds there."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor on {ctx.torch_device}")
    if t.device != ctx.torch_device:
        raise ValueError(f"{name}: tensor is on {t.device}, the context drives {ctx.torch_device}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name}: dtype {t.dtype} not supported here (expected one of {[str(d) for d in dtypes]})")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def gauss_taps(ksize, sigma):
    """The integer 8.8 taps sr_degrade_gauss takes for GaussianBlur((ksize, ksize), sigma): g_i = exp(-(i - r)^2 / (2 sigma^2)) in fp64,
    t_i = floor(256 g_i / sum g + 0.5), the centre tap then takes 256 - sum t (include/sr355.h)."""
    if ksize not in (3, 5, 7) or not sigma > 0:
        raise ValueError(f"gauss_taps: ksize must be 3, 5 or 7 and sigma positive, got {ksize!r}, {sigma!r}")
    r = ksize // 2
    g = np.exp(-((np.arange(ksize, dtype=np.float64) - r) ** 2) / (2.0 * float(sigma) ** 2))
    t = np.floor(256.0 * g / g.sum() + 0.5).astype(np.int64)
    t[r] += 256 - int(t.sum())
    return t.astype(np.int32)


class Context:
    """sr_ctx wrapper; `Context.get(i)` returns the process-wide context of GPU i."""
    _instances = {}

    @classmethod
    def get(cls, device=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("sr355 needs an MI355X: torch.cuda.is_available() is False and there is no CPU path")
            device = torch.cuda.current_device()
        if isinstance(device, torch.device):
            device = device.index if device.index is not None else torch.cuda.current_device()
        if device not in cls._instances:
            cls._instances[device] = cls(device)
        return cls._instances[device]

    def __init__(self, device):
        self.lib = L.load()
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.sr_init(self.device, C.byref(h))
        if rc != L.SR_OK:
            raise Sr355Error(f"sr_init(device={device}) failed with {rc} (no usable GPU?)")
        self.h = h
        self.torch_device = torch.device("cuda", self.device)

    # ------------------------------------------------------------------ helpers
    def check(self, rc):
        if rc != L.SR_OK:
            msg = self.lib.sr_last_error(self.h).decode("utf-8", "replace")
            raise _EXC.get(rc, Sr355Error)(msg)

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.torch_device).cuda_stream)

    def to_device(self, a, dtype=None):
        """NumPy array or tensor -> contiguous tensor on this GPU (the reference hands NumPy arrays to predict)."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.to(self.torch_device, non_blocking=False).contiguous()

    def empty(self, shape, dtype=torch.float32):
        return torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=self.torch_device)

    def mem_info(self):
        cur, peak = C.c_int64(), C.c_int64()
        self.check(self.lib.sr_mem_info(self.h, C.byref(cur), C.byref(peak)))
        return {"current": cur.value, "peak": peak.value}

    def last_forward_ms(self):
        ms = C.c_float()
        self.check(self.lib.sr_last_forward_ms(self.h, C.byref(ms)))
        return ms.value

    def measure_clock_mhz(self):
        """Shader clock held under a dense bf16 MFMA load (in-kernel s_memtime / s_memrealtime), MHz."""
        mhz = C.c_float()
        self.check(self.lib.sr_measure_clock(self.h, C.byref(mhz), self.stream()))
        return mhz.value

    FUSED_ALL = 511
    FUSED_DENSE_TAIL, FUSED_DENSE_MID, FUSED_RGB_TAIL = L.FUSE_DENSE_TAIL, L.FUSE_DENSE_MID, L.FUSE_RGB_TAIL
    FUSED_ATTN_PROJ, FUSED_CELLS, FUSED_CONV1_STREAM = L.FUSE_ATTN_PROJ, L.FUSE_CELLS, L.FUSE_CONV1_STREAM
    FUSED_POOL, FUSED_CONV_STREAM, FUSED_SRCNN_1X1 = L.FUSE_POOL, L.FUSE_CONV_STREAM, L.FUSE_SRCNN_1X1
    FUSED_TWO_UP = L.FUSE_TWO_UP

    def set_fused(self, mask=511, max_workgroups=0):
        """Which fused / persistent paths sr_forward may take: an OR of the FUSED_* bits (include/sr355.h, SR_FUSE_*): FUSED_DENSE_TAIL / FUSED_DENSE_MID:
        a dense block's conv4+conv5 / conv2+conv3 as one kernel; FUSED_RGB_TAIL: the generator's RGB conv in final_conv1's epilogue; FUSED_ATTN_PROJ:
        SelfAttention's f / g / h projections in the epilogue of the conv before it; FUSED_CELLS: batches of small images (VGG16 block 5) packed into one
        tall image with zero separators; FUSED_CONV1_STREAM: conv1 of a dense block on the streaming line-buffer kernel; FUSED_POOL: a 2x2 max-pool inside
        the epilogue of the conv in front of it; FUSED_CONV_STREAM: 3x3 convs from 64 input channels on the persistent kernel with resident weights;
        FUSED_SRCNN_1X1: SRCNN's 1x1 conv in the 9x9 head's epilogue.  FUSED_ALL (the default): all of them; 0 = layer by layer.
        At 8 growth channels (bf16) the three FUSED_TWO_UP bits together run every dense block as one LDS-resident kernel, dense_block_lds<bf16,g8>, for
        every image dense_block_lds_bytes accepts (24 x 24 patches among them); max_workgroups caps that kernel's persistent grid as well."""
        self.check(self.lib.sr_debug_set_fused(self.h, int(mask), int(max_workgroups)))

    @staticmethod
    def dense_block_lds_bytes(growth_channels, H, W):
        """Dynamic LDS bytes the LDS-resident dense-block kernel needs for an H x W image, or -1 where it does not apply (sr_dense_block_lds_bytes)."""
        return int(L.load().sr_dense_block_lds_bytes(int(growth_channels), int(H), int(W)))

    @staticmethod
    def dense_block_stream_lds_bytes(growth_channels, W):
        """Dynamic LDS bytes of the streamed dense-block kernel's row ring for images W wide (any height), or -1 where it does not apply
        (sr_dense_block_stream_lds_bytes)."""
        return int(L.load().sr_dense_block_stream_lds_bytes(int(growth_channels), int(W)))

    @staticmethod
    def dense_block_stream_bands(B, H, num_cus):
        """The first rows of the bands the streamed dense-block kernel cuts each of B images of H rows into on num_cus CUs (sr_dense_block_stream_bands)."""
        lib = L.load()
        n = int(lib.sr_dense_block_stream_bands(int(B), int(H), int(num_cus), None, 0))
        if n < 1:
            raise ValueError("dense_block_stream_bands: B, H and num_cus must be positive")
        y0 = (C.c_int32 * n)()
        if int(lib.sr_dense_block_stream_bands(int(B), int(H), int(num_cus), y0, n)) != n:
            raise RuntimeError("sr_dense_block_stream_bands disagrees with itself")
        return list(y0)

    def set_block_stream_bands(self, n=0):
        """Test hook: the streamed dense-block kernel cuts every image into n bands (at most its height); 0 = automatic (sr_debug_set_block_stream_bands)."""
        self.check(self.lib.sr_debug_set_block_stream_bands(self.h, int(n)))

    def set_alloc_cap(self, nbytes):
        """Test hook: allocations through this context fail once it would hold more than nbytes (0 = no cap)."""
        self.check(self.lib.sr_debug_set_alloc_cap(self.h, int(nbytes)))

    def conv_routes(self, enable=True):
        """Test hook: the kernel variants (e.g. 'wide<f32,k3,kg2,nt2>/sk') of the conv launches since the previous call, in launch order;
        conv launches after this call are logged iff `enable` (sr_debug_conv_routes)."""
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.sr_debug_conv_routes(self.h, int(bool(enable)), buf, len(buf)))
        return buf.value.decode().split()

    def profile_begin(self):
        self.check(self.lib.sr_profile_begin(self.h))

    def profile_end(self):
        """-> [{'kernel','launches','total_ms','flops','bytes'}] per kernel template instance (HIP-event timed)."""
        import json
        buf = C.create_string_buffer(1 << 16)
        self.check(self.lib.sr_profile_end(self.h, buf, len(buf)))
        return json.loads(buf.value.decode())

    # ------------------------------------------------------------------ single ops
    def conv2d(self, x, w, b=None, act="linear", alpha=1.0, skip1=None, beta1=0.0, skip2=None, beta2=0.0,
               clip01=False, d2s=1):
        """Keras Conv2D(padding='same') + fused epilogue; x NHWC tensor (f32/bf16), w HWIO NumPy."""
        w = _np32(w)
        b = _np32(b)
        kh, kw, cin, cout = w.shape
        _check_tensor(self, x, "conv2d input", (torch.float32, torch.bfloat16))
        for nm, sk in (("skip1", skip1), ("skip2", skip2)):
            if sk is not None:
                _check_tensor(self, sk, f"conv2d {nm}", (x.dtype,))
        B, H, W, Cx = x.shape
        if Cx != cin:
            raise ValueError("conv2d: input channels do not match the kernel")
        r = max(1, int(d2s))
        y = self.empty((B, H * r, W * r, cout // (r * r)), x.dtype)
        actc = {"linear": L.ACT_LINEAR, None: L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}[act]
        self.check(self.lib.sr_conv2d(self.h, x.data_ptr(), dtype_code(x.dtype), B, H, W, cin, _fptr(w), _fptr(b), kh, kw, cout,
                                      actc, float(alpha), None if skip1 is None else skip1.data_ptr(), float(beta1),
                                      None if skip2 is None else skip2.data_ptr(), float(beta2), int(bool(clip01)), r,
                                      y.data_ptr(), self.stream()))
        return y

    def conv2d_dev(self, x, w_dev, b_dev, cout, rot=False, act="linear", d2s=1, alpha=1.0, skip1=None, beta1=0.0):
        """conv2d with DEVICE fp32 weights: w_dev [K,K,Cin,Cout], or with rot=True the forward kernel [K,K,Cout,Cin] of the layer whose
        input gradient is wanted.  Packs on the device, asynchronous (sr_conv2d_dev)."""
        _check_tensor(self, x, "conv2d_dev input")
        _check_tensor(self, w_dev, "conv2d_dev kernel")
        if b_dev is not None:
            _check_tensor(self, b_dev, "conv2d_dev bias")
        if skip1 is not None:
            _check_tensor(self, skip1, "conv2d_dev skip1")
        B, H, W, Cx = x.shape
        k = w_dev.shape[0]
        want = (k, k, cout, Cx) if rot else (k, k, Cx, cout)
        if tuple(w_dev.shape) != want:
            raise ValueError(f"conv2d_dev: kernel shape {tuple(w_dev.shape)} does not match {want}")
        r = max(1, int(d2s))
        y = self.empty((B, H * r, W * r, cout // (r * r)), torch.float32)
        actc = {"linear": L.ACT_LINEAR, None: L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}[act]
        self.check(self.lib.sr_conv2d_dev(self.h, x.data_ptr(), B, H, W, Cx, w_dev.data_ptr(), None if b_dev is None else b_dev.data_ptr(), k,
                                          int(cout), int(bool(rot)), actc, float(alpha), None if skip1 is None else skip1.data_ptr(), float(beta1),
                                          None, 0.0, 0, r, y.data_ptr(), self.stream()))
        return y

    def self_attention(self, x, wf, bf, wg, bg, wh, bh, wv, bv):
        _check_tensor(self, x, "self_attention input", (torch.float32, torch.bfloat16))
        B, H, W, Cx = x.shape
        arrs = [_np32(a) for a in (wf, bf, wg, bg, wh, bh, wv, bv)]
        y = torch.empty_like(x)
        self.check(self.lib.sr_self_attention(self.h, x.data_ptr(), dtype_code(x.dtype), B, H, W, Cx, *[_fptr(a) for a in arrs],
                                              y.data_ptr(), self.stream()))
        return y

    def bicubic(self, x, out_h, out_w):
        _check_tensor(self, x, "bicubic input", (torch.float32, torch.uint8))
        B, H, W, Cx = x.shape
        y = self.empty((B, out_h, out_w, Cx), x.dtype)
        self.check(self.lib.sr_bicubic(self.h, x.data_ptr(), dtype_code(x.dtype), B, H, W, Cx, int(out_h), int(out_w), y.data_ptr(),
                                       self.stream()))
        return y

    INTERPOLATIONS = {"INTER_NEAREST": 0, "INTER_LINEAR": 1, "INTER_CUBIC": 2, "INTER_AREA": 3, "INTER_LANCZOS4": 4, "INTER_LINEAR_EXACT": 5}

    def resize(self, x, out_h, out_w, interpolation="INTER_CUBIC"):
        """cv2.resize(x, (out_w, out_h), interpolation): x [B,H,W,C] f32 or u8 tensor; interpolation = OpenCV name or code
        (INTER_NEAREST 0, INTER_LINEAR 1, INTER_CUBIC 2, INTER_AREA 3, INTER_LANCZOS4 4; INTER_LINEAR_EXACT 5 on float images, where
        OpenCV itself falls back to INTER_LINEAR).  Codes cv2.resize rejects, and the two it accepts that are not restated here
        (INTER_NEAREST_EXACT 6; INTER_LINEAR_EXACT on uint8), raise ValueError -- cv2.error where the reference runs."""
        code = self.INTERPOLATIONS.get(interpolation, interpolation)
        _check_tensor(self, x, "resize input", (torch.float32, torch.uint8))
        if code == 5 and x.dtype == torch.float32:
            code = 1
        if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or int(code) not in (0, 1, 2, 3, 4):
            raise ValueError(f"unsupported interpolation {interpolation!r}")
        B, H, W, Cx = x.shape
        y = self.empty((B, out_h, out_w, Cx), x.dtype)
        self.check(self.lib.sr_resize(self.h, x.data_ptr(), dtype_code(x.dtype), B, H, W, Cx, int(out_h), int(out_w), int(code), y.data_ptr(),
                                      self.stream()))
        return y

    def _metric(self, fn, a, b, max_val):
        _check_tensor(self, a, "metric input a")
        _check_tensor(self, b, "metric input b")
        if a.shape != b.shape or a.dim() != 4:
            raise ValueError("metric inputs must be two [B,H,W,C] tensors of the same shape")
        B, H, W, Cx = a.shape
        out = self.empty((B,), torch.float32)
        if B:
            self.check(fn(self.h, a.data_ptr(), b.data_ptr(), B, H, W, Cx, float(max_val), out.data_ptr(), self.stream()))
        return out

    def psnr(self, a, b, max_val=1.0):
        return self._metric(self.lib.sr_psnr, a, b, max_val)

    def ssim(self, a, b, max_val=1.0):
        return self._metric(self.lib.sr_ssim, a, b, max_val)

    def mse(self, a, b):
        _check_tensor(self, a, "mse input a")
        _check_tensor(self, b, "mse input b")
        if a.shape != b.shape:
            raise ValueError("mse inputs must have the same shape")
        out = self.empty((1,), torch.float32)
        self.check(self.lib.sr_mse(self.h, a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), self.stream()))
        return out

    # ------------------------------------------------------------------ the classical study's other four up-scalers (classic_algorithms.py:23-108)
    def _gray_batch(self, x, name):
        _check_tensor(self, x, name, (torch.uint8,))
        if x.dim() != 3:
            raise ValueError(f"{name}: expected a [B,h,w] uint8 batch of grayscale images, got shape {tuple(x.shape)}")
        return x.shape

    def back_projection(self, hr, lr, iterations=10, raw=False):
        """Iterative back-projection (sr_back_projection): hr [B,H,W] uint8 starting estimate, lr [B,h,w] uint8 -> uint8 [B,H,W]; with
        raw=True also the float32 estimate before the clip and truncation."""
        B, H, W = self._gray_batch(hr, "back_projection hr")
        Bl, h, w = self._gray_batch(lr, "back_projection lr")
        if Bl != B:
            raise ValueError("back_projection: hr and lr batches differ in size")
        y = self.empty((B, H, W), torch.uint8)
        est = self.empty((B, H, W), torch.float32) if raw else None
        self.check(self.lib.sr_back_projection(self.h, hr.data_ptr(), lr.data_ptr(), B, H, W, h, w, int(iterations), y.data_ptr(),
                                               None if est is None else est.data_ptr(), self.stream()))
        return (y, est) if raw else y

    def noise_sigma(self, x):
        """skimage estimate_sigma of each [h,w] uint8 image of x [B,h,w] (sr_noise_sigma) -> float64 [B] on the device (NaN: no detail)."""
        B, h, w = self._gray_batch(x, "noise_sigma input")
        sigma = self.empty((B,), torch.float64)
        self.check(self.lib.sr_noise_sigma(self.h, x.data_ptr(), B, h, w, sigma.data_ptr(), self.stream()))
        return sigma

    @staticmethod
    def nlm_sigma_error(indices):
        """The ValueError non_local_means raises for the images whose noise estimate is zero or not finite."""
        return ValueError(f"non_local_means: the noise estimate of image(s) {[int(i) for i in indices]} is zero or not finite "
                          "(an image without detail); the reference would divide by zero")

    def non_local_means(self, lr, H, W, patch_size=5, patch_distance=6, h_scale=1.15, raw=False, check=True):
        """non_local_means (classic_algorithms.py:45-62) on lr [B,h,w] uint8: sigma, fast NL-means with h = h_scale * sigma, then
        INTER_LANCZOS4 to (H, W) -> float32 [B,H,W]; raw=True -> (that, the denoised [B,h,w], sigma [B]).  A sigma that is zero or not
        finite (an image without detail: the reference divides by zero there) raises ValueError -- checking it waits for the device.
        check=False does not wait: the result is followed by the device flag tensor, bool [B], true for such an image (its output is
        then not a number), and the caller raises nlm_sigma_error once it has read the flags."""
        B, h, w = self._gray_batch(lr, "non_local_means input")
        sigma = self.noise_sigma(lr)
        bad = ~torch.isfinite(sigma) | (sigma <= 0)
        if check and bool(bad.any()):
            raise self.nlm_sigma_error(torch.nonzero(bad).flatten().tolist())
        den = self.empty((B, h, w), torch.float32)
        self.check(self.lib.sr_nl_means(self.h, lr.data_ptr(), B, h, w, int(patch_size), int(patch_distance), sigma.data_ptr(), float(h_scale),
                                        den.data_ptr(), self.stream()))
        up = self.resize(den.unsqueeze(-1), int(H), int(W), "INTER_LANCZOS4").squeeze(-1)
        out = (up, den, sigma) if raw else (up,)
        if not check:
            return out + (bad,)
        return out if raw else up

    def edge_guided(self, x, H, W, weight=0.3, raw=False):
        """edge_guided_interpolation (sr_edge_guided) on x [B,h,w] uint8 -> uint8 [B,H,W]; raw=True -> (that, the float32 up-sized edges)."""
        B, h, w = self._gray_batch(x, "edge_guided input")
        y = self.empty((B, H, W), torch.uint8)
        up_e = self.empty((B, H, W), torch.float32) if raw else None
        self.check(self.lib.sr_edge_guided(self.h, x.data_ptr(), B, h, w, int(H), int(W), float(weight), y.data_ptr(),
                                           None if up_e is None else up_e.data_ptr(), self.stream()))
        return (y, up_e) if raw else y

    def freq_extrapolate(self, x, H, W):
        """frequency_extrapolation (sr_freq_extrapolate) on x [B,h,w] uint8 -> float64 [B,H,W]."""
        B, h, w = self._gray_batch(x, "freq_extrapolate input")
        y = self.empty((B, H, W), torch.float64)
        self.check(self.lib.sr_freq_extrapolate(self.h, x.data_ptr(), B, h, w, int(H), int(W), y.data_ptr(), self.stream()))
        return y

    # ------------------------------------------------------------------ channel-range views (the training tape's dense blocks: sr_*_views)
    # ------------------------------------------------------------------ the classical study's image-quality scores (profiling_methods.py:45-167)
    SCORE_NAMES = L.SCORE_NAMES

    def _score_data_range(self, hr, data_range):
        B = hr.shape[0]
        if isinstance(data_range, str):
            if data_range != "hr_span":
                raise ValueError(f"classic_scores: data_range must be a number, a per-pair array or 'hr_span', not {data_range!r}")
            flat = hr.reshape(B, -1)
            span = (flat.amax(1) - flat.amin(1)).to(torch.float64)       # in hr's own dtype first, as the notebook's numpy scalars
            return torch.where(span == 0, torch.full_like(span, 255.0), span).contiguous()
        if isinstance(data_range, torch.Tensor):
            dr = data_range.to(self.torch_device, torch.float64).reshape(-1)
        else:
            dr = torch.as_tensor(np.asarray(data_range, dtype=np.float64).reshape(-1), device=self.torch_device)
        if dr.numel() == 1:
            dr = dr.expand(B)
        if dr.numel() != B:
            raise ValueError(f"classic_scores: data_range has {dr.numel()} entries for {B} pairs")
        return dr.contiguous()

    def classic_scores(self, hr, sr, data_range=255.0, hf_radius_frac=0.6, raw=False):
        """The nine scores of each pair (sr_classic_scores; columns SCORE_NAMES) -> float64 [B, 9] on the device.
        hr, sr: [B,H,W] (gray) or [B,H,W,3] (RGB) device tensors, each uint8 or float32, H and W >= 7.  data_range: a number, a [B]
        array / tensor, or 'hr_span' (max(hr) - min(hr) per pair, 255 where that is 0: the notebook's NL-means rule).
        raw=True -> (scores, dict of the intermediates: 'gray' and 'sobel' float32 [B,2,H,W] (hr, sr), 'hist_luma' int32 [B,2,256],
        'hist_color' int32 [B,2,3,64] for RGB).  For float RGB pairs the gray-derived columns are NaN and the gray intermediates unset."""
        _check_tensor(self, hr, "classic_scores hr", (torch.uint8, torch.float32))
        _check_tensor(self, sr, "classic_scores sr", (torch.uint8, torch.float32))
        if hr.shape != sr.shape or hr.dim() not in (3, 4) or (hr.dim() == 4 and hr.shape[3] not in (1, 3)):
            raise ValueError(f"classic_scores: expected two [B,H,W] or [B,H,W,3] batches of one shape, got {tuple(hr.shape)} and {tuple(sr.shape)}")
        B, H, W = hr.shape[:3]
        Cx = hr.shape[3] if hr.dim() == 4 else 1
        if H < 7 or W < 7:
            raise ValueError(f"classic_scores: images of {H} x {W} are smaller than the 7 x 7 SSIM window")
        dr = self._score_data_range(hr, data_range)
        out = self.empty((B, len(self.SCORE_NAMES)), torch.float64)
        inter = None
        if raw:
            inter = {"gray": self.empty((B, 2, H, W)), "sobel": self.empty((B, 2, H, W)),
                     "hist_luma": self.empty((B, 2, 256), torch.int32)}
            if Cx == 3:
                inter["hist_color"] = self.empty((B, 2, 3, 64), torch.int32)
        ptr = (lambda k: None if inter is None or k not in inter else inter[k].data_ptr())
        self.check(self.lib.sr_classic_scores(self.h, hr.data_ptr(), dtype_code(hr.dtype), sr.data_ptr(), dtype_code(sr.dtype), B, H, W, Cx,
                                              dr.data_ptr(), float(hf_radius_frac), out.data_ptr(), ptr("gray"), ptr("sobel"),
                                              ptr("hist_luma"), ptr("hist_color"), self.stream()))
        return (out, inter) if raw else out

    # ------------------------------------------------------------------ the classical study's loop glue and SSIM maps (notebook cell 8; visualization_methods.py:553-591)
    def rgb2gray(self, x):
        """cv2.cvtColor(x, COLOR_RGB2GRAY) on a uint8 [B,H,W,3] device batch -> uint8 [B,H,W] on the device (sr_rgb2gray_u8)."""
        _check_tensor(self, x, "rgb2gray input", (torch.uint8,))
        if x.dim() != 4 or x.shape[3] != 3 or x.numel() == 0:
            raise ValueError(f"rgb2gray: expected a non-empty [B,H,W,3] uint8 batch, got shape {tuple(x.shape)}")
        B, H, W, _ = x.shape
        y = self.empty((B, H, W), torch.uint8)
        self.check(self.lib.sr_rgb2gray_u8(self.h, x.data_ptr(), B, H, W, y.data_ptr(), self.stream()))
        return y

    def freq_to_u8(self, f):
        """The notebook's normalisation of frequency_extrapolation's output, (f / max(f) * 255.0) truncated to uint8 where max(f) > 0 and
        f truncated otherwise, per image: f float64 [B,H,W] on the device -> (uint8 [B,H,W], the maxima float64 [B]) (sr_freq_to_u8)."""
        _check_tensor(self, f, "freq_to_u8 input", (torch.float64,))
        if f.dim() != 3 or f.numel() == 0:
            raise ValueError(f"freq_to_u8: expected a non-empty [B,H,W] float64 batch, got shape {tuple(f.shape)}")
        B, H, W = f.shape
        y = self.empty((B, H, W), torch.uint8)
        mx = self.empty((B,), torch.float64)
        self.check(self.lib.sr_freq_to_u8(self.h, f.data_ptr(), B, H, W, y.data_ptr(), mx.data_ptr(), self.stream()))
        return y, mx

    def ssim_map(self, a, b, data_range=255.0):
        """skimage's structural_similarity(a, b, data_range=..., full=True) for each pair (sr_ssim_map): a, b [B,H,W] or [B,H,W,C] (C 1 or 3)
        device tensors, each uint8 or float32; data_range as classic_scores takes it -> (S float64 of a's shape, over the whole image with
        scipy's 'reflect' border, and mssim float64 [B]), both on the device."""
        _check_tensor(self, a, "ssim_map a", (torch.uint8, torch.float32))
        _check_tensor(self, b, "ssim_map b", (torch.uint8, torch.float32))
        if a.shape != b.shape or a.dim() not in (3, 4) or (a.dim() == 4 and a.shape[3] not in (1, 3)) or a.shape[0] < 1:
            raise ValueError(f"ssim_map: expected two [B,H,W] or [B,H,W,C] (C 1 or 3) batches of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        B, H, W = a.shape[:3]
        Cx = a.shape[3] if a.dim() == 4 else 1
        if H < 7 or W < 7:
            raise ValueError(f"ssim_map: images of {H} x {W} are smaller than the 7 x 7 SSIM window")
        dr = self._score_data_range(a, data_range)
        smap = self.empty(tuple(a.shape), torch.float64)
        mean = self.empty((B,), torch.float64)
        self.check(self.lib.sr_ssim_map(self.h, a.data_ptr(), dtype_code(a.dtype), b.data_ptr(), dtype_code(b.dtype), B, H, W, Cx, dr.data_ptr(),
                                        smap.data_ptr(), mean.data_ptr(), self.stream()))
        return smap, mean

    EDA_STAT_NAMES = L.EDA_STAT_NAMES

    def _eda_pair(self, lr, hr, who):
        _check_tensor(self, lr, f"{who} lr", (torch.uint8,))
        _check_tensor(self, hr, f"{who} hr", (torch.uint8,))
        if lr.shape != hr.shape or lr.dim() != 4 or lr.shape[3] != 3:
            raise ValueError(f"{who}: expected two uint8 BGR batches [B,H,W,3] of one shape, got {tuple(lr.shape)} and {tuple(hr.shape)}")
        return lr.shape[:3]

    def eda_pair_stats(self, lr, hr, glcm_levels=64, angles=(0,), raw=False):
        """The EDA's per-pair statistics (sr_eda_pair_stats; columns EDA_STAT_NAMES) -> float64 [B, 46] on the device.  lr, hr: uint8 BGR
        device tensors [B,H,W,3] of one shape (lr aligned to hr).  glcm_levels 64 or 256; angles: indices into (0, 45, 90, 135 degrees).
        raw=True -> (stats, dict of the intermediates: 'gray', 'sat', 'val', 'blur3', 'edges' uint8 [B,2,H,W] (lr, hr), 'blur5' uint8
        [B,2,H,W,3], 'glcm' int32 [B,nangles,L,L] lr's counts before symmetrisation, 'dct' float64 [B,2,H,W])."""
        B, H, W = self._eda_pair(lr, hr, "eda_pair_stats")
        angles = sorted(set(int(a) for a in angles))
        if not angles or angles[0] < 0 or angles[-1] > 3:
            raise ValueError(f"eda_pair_stats: angles are indices 0..3 into (0, 45, 90, 135 degrees), got {angles}")
        if glcm_levels not in (64, 256):
            raise ValueError(f"eda_pair_stats: glcm_levels must be 64 or 256, got {glcm_levels}")
        out = self.empty((B, len(self.EDA_STAT_NAMES)), torch.float64)
        inter = {}
        if raw:
            inter = {k: self.empty((B, 2, H, W), torch.uint8) for k in ("gray", "sat", "val", "blur3", "edges")}
            inter["blur5"] = self.empty((B, 2, H, W, 3), torch.uint8)
            inter["glcm"] = self.empty((B, len(angles), glcm_levels, glcm_levels), torch.int32)
            inter["dct"] = self.empty((B, 2, H, W), torch.float64)
        ptr = (lambda k: inter[k].data_ptr() if k in inter else None)
        self.check(self.lib.sr_eda_pair_stats(self.h, lr.data_ptr(), hr.data_ptr(), B, H, W, int(glcm_levels), sum(1 << a for a in angles), out.data_ptr(),
                                              ptr("gray"), ptr("sat"), ptr("val"), ptr("blur3"), ptr("blur5"), ptr("edges"), ptr("glcm"), ptr("dct"),
                                              self.stream()))
        return (out, inter) if raw else out

    def eda_accumulate(self, lr, hr, acc=None):
        """Adds the pairs' global EDA data (sr_eda_accumulate) into `acc`, a dict of device buffers made on the first call and returned:
        'lr_fft_sum', 'hr_fft_sum', 'grad_hr_sum' float64 [H,W], 'glcm_sum' float64 [256,256], 'sat_counts' int64 [2,50] (lr, hr)."""
        B, H, W = self._eda_pair(lr, hr, "eda_accumulate")
        if acc is None:
            acc = {k: torch.zeros((H, W), dtype=torch.float64, device=self.torch_device) for k in ("lr_fft_sum", "hr_fft_sum", "grad_hr_sum")}
            acc["glcm_sum"] = torch.zeros((256, 256), dtype=torch.float64, device=self.torch_device)
            acc["sat_counts"] = torch.zeros((2, 50), dtype=torch.int64, device=self.torch_device)
        if tuple(acc["lr_fft_sum"].shape) != (H, W):
            raise ValueError(f"eda_accumulate: the accumulators hold {tuple(acc['lr_fft_sum'].shape)} images, the batch is {H} x {W}")
        self.check(self.lib.sr_eda_accumulate(self.h, lr.data_ptr(), hr.data_ptr(), B, H, W, acc["lr_fft_sum"].data_ptr(), acc["hr_fft_sum"].data_ptr(),
                                              acc["grad_hr_sum"].data_ptr(), acc["glcm_sum"].data_ptr(), acc["sat_counts"].data_ptr(), self.stream()))
        return acc

    EDA_PANEL_OUTPUTS = ("spec_lr", "spec_hr", "grad_hr", "glcm_lr", "noise_lr", "diff", "sat_hist", "glcm_contrast", "noise_mean")

    def eda_pair_panels(self, lr, hr, which=None):
        """The maps of the EDA's per-pair panels (sr_eda_pair_panels), unsummed -> dict of device tensors: 'spec_lr', 'spec_hr' float64
        [B,H,W] (|fftshift(fft2(gray))|, the magnitude: the panel's log is the caller's), 'grad_hr', 'noise_lr' float64 [B,H,W], 'glcm_lr'
        float64 [B,256,256], 'diff' uint8 [B,H,W], 'sat_hist' int64 [B,2,256] (lr, hr), 'glcm_contrast', 'noise_mean' float64 [B].
        which: the names wanted (None: all); the others are neither computed nor returned."""
        B, H, W = self._eda_pair(lr, hr, "eda_pair_panels")
        names = self.EDA_PANEL_OUTPUTS if which is None else tuple(which)
        unknown = [k for k in names if k not in self.EDA_PANEL_OUTPUTS]
        if unknown or not names:
            raise ValueError(f"eda_pair_panels: which names outputs among {self.EDA_PANEL_OUTPUTS}, got {list(names)}")
        shapes = {"spec_lr": ((B, H, W), torch.float64), "spec_hr": ((B, H, W), torch.float64), "grad_hr": ((B, H, W), torch.float64),
                  "glcm_lr": ((B, 256, 256), torch.float64), "noise_lr": ((B, H, W), torch.float64), "diff": ((B, H, W), torch.uint8),
                  "sat_hist": ((B, 2, 256), torch.int64)}
        out = {k: self.empty(*shapes[k]) for k in shapes if k in names}
        scalars = self.empty((B, 2), torch.float64) if ("glcm_contrast" in names or "noise_mean" in names) else None
        ptr = (lambda k: out[k].data_ptr() if k in out else None)
        self.check(self.lib.sr_eda_pair_panels(self.h, lr.data_ptr(), hr.data_ptr(), B, H, W, ptr("spec_lr"), ptr("spec_hr"), ptr("grad_hr"), ptr("glcm_lr"),
                                               ptr("noise_lr"), ptr("diff"), ptr("sat_hist"), None if scalars is None else scalars.data_ptr(),
                                               self.stream()))
        for j, k in enumerate(("glcm_contrast", "noise_mean")):           # SR_EDA_PANEL_* order
            if k in names:
                out[k] = scalars[:, j].contiguous()
        return out

    # ------------------------------------------------------------------ LPIPS (data/EDA.ipynb lpips_score; csrc/lpips.hip)
    def lpips_set_weights(self, weights):
        """Sets (a dict from sr355.lpips.load_weights / seeded_weights) or, with None, unloads the weights of lpips / sr_lpips on this context.
        The library copies and packs them once."""
        if weights is None:
            self.check(self.lib.sr_lpips_set_weights(self.h, None, None, None))
            return
        from .lpips import check_weights
        w = check_weights(weights)
        arr = lambda k: (C.POINTER(C.c_float) * 5)(*[_fptr(a) for a in w[k]])
        self.check(self.lib.sr_lpips_set_weights(self.h, arr("conv_w"), arr("conv_b"), arr("lin_w")))

    def lpips(self, a, b, raw=False):
        """LPIPS (AlexNet, version 0.1) of the pairs (a[i], b[i]) -> float32 [B] on the device.  a, b: device tensors [B,H,W,3] of one shape, both
        uint8 BGR (the EDA's images) or both float32 RGB in [-1, 1]; 31 <= H, W.  raw=True -> (score, terms float32 [B,5], taps: five float32
        tensors [2,B,h,w,C], the raw ReLU features of a then b).  RuntimeError while no weights are set (lpips_set_weights)."""
        _check_tensor(self, a, "lpips a", (torch.uint8, torch.float32))
        _check_tensor(self, b, "lpips b", (a.dtype,))
        if a.shape != b.shape or a.dim() != 4 or a.shape[3] != 3 or a.shape[0] < 1:
            raise ValueError(f"lpips: expected two batches [B,H,W,3] of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        B, H, W = (int(v) for v in a.shape[:3])
        from .lpips import TAP_CHANNELS, tap_shapes
        hw = tap_shapes(H, W)
        score = self.empty((B,))
        terms = self.empty((B, 5)) if raw else None
        taps = [self.empty((2, B, h, w, c)) for (h, w), c in zip(hw, TAP_CHANNELS)] if raw else None
        tp = (C.c_void_p * 5)(*[t.data_ptr() for t in taps]) if raw else None
        self.check(self.lib.sr_lpips(self.h, a.data_ptr(), b.data_ptr(), _TORCH2DT[a.dtype], B, H, W, score.data_ptr(), terms.data_ptr() if raw else None, tp,
                                     self.stream()))
        return (score, terms, taps) if raw else score

    # ------------------------------------------------------------------ dataset synthesis: degrade_image's per-pixel stages (common_methods.py:52-107)
    @staticmethod
    def degrade_params(records):
        """Host int32 table [B, 16] (SR_DEG_* columns) from one dict per image: gauss_ksize (0 / None: off) with gauss_sigma or gauss_taps,
        motion_size (0: off), noise_std (None: off), jpeg_quality (0: off), interp_code.  Missing keys mean off."""
        t = np.zeros((len(records), L.DEG_PARAMS), np.int32)
        for i, r in enumerate(records):
            k = int(r.get("gauss_ksize") or 0)
            if k:
                taps = r["gauss_taps"] if r.get("gauss_taps") is not None else gauss_taps(k, r["gauss_sigma"])
                t[i, L.DEG_GAUSS_KSIZE] = k
                t[i, L.DEG_GAUSS_TAP0:L.DEG_GAUSS_TAP0 + len(taps)] = taps
            t[i, L.DEG_MOTION_SIZE] = int(r.get("motion_size") or 0)
            if r.get("noise_std") is not None:
                t[i, L.DEG_NOISE_ON] = 1
                t[i, L.DEG_NOISE_STD] = np.array([r["noise_std"]], np.float32).view(np.int32)[0]
            t[i, L.DEG_JPEG_QUALITY] = int(r.get("jpeg_quality") or 0)
            t[i, L.DEG_INTERP] = int(r.get("interp_code") or 0)
        return t

    def _degrade_args(self, x, params, who):
        if isinstance(x, torch.Tensor) and x.dtype != torch.uint8:
            raise NotImplementedError(f"{who}: {x.dtype} images are not offered (the dataset's frames are 8-bit BGR)")
        _check_tensor(self, x, f"{who} input", (torch.uint8,))
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"{who}: expected a uint8 BGR batch [B,H,W,3], got shape {tuple(x.shape)}")
        if not isinstance(params, torch.Tensor):
            params = self.to_device(np.ascontiguousarray(params, dtype=np.int32))
        _check_tensor(self, params, f"{who} params", (torch.int32,))
        if tuple(params.shape) != (x.shape[0], L.DEG_PARAMS):
            raise ValueError(f"{who}: the parameter table must be int32 [{x.shape[0]}, {L.DEG_PARAMS}], got {tuple(params.shape)}")
        return params, x.shape[0], x.shape[1], x.shape[2]

    def degrade_status(self):
        """Waits for the stream and raises ValueError when a degrade stage met a parameter row outside its contract (sr_degrade_status)."""
        self.check(self.lib.sr_degrade_status(self.h, self.stream()))

    def degrade_gauss(self, x, params, check=True):
        """cv2.GaussianBlur per image of x [B,H,W,3] uint8 with the kernel size and 8.8 taps of its row of `params` (sr_degrade_gauss).
        check=False leaves the table's validation to a later degrade_status() (no wait for the device here)."""
        params, B, H, W = self._degrade_args(x, params, "degrade_gauss")
        y = torch.empty_like(x)
        self.check(self.lib.sr_degrade_gauss(self.h, x.data_ptr(), B, H, W, params.data_ptr(), y.data_ptr(), self.stream()))
        if check:
            self.degrade_status()
        return y

    def degrade_motion(self, x, params, check=True):
        """The reference's horizontal motion blur (filter2D with a centre row of 1 / size) per image (sr_degrade_motion)."""
        params, B, H, W = self._degrade_args(x, params, "degrade_motion")
        y = torch.empty_like(x)
        self.check(self.lib.sr_degrade_motion(self.h, x.data_ptr(), B, H, W, params.data_ptr(), y.data_ptr(), self.stream()))
        if check:
            self.degrade_status()
        return y

    def degrade_noise(self, x, params, field=None, seed=0, raw=False, check=True):
        """clip(float32(x) + n, 0, 255) truncated (sr_degrade_noise).  field: float32 [B,H,W,3] device tensor of n (the reference's host
        draw); None: n = std * z from the kernel's Philox4x32-10 stream keyed by the 64-bit `seed`, and raw=True -> (y, z float32)."""
        params, B, H, W = self._degrade_args(x, params, "degrade_noise")
        if field is not None:
            _check_tensor(self, field, "degrade_noise field")
            if field.shape != x.shape:
                raise ValueError(f"degrade_noise: the field's shape {tuple(field.shape)} is not the batch's {tuple(x.shape)}")
            if raw:
                raise ValueError("degrade_noise: raw=True returns the kernel's own z; there is none with a supplied field")
        y = torch.empty_like(x)
        z = self.empty(x.shape, torch.float32) if raw else None
        self.check(self.lib.sr_degrade_noise(self.h, x.data_ptr(), B, H, W, params.data_ptr(), None if field is None else field.data_ptr(),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, y.data_ptr(), None if z is None else z.data_ptr(), self.stream()))
        if check:
            self.degrade_status()
        return (y, z) if raw else y

    def degrade_jpeg(self, x, params, raw=False, check=True):
        """The baseline-JPEG round trip of cv2.imencode / imdecode at each row's quality (sr_degrade_jpeg).  raw=True -> (y, dict: 'coef_y'
        int16 [B,16 my,16 mx], 'coef_cb', 'coef_cr' int16 [B,8 my,8 mx] quantised coefficients, 'y', 'cb', 'cr' uint8 decoded planes of those
        shapes; mx, my = ceil(W / 16), ceil(H / 16)); zeros for images whose quality is 0."""
        params, B, H, W = self._degrade_args(x, params, "degrade_jpeg")
        y = torch.empty_like(x)
        inter = {}
        if raw:
            mx, my = (W + 15) // 16, (H + 15) // 16
            for k, f in (("y", 16), ("cb", 8), ("cr", 8)):
                inter["coef_" + k] = torch.zeros((B, f * my, f * mx), dtype=torch.int16, device=self.torch_device)
                inter[k] = torch.zeros((B, f * my, f * mx), dtype=torch.uint8, device=self.torch_device)
        ptr = (lambda k: inter[k].data_ptr() if k in inter else None)
        self.check(self.lib.sr_degrade_jpeg(self.h, x.data_ptr(), B, H, W, params.data_ptr(), y.data_ptr(), ptr("coef_y"), ptr("coef_cb"), ptr("coef_cr"),
                                            ptr("y"), ptr("cb"), ptr("cr"), self.stream()))
        if check:
            self.degrade_status()
        return (y, inter) if raw else y

    # ------------------------------------------------------------------ dataset synthesis: smart_square_crop for a stack of frames (common_methods.py:4-49)
    def _crop_frames(self, x, who):
        if isinstance(x, torch.Tensor) and x.dtype != torch.uint8:
            raise NotImplementedError(f"{who}: {x.dtype} images are not offered (the dataset's frames are 8-bit BGR)")
        _check_tensor(self, x, f"{who} input", (torch.uint8,))
        if x.dim() != 4 or x.shape[3] != 3 or x.shape[0] < 1:
            raise ValueError(f"{who}: expected a non-empty uint8 BGR batch [B,H,W,3], got shape {tuple(x.shape)}")
        return x.shape[0], x.shape[1], x.shape[2]

    def object_boxes(self, x, raw=False):
        """Per frame of x [B,H,W,3] uint8 BGR (device tensor): the Otsu mask's largest external contour and the square crop centred on it
        (sr_object_boxes) -> int32 [B, 8] on the device, columns BOX_NAMES: found, x, y, w, h (the contour's bounding rectangle), left,
        top (the crop's origin), otsu_t.  raw=True -> (boxes, dict: 'gray' uint8 [B,H,W], 'mask' uint8 [B,H,W] (0 / 255), 'labels' int32
        [B,H,W]: the smallest raster index of the pixel's component of the hole-filled mask, -1 outside it)."""
        B, H, W = self._crop_frames(x, "object_boxes")
        boxes = self.empty((B, len(L.BOX_NAMES)), torch.int32)
        inter = {}
        if raw:
            inter = {"gray": self.empty((B, H, W), torch.uint8), "mask": self.empty((B, H, W), torch.uint8), "labels": self.empty((B, H, W), torch.int32)}
        ptr = (lambda k: inter[k].data_ptr() if k in inter else None)
        self.check(self.lib.sr_object_boxes(self.h, x.data_ptr(), B, H, W, boxes.data_ptr(), ptr("gray"), ptr("mask"), ptr("labels"), self.stream()))
        return (boxes, inter) if raw else boxes

    def square_crop(self, x, boxes=None, check=True):
        """x[b, top : top + S, left : left + S], S = min(H, W), with left and top from frame b's row of `boxes` (sr_square_crop) -> uint8
        [B,S,S,3] on the device.  boxes None: object_boxes(x), nothing returning to the host in between.  A table of the caller's (int32
        [B, 8], device tensor or array) is validated here when check=True, which waits for the device; check=False leaves a left or top
        outside the frame to the kernel, which clamps it into the frame."""
        B, H, W = self._crop_frames(x, "square_crop")
        S = min(H, W)
        if boxes is None:
            boxes = self.object_boxes(x)
        else:
            if not isinstance(boxes, torch.Tensor):
                boxes = self.to_device(np.ascontiguousarray(boxes, dtype=np.int32))
            _check_tensor(self, boxes, "square_crop boxes", (torch.int32,))
            if tuple(boxes.shape) != (B, len(L.BOX_NAMES)):
                raise ValueError(f"square_crop: the box table must be int32 [{B}, {len(L.BOX_NAMES)}], got {tuple(boxes.shape)}")
            if check:
                lt = boxes[:, 5:7].cpu().numpy()
                bad = np.nonzero((lt[:, 0] < 0) | (lt[:, 0] > W - S) | (lt[:, 1] < 0) | (lt[:, 1] > H - S))[0]
                if bad.size:
                    raise ValueError(f"square_crop: row {int(bad[0])} of the box table puts the {S} x {S} square at left {int(lt[bad[0], 0])}, top "
                                     f"{int(lt[bad[0], 1])}, outside the {H} x {W} frame")
        y = self.empty((B, S, S, 3), torch.uint8)
        self.check(self.lib.sr_square_crop(self.h, x.data_ptr(), B, H, W, boxes.data_ptr(), y.data_ptr(), self.stream()))
        return y

    @staticmethod
    def _view(t, coff, c):
        """(tensor [B,H,W,Cbuf] fp32 contiguous, first channel, channels) -> sr_view."""
        if not (isinstance(t, torch.Tensor) and t.dim() == 4 and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda):
            raise ValueError("a view needs a contiguous fp32 NHWC device tensor")
        if coff < 0 or c <= 0 or coff + c > t.shape[3]:
            raise ValueError(f"channel range [{coff}, {coff + c}) outside the buffer's {t.shape[3]} channels")
        return L.View(t.data_ptr(), int(t.shape[3]), int(coff))

    def conv2d_dev_view(self, xbuf, x_coff, cin, w_dev, b_dev, cout, ybuf, y_coff, rot=False, act="linear", alpha=1.0, skip_buf=None, skip_coff=0, beta1=0.0):
        """sr_conv2d_dev on channel ranges: reads xbuf[..., x_coff : x_coff + cin], writes ybuf[..., y_coff : y_coff + cout] (other channels untouched);
        skip_buf / skip_coff: out = alpha * act(conv) + beta1 * skip -- skip may be the output range itself (in-place accumulation)."""
        B, H, W, _ = xbuf.shape
        if tuple(ybuf.shape[:3]) != (B, H, W):
            raise ValueError("conv2d_dev_view: input and output buffers must share [B,H,W]")
        k = w_dev.shape[0]
        want = (k, k, cout, cin) if rot else (k, k, cin, cout)
        if tuple(w_dev.shape) != want:
            raise ValueError(f"conv2d_dev_view: kernel shape {tuple(w_dev.shape)} does not match {want}")
        xv, yv = self._view(xbuf, x_coff, cin), self._view(ybuf, y_coff, cout)
        sv = None if skip_buf is None else self._view(skip_buf, skip_coff, cout)
        actc = {"linear": L.ACT_LINEAR, None: L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}[act]
        self.check(self.lib.sr_conv2d_dev_views(self.h, C.byref(xv), B, H, W, int(cin), w_dev.data_ptr(), None if b_dev is None else b_dev.data_ptr(), k, int(cout),
                                                int(bool(rot)), actc, float(alpha), None if sv is None else C.byref(sv), float(beta1), C.byref(yv), self.stream()))

    def pack_list(self, uses):
        """uses: [(w_dev [K,K,I,O] fp32 device tensor, b_dev or None, rot)] -> an object for conv_prepack.  rot=False is the layer's forward use (the call's Cin = I,
        Cout = O, with its bias), rot=True its input-gradient use (Cin = O, Cout = I, no bias) -- exactly the arguments conv2d_dev / conv2d_dev_view pass for them."""
        arr = (L.PackDesc * max(len(uses), 1))()
        keep = []
        for d, (w, b, rot) in zip(arr, uses):
            _check_tensor(self, w, "pack_list kernel")
            if b is not None:
                _check_tensor(self, b, "pack_list bias")
            k, _, ci, co = w.shape
            d.w, d.bias, d.K = w.data_ptr(), (None if b is None else b.data_ptr()), k
            d.Cin, d.Cout, d.rot = (co, ci, 1) if rot else (ci, co, 0)
            keep.append((w, b))
        return (arr, len(uses), keep)

    def conv_prepack(self, packed_list):
        """sr_conv_prepack: pack every listed use by one launch from the weights' CURRENT contents; later conv2d_dev / conv2d_dev_view calls with the same tensors skip
        their own pack.  Call again after every change of a listed weight; conv_prepack(None) forgets the list."""
        if packed_list is None:
            self.check(self.lib.sr_conv_prepack(self.h, None, 0, self.stream()))
            return
        arr, n, _ = packed_list
        self.check(self.lib.sr_conv_prepack(self.h, arr, n, self.stream()))

    def conv2d_wgrad_view(self, xbuf, x_coff, cin, dybuf, dy_coff, cout, k):
        """sr_conv2d_wgrad on channel ranges -> (dw HWIO [k,k,cin,cout], db [cout]) device tensors."""
        B, H, W, _ = xbuf.shape
        xv, dv = self._view(xbuf, x_coff, cin), self._view(dybuf, dy_coff, cout)
        dw = self.empty((k, k, cin, cout), torch.float32)
        db = self.empty((cout,), torch.float32)
        self.check(self.lib.sr_conv2d_wgrad_views(self.h, C.byref(xv), C.byref(dv), B, H, W, int(cin), int(cout), int(k), dw.data_ptr(), db.data_ptr(), self.stream()))
        return dw, db

    def eltwise_view(self, op, abuf, a_coff, bbuf, b_coff, obuf, o_coff, c, alpha=1.0, beta=0.0):
        """sr_eltwise over c channels of every pixel: out range = op(a range, b range) (bbuf None for one-operand ops)."""
        B, H, W, _ = abuf.shape
        av, ov = self._view(abuf, a_coff, c), self._view(obuf, o_coff, c)
        bv = None if bbuf is None else self._view(bbuf, b_coff, c)
        self.check(self.lib.sr_eltwise_views(self.h, int(op), C.byref(av), None if bv is None else C.byref(bv), float(alpha), float(beta), C.byref(ov), B * H * W, int(c),
                                             self.stream()))

    # ------------------------------------------------------------------ backward-pass pieces (sr355/train.py)
    def conv2d_wgrad(self, x, dy, k, out=None):
        """Kernel and bias gradient of Conv2D(k x k, SAME, stride 1): x [B,H,W,Cin], dy [B,H,W,Cout] fp32 -> (dw HWIO, db) device tensors
        (out: a (dw, db) pair to write into, views of a flat gradient bucket for instance)."""
        _check_tensor(self, x, "wgrad x")
        _check_tensor(self, dy, "wgrad dy")
        B, H, W, cin = x.shape
        if tuple(dy.shape[:3]) != (B, H, W):
            raise ValueError("wgrad: x and dy must share [B,H,W]")
        cout = dy.shape[3]
        if out is None:
            dw = self.empty((k, k, cin, cout), torch.float32)
            db = self.empty((cout,), torch.float32)
        else:
            dw, db = out
            _check_tensor(self, dw, "wgrad out dw")
            _check_tensor(self, db, "wgrad out db")
            if tuple(dw.shape) != (k, k, cin, cout) or tuple(db.shape) != (cout,):
                raise ValueError("wgrad: out must be (dw [k,k,Cin,Cout], db [Cout])")
        self.check(self.lib.sr_conv2d_wgrad(self.h, x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, int(k), dw.data_ptr(), db.data_ptr(), self.stream()))
        return dw, db

    def conv2d_wgrad_maps(self, x, dy, out=None):
        """conv2d_wgrad of a 3x3 layer on maps of at most 8 x 8 (sr_conv2d_wgrad_maps: several images per staged tile)."""
        _check_tensor(self, x, "wgrad_maps x")
        _check_tensor(self, dy, "wgrad_maps dy")
        if x.dim() != 4 or dy.dim() != 4 or tuple(dy.shape[:3]) != tuple(x.shape[:3]):
            raise ValueError("wgrad_maps: x and dy must share [B,H,W]")
        B, H, W, cin = x.shape
        cout = dy.shape[3]
        if H > 8 or W > 8:
            raise ValueError(f"wgrad_maps: maps of at most 8 x 8, got {H} x {W}")
        if out is None:
            dw, db = self.empty((3, 3, cin, cout), torch.float32), self.empty((cout,), torch.float32)
        else:
            dw, db = out
            _check_tensor(self, dw, "wgrad_maps out dw")
            _check_tensor(self, db, "wgrad_maps out db")
            if tuple(dw.shape) != (3, 3, cin, cout) or tuple(db.shape) != (cout,):
                raise ValueError("wgrad_maps: out must be (dw [3,3,Cin,Cout], db [Cout])")
        self.check(self.lib.sr_conv2d_wgrad_maps(self.h, x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, dw.data_ptr(), db.data_ptr(), self.stream()))
        return dw, db

    def eltwise(self, op, a, b=None, alpha=1.0, beta=0.0):
        """Element-wise halves of the chain rule (L.ELT_*): fp32 tensors of one shape -> new tensor."""
        _check_tensor(self, a, "eltwise a")
        if b is not None:
            _check_tensor(self, b, "eltwise b")
            if b.shape != a.shape:
                raise ValueError("eltwise operands must have the same shape")
        out = torch.empty_like(a)
        self.check(self.lib.sr_eltwise(self.h, int(op), a.data_ptr(), None if b is None else b.data_ptr(), float(alpha), float(beta), out.data_ptr(),
                                       a.numel(), self.stream()))
        return out

    def adam_step(self, w, g, m, v, lr_t, beta_1=0.9, beta_2=0.999, epsilon=1e-7, grad_scale=1.0):
        """In-place Keras-Adam update of the flat fp32 device bucket w with gradient g and moments m, v (sr_adam)."""
        import numpy as np
        for t, what in ((w, "adam w"), (g, "adam g"), (m, "adam m"), (v, "adam v")):
            _check_tensor(self, t, what)
            if t.dtype != torch.float32 or t.numel() != w.numel():
                raise ValueError("adam_step: four fp32 tensors of one size")
        f = lambda x: float(np.float32(x))
        self.check(self.lib.sr_adam(self.h, w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), f(lr_t), f(beta_1), f(1.0 - beta_1),
                                    f(beta_2), f(1.0 - beta_2), f(epsilon), f(grad_scale), self.stream()))

    # ------------------------------------------------------------------ mixed-precision training pieces (sr355/train.py, edsr_loss_and_grads_bf16)
    _BF16 = (torch.bfloat16,)

    def conv2d_dev_bf16(self, x, w_dev, b_dev, cout, rot=False, act="linear", d2s=1, alpha=1.0, skip1=None, beta1=0.0, skip2=None, beta2=0.0):
        """conv2d_dev on bf16 tensors with the fp32 DEVICE kernel w_dev ([K,K,Cin,Cout], or with rot=True the forward kernel [K,K,Cout,Cin] of the layer whose
        input gradient is wanted) and fp32 bias: the kernel is rounded to bf16 once on the device, the conv accumulates in fp32, applies
        alpha * act(conv + b) + beta1 * skip1 + beta2 * skip2 in fp32 and rounds once (sr_conv2d_dev_bf16)."""
        _check_tensor(self, x, "conv2d_dev_bf16 input", self._BF16)
        _check_tensor(self, w_dev, "conv2d_dev_bf16 kernel")
        if b_dev is not None:
            _check_tensor(self, b_dev, "conv2d_dev_bf16 bias")
        if x.dim() != 4 or w_dev.dim() != 4:
            raise ValueError("conv2d_dev_bf16: x must be [B,H,W,C], the kernel [K,K,I,O]")
        B, H, W, Cx = x.shape
        k = w_dev.shape[0]
        want = (k, k, cout, Cx) if rot else (k, k, Cx, cout)
        if tuple(w_dev.shape) != want:
            raise ValueError(f"conv2d_dev_bf16: kernel shape {tuple(w_dev.shape)} does not match {want}")
        r = max(1, int(d2s))
        for nm, sk in (("skip1", skip1), ("skip2", skip2)):
            if sk is not None:
                _check_tensor(self, sk, f"conv2d_dev_bf16 {nm}", self._BF16)
                if tuple(sk.shape) != (B, H * r, W * r, cout // (r * r)):
                    raise ValueError(f"conv2d_dev_bf16: {nm} must have the output's shape")
        y = self.empty((B, H * r, W * r, cout // (r * r)), torch.bfloat16)
        actc = {"linear": L.ACT_LINEAR, None: L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}[act]
        self.check(self.lib.sr_conv2d_dev_bf16(self.h, x.data_ptr(), B, H, W, Cx, w_dev.data_ptr(), None if b_dev is None else b_dev.data_ptr(), k,
                                               int(cout), int(bool(rot)), actc, float(alpha), None if skip1 is None else skip1.data_ptr(), float(beta1),
                                               None if skip2 is None else skip2.data_ptr(), float(beta2), 0, r, y.data_ptr(), self.stream()))
        return y

    def conv_prepack_bf16(self, packed_list):
        """sr_conv_prepack_bf16: conv_prepack for conv2d_dev_bf16 (a pack_list; None forgets the bf16 list).  The fp32 list of conv_prepack is a separate one."""
        if packed_list is None:
            self.check(self.lib.sr_conv_prepack_bf16(self.h, None, 0, self.stream()))
            return
        arr, n, _ = packed_list
        self.check(self.lib.sr_conv_prepack_bf16(self.h, arr, n, self.stream()))

    def conv2d_wgrad_bf16(self, x, dy, k=3, scale=1.0, cin=None, out=None):
        """Kernel and bias gradient of Conv2D(3 x 3, SAME, stride 1) from bf16 x [B,H,W,Cx] and dy [B,H,W,Cout] -> fp32 (dw HWIO, db), both times `scale`
        (sr_conv2d_wgrad_bf16).  cin: the channels of x that count (x a channel-padded buffer; default all).  out: a (dw, db) pair to write into."""
        _check_tensor(self, x, "wgrad_bf16 x", self._BF16)
        _check_tensor(self, dy, "wgrad_bf16 dy", self._BF16)
        if x.dim() != 4 or dy.dim() != 4 or tuple(dy.shape[:3]) != tuple(x.shape[:3]):
            raise ValueError("wgrad_bf16: x and dy must share [B,H,W]")
        if int(k) != 3:
            raise ValueError("wgrad_bf16: 3x3 layers only")
        B, H, W, cx = x.shape
        cin = cx if cin is None else int(cin)
        if not 0 < cin <= cx:
            raise ValueError(f"wgrad_bf16: cin {cin} outside the buffer's {cx} channels")
        cout = dy.shape[3]
        if out is None:
            dw, db = self.empty((3, 3, cin, cout), torch.float32), self.empty((cout,), torch.float32)
        else:
            dw, db = out
            _check_tensor(self, dw, "wgrad_bf16 out dw")
            _check_tensor(self, db, "wgrad_bf16 out db")
            if tuple(dw.shape) != (3, 3, cin, cout) or tuple(db.shape) != (cout,):
                raise ValueError("wgrad_bf16: out must be (dw [3,3,Cin,Cout], db [Cout])")
        self.check(self.lib.sr_conv2d_wgrad_bf16(self.h, x.data_ptr(), cx, dy.data_ptr(), cout, B, H, W, cin, cout, 3, float(scale), dw.data_ptr(), db.data_ptr(),
                                                 self.stream()))
        return dw, db

    # ---- the same on channel ranges of bf16 buffers (sr355/gan_train.py, Tape.trunk_bf16: a dense block's virtual-concat buffers)
    def cu_count(self):
        """Compute units of the context's GPU (the pixel-split counts of the weight-gradient kernels follow it)."""
        return int(torch.cuda.get_device_properties(self.torch_device).multi_processor_count)

    @staticmethod
    def _view_bf16(t, coff, c):
        """(tensor [B,H,W,Cbuf] bf16 contiguous, first channel, channels) -> sr_view (in bf16 elements)."""
        if not (isinstance(t, torch.Tensor) and t.dim() == 4 and t.dtype == torch.bfloat16 and t.is_contiguous() and t.is_cuda):
            raise ValueError("a bf16 view needs a contiguous bf16 NHWC device tensor")
        if coff < 0 or c <= 0 or coff + c > t.shape[3]:
            raise ValueError(f"channel range [{coff}, {coff + c}) outside the buffer's {t.shape[3]} channels")
        return L.View(t.data_ptr(), int(t.shape[3]), int(coff))

    def conv2d_dev_view_bf16(self, xbuf, x_coff, cin, w_dev, b_dev, cout, ybuf, y_coff, rot=False, act="linear", alpha=1.0, skip1=None, beta1=0.0, skip2=None, beta2=0.0):
        """conv2d_dev_view on bf16 buffers with the fp32 device kernel w_dev (sr_conv2d_dev_views_bf16): reads xbuf[..., x_coff : x_coff + cin], writes
        ybuf[..., y_coff : y_coff + cout] = bf16(alpha * act(conv + b) + beta1 * skip1 + beta2 * skip2); skip1 / skip2: (buffer, first channel) or None -- a skip may be
        the output range itself.  Channel offsets and buffer widths are multiples of 8, cin a multiple of 32."""
        B, H, W, _ = xbuf.shape
        if tuple(ybuf.shape[:3]) != (B, H, W):
            raise ValueError("conv2d_dev_view_bf16: input and output buffers must share [B,H,W]")
        _check_tensor(self, w_dev, "conv2d_dev_view_bf16 kernel")
        if b_dev is not None:
            _check_tensor(self, b_dev, "conv2d_dev_view_bf16 bias")
        k = w_dev.shape[0]
        want = (k, k, cout, cin) if rot else (k, k, cin, cout)
        if tuple(w_dev.shape) != want:
            raise ValueError(f"conv2d_dev_view_bf16: kernel shape {tuple(w_dev.shape)} does not match {want}")
        xv, yv = self._view_bf16(xbuf, x_coff, cin), self._view_bf16(ybuf, y_coff, cout)
        svs = []
        for sk in (skip1, skip2):
            if sk is not None and tuple(sk[0].shape[:3]) != (B, H, W):
                raise ValueError("conv2d_dev_view_bf16: a skip buffer must share [B,H,W]")
            svs.append(None if sk is None else self._view_bf16(sk[0], sk[1], cout))
        actc = {"linear": L.ACT_LINEAR, None: L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}[act]
        self.check(self.lib.sr_conv2d_dev_views_bf16(self.h, C.byref(xv), B, H, W, int(cin), w_dev.data_ptr(), None if b_dev is None else b_dev.data_ptr(), k, int(cout),
                                                     int(bool(rot)), actc, float(alpha), None if svs[0] is None else C.byref(svs[0]), float(beta1),
                                                     None if svs[1] is None else C.byref(svs[1]), float(beta2), C.byref(yv), self.stream()))

    def conv2d_wgrad_group_bf16(self, jobs):
        """The kernel and bias gradients of up to 8 3x3 layers that share [B,H,W] by one main and one finish launch (sr_conv2d_wgrad_group_bf16).
        jobs: [(xbuf, x_coff, cin, dybuf, dy_coff, cout, scale, dw fp32 [3,3,cin,cout], db fp32 [cout] or None)] on bf16 buffers; dw / db are written in place
        (views of a flat gradient bucket)."""
        if not jobs:
            raise ValueError("wgrad_group_bf16: at least one job")
        arr = (L.WgradJob * len(jobs))()
        B, H, W, _ = jobs[0][0].shape
        for d, (xbuf, x_coff, cin, dybuf, dy_coff, cout, scale, dw, db) in zip(arr, jobs):
            if tuple(xbuf.shape[:3]) != (B, H, W) or tuple(dybuf.shape[:3]) != (B, H, W):
                raise ValueError("wgrad_group_bf16: every buffer must share [B,H,W]")
            _check_tensor(self, dw, "wgrad_group_bf16 dw")
            if tuple(dw.shape) != (3, 3, cin, cout):
                raise ValueError(f"wgrad_group_bf16: dw must be [3,3,{cin},{cout}], got {tuple(dw.shape)}")
            if db is not None:
                _check_tensor(self, db, "wgrad_group_bf16 db")
                if tuple(db.shape) != (cout,):
                    raise ValueError(f"wgrad_group_bf16: db must be [{cout}]")
            d.x, d.dy = self._view_bf16(xbuf, x_coff, cin), self._view_bf16(dybuf, dy_coff, cout)
            d.Cin, d.Cout, d.scale = int(cin), int(cout), float(scale)
            d.dw, d.db = dw.data_ptr(), (None if db is None else db.data_ptr())
        self.check(self.lib.sr_conv2d_wgrad_group_bf16(self.h, arr, len(jobs), B, H, W, self.stream()))

    def eltwise_view_bf16(self, op, abuf, a_coff, bbuf, b_coff, obuf, o_coff, c, alpha=1.0, beta=0.0):
        """sr_eltwise_views_bf16 over c channels of every pixel of bf16 buffers: L.ELT_RELU_BWD (out = a where b > 0, else 0: a select on bits) or L.ELT_AXPBY
        (out = bf16(alpha * a + beta * b), bbuf None for alpha * a)."""
        B, H, W, _ = abuf.shape
        av, ov = self._view_bf16(abuf, a_coff, c), self._view_bf16(obuf, o_coff, c)
        bv = None if bbuf is None else self._view_bf16(bbuf, b_coff, c)
        for t in (bbuf, obuf):
            if t is not None and tuple(t.shape[:3]) != (B, H, W):
                raise ValueError("eltwise_view_bf16: every buffer must share [B,H,W]")
        self.check(self.lib.sr_eltwise_views_bf16(self.h, int(op), C.byref(av), None if bv is None else C.byref(bv), float(alpha), float(beta), C.byref(ov), B * H * W, int(c),
                                                  self.stream()))

    # ---- a G = 8 dense block trained on the LDS-resident image (csrc/dense_block_train.hip; sr355/gan_train.py, Tape.trunk_lds)
    @staticmethod
    def dense_block_train_max_pixels():
        """The largest (H + 2)(W + 2) dense_block_bwd_bf16 takes (sr_dense_block_train_max_pixels)."""
        return int(L.load().sr_dense_block_train_max_pixels())

    @classmethod
    def dense_block_train_fits(cls, H, W):
        """Whether the LDS-resident training kernels take an H x W image: the forward's LDS bound and the backward's pixel bound."""
        return cls.dense_block_lds_bytes(8, H, W) != -1 and (int(H) + 2) * (int(W) + 2) <= cls.dense_block_train_max_pixels()

    @staticmethod
    def dense_block_pack_sizes():
        """(bytes of the forward fragments, floats of the bias table, bytes of the input-gradient fragments) of one packed block (sr_dense_block_pack_sizes)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.load().sr_dense_block_pack_sizes(C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def dense_block_pack_table(self, blocks):
        """blocks: per dense block ([five fp32 HWIO device kernels], [five fp32 device biases]) -> the device pointer table sr_dense_block_pack_dev reads.  The
        caller keeps the tensors alive and in place for as long as it uses the table."""
        rows = []
        for ks, bs in blocks:
            if len(ks) != 5 or len(bs) != 5:
                raise ValueError("dense_block_pack_table: five kernels and five biases per block")
            for i, (k, b) in enumerate(zip(ks, bs)):
                _check_tensor(self, k, "dense_block_pack_table kernel")
                _check_tensor(self, b, "dense_block_pack_table bias")
                want = (3, 3, 64 + 8 * i, 8) if i < 4 else (3, 3, 96, 64)
                if tuple(k.shape) != want or tuple(b.shape) != (want[3],):
                    raise ValueError(f"dense_block_pack_table: conv{i + 1} must be {want} with a bias of {want[3]}, got {tuple(k.shape)} and {tuple(b.shape)}")
            rows.append([k.data_ptr() for k in ks] + [b.data_ptr() for b in bs])
        return self.to_device(np.asarray(rows, np.int64))

    def dense_block_pack_buffers(self, nblocks):
        """Uninitialised (fwd uint8 [n, bytes], bias fp32 [n, floats], bwd uint8 [n, bytes]) for dense_block_pack_dev."""
        fb, nb, bb = self.dense_block_pack_sizes()
        return self.empty((nblocks, fb), torch.uint8), self.empty((nblocks, nb), torch.float32), self.empty((nblocks, bb), torch.uint8)

    def dense_block_pack_dev(self, table, fwd, bias, bwd):
        """sr_dense_block_pack_dev: one launch packs the current weights of every block of `table` (dense_block_pack_table) into fwd / bias / bwd
        (dense_block_pack_buffers)."""
        n = int(table.shape[0])
        fb, nb, bb = self.dense_block_pack_sizes()
        if table.dtype != torch.int64 or tuple(table.shape) != (n, 10) or not table.is_cuda or not table.is_contiguous():
            raise ValueError("dense_block_pack_dev: the table is an int64 device tensor [n, 10]")
        for t, shape, dt in ((fwd, (n, fb), torch.uint8), (bias, (n, nb), torch.float32), (bwd, (n, bb), torch.uint8)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shape):
                raise ValueError(f"dense_block_pack_dev: a pack buffer must be a contiguous device tensor {shape} of {dt}")
        self.check(self.lib.sr_dense_block_pack_dev(self.h, table.data_ptr(), n, fwd.data_ptr(), bias.data_ptr(), bwd.data_ptr(), self.stream()))

    def dense_block_fwd_bf16(self, fwd_w, bias, F, out, out_coff=0, skip2=None, alpha=0.2, beta1=1.0, beta2=0.0):
        """sr_dense_block_fwd_bf16: a whole G = 8 dense block on the bf16 NHWC concat buffer F [B,H,W,>=96] as ONE kernel: reads F[..., :64], writes the four growth
        slices into F[..., 64:96] and out[..., out_coff : out_coff + 64] = bf16(alpha * (conv5 + b5) + beta1 * F[..., :64] + beta2 * skip2); skip2: (buffer, first
        channel) or None.  fwd_w / bias: one block's rows of dense_block_pack_dev's buffers."""
        B, H, W, _ = F.shape
        self._view_bf16(F, 0, 96)
        ov = self._view_bf16(out, out_coff, 64)
        sv = None if skip2 is None else self._view_bf16(skip2[0], skip2[1], 64)
        for t in (out,) + (() if skip2 is None else (skip2[0],)):
            if tuple(t.shape[:3]) != (B, H, W):
                raise ValueError("dense_block_fwd_bf16: every buffer must share [B,H,W]")
        self.check(self.lib.sr_dense_block_fwd_bf16(self.h, fwd_w.data_ptr(), bias.data_ptr(), F.data_ptr(), int(F.shape[3]), B, H, W, C.byref(ov),
                                                    None if sv is None else C.byref(sv), float(alpha), float(beta1), float(beta2), self.stream()))

    def dense_block_bwd_bf16(self, bwd_w, dY, F, a5, bx, dz, dX, dy_coff=0, dx_coff=0, stages=None):
        """sr_dense_block_bwd_bf16: the whole backward of that block's activations as ONE kernel, from dY[..., dy_coff : dy_coff + 64] and the stored F: writes
        dz [B,H,W,32] (dz_k in slice k - 1) and dX[..., dx_coff : dx_coff + 64]; stages: None or a bf16 [4,B,H,W,96] receiving G after conv5's input gradient and
        after each in-place accumulate.  bwd_w: one block's row of dense_block_pack_dev's bwd buffer."""
        B, H, W, _ = F.shape
        self._view_bf16(F, 0, 96)
        yv, xv = self._view_bf16(dY, dy_coff, 64), self._view_bf16(dX, dx_coff, 64)
        self._view_bf16(dz, 0, 32)
        if tuple(dz.shape) != (B, H, W, 32) or tuple(dY.shape[:3]) != (B, H, W) or tuple(dX.shape[:3]) != (B, H, W):
            raise ValueError("dense_block_bwd_bf16: dY and dX share F's [B,H,W], dz is [B,H,W,32]")
        if stages is not None and not (stages.dtype == torch.bfloat16 and stages.is_cuda and stages.is_contiguous() and tuple(stages.shape) == (4, B, H, W, 96)):
            raise ValueError("dense_block_bwd_bf16: stages is a contiguous bf16 device tensor [4,B,H,W,96]")
        self.check(self.lib.sr_dense_block_bwd_bf16(self.h, bwd_w.data_ptr(), C.byref(yv), F.data_ptr(), int(F.shape[3]), B, H, W, float(a5), float(bx), dz.data_ptr(),
                                                    C.byref(xv), None if stages is None else stages.data_ptr(), self.stream()))

    def relu_bwd_bf16(self, dy, y):
        """dy where y > 0, else 0, on bf16 tensors of one shape (sr_relu_bwd_bf16)."""
        _check_tensor(self, dy, "relu_bwd_bf16 dy", self._BF16)
        _check_tensor(self, y, "relu_bwd_bf16 y", self._BF16)
        if y.shape != dy.shape:
            raise ValueError("relu_bwd_bf16: operands must have the same shape")
        out = torch.empty_like(dy)
        self.check(self.lib.sr_relu_bwd_bf16(self.h, dy.data_ptr(), y.data_ptr(), out.data_ptr(), dy.numel(), self.stream()))
        return out

    # ---- 3x3 convs over many small images (sr_conv3x3_small_bf16: the 3 x 3 and 6 x 6 images of the VGG19 extractor's blocks 4-5 on training patches; gan_train.small_conv_wins says which calls)
    SMALL_CONV_MAX_PIXELS = 144

    @classmethod
    def small_conv_takes(cls, H, W, cin, cout):
        """The shape class of sr_conv3x3_small_bf16: images of at most 144 pixels, channel counts multiples of 32."""
        return H >= 1 and W >= 1 and H * W <= cls.SMALL_CONV_MAX_PIXELS and cin > 0 and cout > 0 and cin % 32 == 0 and cout % 32 == 0

    def conv3x3_small_pack(self, w_dev, rot=False):
        """The packed-kernel handle of conv3x3_small_bf16 for the fp32 device kernel w_dev ([3,3,Cin,Cout], or with rot=True the forward kernel of the layer whose
        input gradient is wanted): a bf16 tensor the caller keeps for as long as the weights stand (sr_conv3x3_small_pack_bf16)."""
        _check_tensor(self, w_dev, "conv3x3_small_pack kernel")
        if w_dev.dim() != 4 or tuple(w_dev.shape[:2]) != (3, 3):
            raise ValueError("conv3x3_small_pack: the kernel must be [3,3,I,O]")
        cin, cout = (int(w_dev.shape[3]), int(w_dev.shape[2])) if rot else (int(w_dev.shape[2]), int(w_dev.shape[3]))
        nbytes = int(self.lib.sr_conv3x3_small_pack_bytes(cin, cout))
        packed = self.empty((max(nbytes, 2) // 2,), torch.bfloat16)
        self.check(self.lib.sr_conv3x3_small_pack_bf16(self.h, w_dev.data_ptr(), cin, cout, int(bool(rot)), packed.data_ptr(), self.stream()))
        return packed

    def conv3x3_small_bf16(self, x, w_dev, b_dev, cout, rot=False, act="linear", mask=None, packed=None):
        """bf16 x [B,H,W,Cin] (H * W <= 144, Cin and cout multiples of 32) -> bf16(act(conv3x3(x) + b)), zeroed where mask <= 0 (sr_conv3x3_small_bf16).  The
        kernel comes from w_dev as conv2d_dev_bf16 takes it, or from a handle of conv3x3_small_pack (then w_dev may be None)."""
        _check_tensor(self, x, "conv3x3_small_bf16 input", self._BF16)
        if x.dim() != 4:
            raise ValueError("conv3x3_small_bf16: x must be [B,H,W,C]")
        B, H, W, Cx = x.shape
        if packed is None:
            _check_tensor(self, w_dev, "conv3x3_small_bf16 kernel")
            want = (3, 3, cout, Cx) if rot else (3, 3, Cx, cout)
            if tuple(w_dev.shape) != want:
                raise ValueError(f"conv3x3_small_bf16: kernel shape {tuple(w_dev.shape)} does not match {want}")
        else:
            _check_tensor(self, packed, "conv3x3_small_bf16 packed kernel", self._BF16)
            if packed.numel() * 2 != int(self.lib.sr_conv3x3_small_pack_bytes(Cx, int(cout))):
                raise ValueError("conv3x3_small_bf16: the packed kernel was made for other channel counts")
        if b_dev is not None:
            _check_tensor(self, b_dev, "conv3x3_small_bf16 bias")
            if b_dev.numel() != cout:
                raise ValueError("conv3x3_small_bf16: the bias must have one value per output channel")
        if mask is not None:
            _check_tensor(self, mask, "conv3x3_small_bf16 mask", self._BF16)
            if tuple(mask.shape) != (B, H, W, cout):
                raise ValueError("conv3x3_small_bf16: the mask must have the output's shape")
        if act not in ("linear", None, "relu"):
            raise ValueError("conv3x3_small_bf16: act is 'linear' or 'relu'")
        y = self.empty((B, H, W, cout), torch.bfloat16)
        self.check(self.lib.sr_conv3x3_small_bf16(self.h, x.data_ptr(), B, H, W, Cx, None if packed is not None else w_dev.data_ptr(),
                                                  None if packed is None else packed.data_ptr(), None if b_dev is None else b_dev.data_ptr(), int(cout),
                                                  int(bool(rot)), L.ACT_RELU if act == "relu" else L.ACT_LINEAR, None if mask is None else mask.data_ptr(),
                                                  y.data_ptr(), self.stream()))
        return y

    # ---- the other kernels of the bf16 perceptual branch (sr355/gan_train.py, PerceptualBf16)
    def vgg_preprocess_bf16(self, fake, hr):
        """fake, hr fp32 [B,H,W,3] in [-1,1] -> bf16 [2B,H,W,6], fake first: caffe preprocessing as a hi + lo pair of bf16 (sr_vgg_preprocess_bf16)."""
        _check_tensor(self, fake, "vgg_preprocess_bf16 fake")
        _check_tensor(self, hr, "vgg_preprocess_bf16 hr")
        if fake.dim() != 4 or fake.shape[3] != 3 or hr.shape != fake.shape:
            raise ValueError("vgg_preprocess_bf16: two [B,H,W,3] tensors of one shape")
        B, H, W, _ = fake.shape
        out = self.empty((2 * B, H, W, 6), torch.bfloat16)
        self.check(self.lib.sr_vgg_preprocess_bf16(self.h, fake.data_ptr(), hr.data_ptr(), B, H, W, out.data_ptr(), self.stream()))
        return out

    def vgg_preprocess_bwd(self, dv):
        """The bf16 gradient [B,H,W,3] of the preprocessed image -> the fp32 gradient of the [-1,1] RGB image (sr_vgg_preprocess_bwd)."""
        _check_tensor(self, dv, "vgg_preprocess_bwd dv", self._BF16)
        if dv.dim() != 4 or dv.shape[3] != 3:
            raise ValueError("vgg_preprocess_bwd: dv must be [B,H,W,3]")
        out = self.empty(dv.shape, torch.float32)
        self.check(self.lib.sr_vgg_preprocess_bwd(self.h, dv.data_ptr(), dv.numel() // 3, out.data_ptr(), self.stream()))
        return out

    def maxpool2_bf16(self, x):
        """MaxPooling2D(2,2) VALID on bf16 [B,H,W,C] (sr_maxpool2_bf16)."""
        _check_tensor(self, x, "maxpool2_bf16 input", self._BF16)
        if x.dim() != 4:
            raise ValueError("maxpool2_bf16: x must be [B,H,W,C]")
        B, H, W, Cx = x.shape
        y = self.empty((B, H // 2, W // 2, Cx), torch.bfloat16)
        self.check(self.lib.sr_maxpool2_bf16(self.h, x.data_ptr(), B, H, W, Cx, y.data_ptr(), self.stream()))
        return y

    def maxpool2_bwd_bf16(self, x, dy):
        """dy routed to each window's winner where the pre-pool activation x is positive, else 0 (sr_maxpool2_bwd_bf16)."""
        _check_tensor(self, x, "maxpool2_bwd_bf16 x", self._BF16)
        _check_tensor(self, dy, "maxpool2_bwd_bf16 dy", self._BF16)
        if x.dim() != 4 or tuple(dy.shape) != (x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]):
            raise ValueError("maxpool2_bwd_bf16: dy must be [B,H/2,W/2,C] of x [B,H,W,C]")
        B, H, W, Cx = x.shape
        dx = torch.empty_like(x)
        self.check(self.lib.sr_maxpool2_bwd_bf16(self.h, x.data_ptr(), dy.data_ptr(), B, H, W, Cx, dx.data_ptr(), self.stream()))
        return dx

    def mse_grad_bf16(self, feats):
        """feats bf16 [2B,...] = [ff | fr] -> (perc fp32 [1] = mean((ff - fr)^2), dff bf16 [B,...] = 2 / n * (ff - fr) where ff > 0, else 0) (sr_mse_grad_bf16)."""
        _check_tensor(self, feats, "mse_grad_bf16 feats", self._BF16)
        if feats.dim() < 1 or feats.shape[0] % 2:
            raise ValueError("mse_grad_bf16: the leading axis holds the two halves of the batch")
        half = feats.shape[0] // 2
        perc = self.empty((1,), torch.float32)
        dff = self.empty((half,) + tuple(feats.shape[1:]), torch.bfloat16)
        self.check(self.lib.sr_mse_grad_bf16(self.h, feats.data_ptr(), dff.numel(), perc.data_ptr(), dff.data_ptr(), self.stream()))
        return perc, dff

    def space_to_depth_bf16(self, x, r):
        """space_to_depth on a bf16 tensor (sr_space_to_depth_bf16)."""
        _check_tensor(self, x, "space_to_depth_bf16 input", self._BF16)
        if x.dim() != 4:
            raise ValueError("space_to_depth_bf16: x must be [B,H,W,C]")
        B, Hr, Wr, Cx = x.shape
        r = int(r)
        if r < 1 or Hr % r or Wr % r:
            raise ValueError("space_to_depth_bf16: spatial size not divisible by the block")
        y = self.empty((B, Hr // r, Wr // r, r * r * Cx), torch.bfloat16)
        self.check(self.lib.sr_space_to_depth_bf16(self.h, x.data_ptr(), B, Hr // r, Wr // r, Cx, r, y.data_ptr(), self.stream()))
        return y

    def mse_clip_grad_bf16(self, pre, t, want_y=True):
        """pre bf16, t fp32 (same shape) -> (y fp32 = clip(pre, 0, 1) or None, loss fp32 [1] = mean((y - t)^2), dpre bf16 = 2 / n * (y - t) inside the clip
        range, else 0) by one kernel and its reduction (sr_mse_clip_grad_bf16)."""
        _check_tensor(self, pre, "mse_clip_grad_bf16 pre", self._BF16)
        _check_tensor(self, t, "mse_clip_grad_bf16 target")
        if t.shape != pre.shape:
            raise ValueError("mse_clip_grad_bf16: pre and the target must have the same shape")
        loss = self.empty((1,), torch.float32)
        dpre = torch.empty_like(pre)
        y = torch.empty_like(t) if want_y else None
        self.check(self.lib.sr_mse_clip_grad_bf16(self.h, pre.data_ptr(), t.data_ptr(), pre.numel(), loss.data_ptr(), dpre.data_ptr(),
                                                  None if y is None else y.data_ptr(), self.stream()))
        return y, loss, dpre

    def space_to_depth(self, x, r):
        """Inverse of tf.nn.depth_to_space (DCR): [B,H*r,W*r,C] -> [B,H,W,r*r*C]."""
        _check_tensor(self, x, "space_to_depth input")
        B, Hr, Wr, Cx = x.shape
        if Hr % r or Wr % r:
            raise ValueError("space_to_depth: spatial size not divisible by the block")
        y = self.empty((B, Hr // r, Wr // r, r * r * Cx), torch.float32)
        self.check(self.lib.sr_space_to_depth(self.h, x.data_ptr(), B, Hr // r, Wr // r, Cx, int(r), y.data_ptr(), self.stream()))
        return y

    def spatial_op(self, op, x):
        """L.SP_MAXPOOL2 / SP_GAP / SP_PICK2 / SP_VGG_PREPROCESS on an fp32 [B,H,W,C] tensor."""
        _check_tensor(self, x, "spatial op input")
        B, H, W, Cx = x.shape
        shape = {L.SP_MAXPOOL2: (B, H // 2, W // 2, Cx), L.SP_GAP: (B, Cx), L.SP_PICK2: (B, (H + 1) // 2, (W + 1) // 2, Cx),
                 L.SP_VGG_PREPROCESS: (B, H, W, Cx)}[op]
        y = self.empty(shape, torch.float32)
        self.check(self.lib.sr_spatial_op(self.h, int(op), x.data_ptr(), B, H, W, Cx, y.data_ptr(), self.stream()))
        return y

    def matmul(self, a, b, trans_a=False, trans_b=False, alpha=1.0):
        """Batched fp32 product alpha * op(a) @ op(b): a [batch, M, K] (or [batch, K, M] when trans_a), b likewise."""
        _check_tensor(self, a, "matmul a")
        _check_tensor(self, b, "matmul b")
        if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0]:
            raise ValueError("matmul operands must be [batch, rows, cols] with equal batch")
        M, K = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
        K2, N = (b.shape[2], b.shape[1]) if trans_b else (b.shape[1], b.shape[2])
        if K != K2:
            raise ValueError("matmul inner dimensions differ")
        c = self.empty((a.shape[0], M, N), torch.float32)
        self.check(self.lib.sr_matmul(self.h, a.data_ptr(), b.data_ptr(), c.data_ptr(), a.shape[0], M, N, K, int(trans_a), int(trans_b), float(alpha), self.stream()))
        return c

    # ------------------------------------------------------------------ classifier training (FineTunedVGG16.fit, VGG16_model.py:111-157)
    @staticmethod
    def warp_params(rot, offset, flip):
        """Per-image affine parameters for affine_warp: rot [n,2,2], offset [n,2] (fp64: output pixel o samples rot @ o + offset) and
        flip [n] (mirror the columns after the warp) -> fp32 [n,16] as sr_affine_warp reads them (fp64 values split into hi + lo)."""
        rot, offset = np.asarray(rot, np.float64).reshape(-1, 4), np.asarray(offset, np.float64).reshape(-1, 2)
        flip = np.asarray(flip, bool).reshape(-1)
        if not len(rot) == len(offset) == len(flip):
            raise ValueError("warp_params: rot, offset and flip must describe the same number of images")
        v = np.concatenate([rot, offset], axis=1)
        hi = v.astype(np.float32)
        out = np.zeros((len(v), 16), np.float32)
        out[:, :6], out[:, 6:12], out[:, 12] = hi, (v - hi).astype(np.float32), flip
        return out

    def affine_warp(self, x, idx, params, out=None):
        """Augmented batch of a device-resident image set (sr_affine_warp): x fp32 [N,H,W,C]; idx int32 [n] rows of x and params fp32 [n,16]
        (warp_params), each a device tensor or a host array (host indices are range-checked before the upload) -> fp32 [n,H,W,C]."""
        _check_tensor(self, x, "affine_warp images")
        if x.dim() != 4:
            raise ValueError("affine_warp: images must be [N,H,W,C]")
        N, H, W, Cx = x.shape
        if not isinstance(idx, torch.Tensor):
            idx = np.asarray(idx)
            if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer) or (len(idx) and (idx.min() < 0 or idx.max() >= N)):
                raise ValueError(f"affine_warp: indices must be integers in [0, {N})")
            idx = self.to_device(idx.astype(np.int32))
        if not isinstance(params, torch.Tensor):
            params = self.to_device(np.asarray(params, np.float32))
        _check_tensor(self, idx, "affine_warp indices", (torch.int32,))
        _check_tensor(self, params, "affine_warp params")
        n = idx.numel()
        if idx.dim() != 1 or tuple(params.shape) != (n, 16):
            raise ValueError(f"affine_warp: indices [n] and params [n,16] expected, got {tuple(idx.shape)} and {tuple(params.shape)}")
        y = self.empty((n, H, W, Cx)) if out is None else out
        _check_tensor(self, y, "affine_warp out")
        if tuple(y.shape) != (n, H, W, Cx):
            raise ValueError("affine_warp: out has the wrong shape")
        self.check(self.lib.sr_affine_warp(self.h, x.data_ptr(), N, H, W, Cx, idx.data_ptr(), n, params.data_ptr(), y.data_ptr(), self.stream()))
        return y

    def dense_head_workspace(self, n, num_classes):
        """Device workspace of dense_head_step for up to n rows (allocate once, before the loop)."""
        nb = self.lib.sr_dense_head_workspace_bytes(int(n), int(num_classes))
        if nb < 0:
            raise ValueError("dense_head_workspace: need n >= 1 and num_classes >= 2")
        return self.empty((nb,), torch.uint8)

    def dense_head_step(self, feats, labels, params, num_classes, stats, work, grads=None, keep0=None, keep1=None, keep_scale=1.0, l2_reg=0.0,
                        dfeats=None):
        """One step of the classifier head (sr_dense_head_step): feats fp32 [n,512], labels int32 [n], params the flat fp32 head bucket; with
        grads (fp32, same size) a training step that writes the gradient of mean sparse CCE + l2_reg sum(k1^2), with uint8 dropout keep masks
        keep0 [n,512] / keep1 [n,256] (optional), else an inference pass.  stats fp64 [3] receives (loss sum, correct rows, sum k1^2).
        dfeats fp32 [n,512] (training steps only): sr_dense_head_step_dx instead -- the same grads and stats, and the gradient at feats."""
        C_ = int(num_classes)
        _check_tensor(self, feats, "dense_head feats")
        _check_tensor(self, labels, "dense_head labels", (torch.int32,))
        _check_tensor(self, params, "dense_head params")
        _check_tensor(self, stats, "dense_head stats", (torch.float64,))
        _check_tensor(self, work, "dense_head workspace", (torch.uint8,))
        if feats.dim() != 2 or feats.shape[1] != 512 or feats.shape[0] < 1:
            raise ValueError(f"dense_head_step: features must be [n,512], got {tuple(feats.shape)}")
        n = feats.shape[0]
        nparam = 512 * 256 + 256 + 256 * C_ + C_
        if C_ < 2 or params.numel() != nparam:
            raise ValueError(f"dense_head_step: params must be the flat head bucket of {nparam} values (num_classes >= 2)")
        if labels.shape != (n,) or stats.numel() != 3:
            raise ValueError("dense_head_step: labels [n] and stats [3] expected")
        if grads is not None:
            _check_tensor(self, grads, "dense_head grads")
            if grads.numel() != nparam:
                raise ValueError("dense_head_step: grads must match params")
        if (keep0 is None) != (keep1 is None) or (keep0 is not None and grads is None):
            raise ValueError("dense_head_step: dropout masks come in pairs, in training steps only")
        if keep0 is not None:
            _check_tensor(self, keep0, "dense_head keep0", (torch.uint8,))
            _check_tensor(self, keep1, "dense_head keep1", (torch.uint8,))
            if keep0.shape != (n, 512) or keep1.shape != (n, 256):
                raise ValueError("dense_head_step: keep masks must be [n,512] and [n,256]")
        ptr = lambda t: None if t is None else t.data_ptr()
        if dfeats is not None:
            _check_tensor(self, dfeats, "dense_head dfeats")
            if grads is None or tuple(dfeats.shape) != (n, 512):
                raise ValueError("dense_head_step: dfeats [n,512] comes with grads, in training steps only")
            self.check(self.lib.sr_dense_head_step_dx(self.h, feats.data_ptr(), n, 512, 256, C_, labels.data_ptr(), ptr(keep0), ptr(keep1), float(keep_scale),
                                                      params.data_ptr(), float(l2_reg), grads.data_ptr(), dfeats.data_ptr(), stats.data_ptr(), work.data_ptr(),
                                                      work.numel(), self.stream()))
            return
        self.check(self.lib.sr_dense_head_step(self.h, feats.data_ptr(), n, 512, 256, C_, labels.data_ptr(), ptr(keep0), ptr(keep1), float(keep_scale),
                                               params.data_ptr(), float(l2_reg), ptr(grads), stats.data_ptr(), work.data_ptr(), work.numel(), self.stream()))

    def pool_gap_bwd(self, a, dfeats):
        """MaxPooling2D(2,2) + GlobalAveragePooling2D + the ReLU in front, backward in one launch (sr_pool_gap_bwd): a fp32 [B,H,W,C] the ReLU
        output, dfeats fp32 [B,C] -> dz fp32 [B,H,W,C] at the pre-activation."""
        _check_tensor(self, a, "pool_gap_bwd a")
        _check_tensor(self, dfeats, "pool_gap_bwd dfeats")
        if a.dim() != 4 or tuple(dfeats.shape) != (a.shape[0], a.shape[3]):
            raise ValueError(f"pool_gap_bwd: a [B,H,W,C] and dfeats [B,C] expected, got {tuple(a.shape)} and {tuple(dfeats.shape)}")
        B, H, W, Cx = a.shape
        dz = torch.empty_like(a)
        self.check(self.lib.sr_pool_gap_bwd(self.h, a.data_ptr(), dfeats.data_ptr(), B, H, W, Cx, dz.data_ptr(), self.stream()))
        return dz

    # ------------------------------------------------------------------ the discriminator's update besides its convs (ESRGAN_model.py:347-377, :475-533)
    @staticmethod
    def spectral_norm_table(bucket, layers):
        """The descriptor table of spectral_norm_bucket for the kernels of `layers` (names, in the order of their u vectors) of a
        train.ParamBucket -> (ctypes array of sr_sn_desc, length of the flat u tensor: the layers' Cout one after the other)."""
        offs, o = {}, 0
        for n, shapes in bucket.shapes.items():
            offs[n] = o
            o += sum(int(np.prod(s)) for s in shapes)
        table, uoff = (L.SnDesc * len(layers))(), 0
        for d, n in zip(table, layers):
            if n not in offs:
                raise KeyError(f"spectral_norm_table: the bucket has no layer {n!r}")
            kshape = bucket.shapes[n][0]
            cout = int(kshape[-1])
            d.koff, d.K, d.Cout, d.uoff = offs[n], int(np.prod(kshape)) // cout, cout, uoff
            uoff += cout
        return table, uoff

    def spectral_norm_bucket(self, flat, u, table):
        """tfa's SpectralNormalization (one power iteration) of every kernel `table` describes, in place in the flat fp32 bucket `flat`, by
        one launch (sr_spectral_norm_bucket); u, the flat fp32 tensor of the layers' power-iteration vectors, moves on with it."""
        _check_tensor(self, flat, "spectral_norm bucket")
        _check_tensor(self, u, "spectral_norm u")
        if flat.dim() != 1 or u.dim() != 1:
            raise ValueError("spectral_norm_bucket: the bucket and u must be flat")
        if not isinstance(table, C.Array) or table._type_ is not L.SnDesc or len(table) < 1:
            raise ValueError("spectral_norm_bucket: table must be a non-empty array of sr_sn_desc (spectral_norm_table)")
        self.check(self.lib.sr_spectral_norm_bucket(self.h, flat.data_ptr(), flat.numel(), u.data_ptr(), u.numel(), table, len(table), self.stream()))

    # ------------------------------------------------------------------ training batches from resident stacks (loading_methods.py:40-191)
    def _patch_side(self, side, ph, pw, B, who):
        """side: dict(stack, pad=(pad_h, pad_w), swap, mul, add) -> (sr_patch_side, the fp32 batch tensor [B,ph,pw,3])."""
        stack = side["stack"]
        _check_tensor(self, stack, f"gather_patch_pairs {who} stack", (torch.float32, torch.uint8))
        if stack.dim() != 4 or stack.shape[3] != 3:
            raise ValueError(f"gather_patch_pairs: the {who} stack must be [N,H,W,3]")
        N, H, W, _ = (int(v) for v in stack.shape)
        pad_h, pad_w = (int(v) for v in side.get("pad", (0, 0)))
        if not (0 <= pad_h <= H - 1 and 0 <= pad_w <= W - 1):
            raise ValueError(f"gather_patch_pairs: {who} reflect padding ({pad_h}, {pad_w}) must lie in 0 .. size - 1 of a {H} x {W} image")
        if ph > H + pad_h or pw > W + pad_w:
            raise ValueError(f"gather_patch_pairs: a {ph} x {pw} patch does not fit the padded {who} image")
        out = self.empty((B, ph, pw, 3), torch.float32)
        s = L.PatchSide(stack.data_ptr(), out.data_ptr(), dtype_code(stack.dtype), N, H, W, pad_h, pad_w, int(bool(side.get("swap", False))),
                        float(side.get("mul", 1.0)), float(side.get("add", 0.0)))
        return s, out

    def gather_patch_pairs(self, lr, hr, windows, order, offset, B, patch, scale=1):
        """One batch of aligned patches cut from device-resident stacks by one launch (sr_gather_patch_pairs).  lr / hr: dict(stack=[N,H,W,3]
        uint8 or fp32 device tensor, pad=(pad_h, pad_w) bottom / right reflect padding, swap=BGR->RGB, mul=1, add=0); hr may be None.
        windows int32 device [n,3] (image, y, x in LR-side pixels), order int32 device [m] rows of windows; the batch is windows
        order[offset : offset + B].  patch: int or (h, w) on the LR side.  -> (X fp32 [B,h,w,3], Y fp32 [B,h*scale,w*scale,3] or None).
        The tables' CONTENTS are the caller's to validate before upload (sr355.patches does); the kernel clamps what it reads."""
        ph, pw = (int(patch), int(patch)) if isinstance(patch, (int, np.integer)) else (int(patch[0]), int(patch[1]))
        offset, B, scale = int(offset), int(B), int(scale)
        _check_tensor(self, windows, "gather_patch_pairs windows", (torch.int32,))
        _check_tensor(self, order, "gather_patch_pairs order", (torch.int32,))
        if windows.dim() != 2 or windows.shape[1] != 3 or windows.shape[0] < 1 or order.dim() != 1:
            raise ValueError("gather_patch_pairs: windows must be int32 [n,3] and order int32 [m]")
        if B < 1 or offset < 0 or offset + B > order.numel():
            raise ValueError(f"gather_patch_pairs: batch [{offset}, {offset + B}) reaches outside an order of {order.numel()} entries")
        if ph < 1 or pw < 1 or scale < 1:
            raise ValueError("gather_patch_pairs: patch and scale must be >= 1")
        a, X = self._patch_side(lr, ph, pw, B, "LR")
        b, Y = self._patch_side(hr, ph * scale, pw * scale, B, "HR") if hr is not None else (None, None)
        if hr is not None and hr["stack"].shape[0] != lr["stack"].shape[0]:
            raise ValueError("gather_patch_pairs: the two stacks hold different numbers of images")
        self.check(self.lib.sr_gather_patch_pairs(self.h, C.byref(a), C.byref(b) if b is not None else None, windows.data_ptr(), int(windows.shape[0]),
                                                  order.data_ptr(), order.numel(), offset, B, ph, pw, scale, self.stream()))
        return X, Y

    def gather_warp_patches(self, stack, windows, order, offset, B, patch, params, swap=False, out=None):
        """One augmented batch of the classifier's fit cut from a device-resident frame stack by one launch (sr_gather_warp_patches): stack
        [N,H,W,3] uint8 or fp32, windows int32 device [n,3] (image, y, x), order int32 device [m] rows of windows, params fp32 [B,16]
        (warp_params; a device tensor or a host array) -> fp32 [B,h,w,3]: element b is affine_warp of the patch gather_patch_pairs cuts for
        window order[offset + b], bit for bit, with every tap clamped to the patch.  patch: int or (h, w).  The tables' CONTENTS are the
        caller's to validate before upload (sr355.patches does); the kernel clamps what it reads."""
        ph, pw = (int(patch), int(patch)) if isinstance(patch, (int, np.integer)) else (int(patch[0]), int(patch[1]))
        offset, B = int(offset), int(B)
        _check_tensor(self, stack, "gather_warp_patches stack", (torch.float32, torch.uint8))
        if stack.dim() != 4 or stack.shape[3] != 3 or stack.shape[0] < 1:
            raise ValueError("gather_warp_patches: the stack must be [N,H,W,3]")
        N, H, W, _ = (int(v) for v in stack.shape)
        _check_tensor(self, windows, "gather_warp_patches windows", (torch.int32,))
        _check_tensor(self, order, "gather_warp_patches order", (torch.int32,))
        if windows.dim() != 2 or windows.shape[1] != 3 or windows.shape[0] < 1 or order.dim() != 1:
            raise ValueError("gather_warp_patches: windows must be int32 [n,3] and order int32 [m]")
        if B < 1 or offset < 0 or offset + B > order.numel():
            raise ValueError(f"gather_warp_patches: batch [{offset}, {offset + B}) reaches outside an order of {order.numel()} entries")
        if ph < 1 or pw < 1 or ph > H or pw > W:
            raise ValueError(f"gather_warp_patches: a {ph} x {pw} patch does not fit a {H} x {W} frame")
        if not isinstance(params, torch.Tensor):
            params = self.to_device(np.asarray(params, np.float32))
        _check_tensor(self, params, "gather_warp_patches params")
        if tuple(params.shape) != (B, 16):
            raise ValueError(f"gather_warp_patches: params [{B},16] expected, got {tuple(params.shape)}")
        y = self.empty((B, ph, pw, 3)) if out is None else out
        _check_tensor(self, y, "gather_warp_patches out")
        if tuple(y.shape) != (B, ph, pw, 3):
            raise ValueError("gather_warp_patches: out has the wrong shape")
        self.check(self.lib.sr_gather_warp_patches(self.h, stack.data_ptr(), dtype_code(stack.dtype), N, H, W, windows.data_ptr(), int(windows.shape[0]),
                                                   order.data_ptr(), order.numel(), offset, B, ph, pw, int(bool(swap)), params.data_ptr(), y.data_ptr(),
                                                   self.stream()))
        return y

    def u8_to_unit(self, stack, swap=False):
        """uint8 [N,H,W,3] device stack -> fp32 [N,H,W,3] in [0,1], float(u) / 255.0f per element: sr_gather_patch_pairs with one whole-image
        window per image."""
        _check_tensor(self, stack, "u8_to_unit input", (torch.uint8,))
        N, H, W, _ = stack.shape
        win = np.zeros((N, 3), np.int32)
        win[:, 0] = np.arange(N)
        return self.gather_patch_pairs(dict(stack=stack, swap=swap), None, self.to_device(win), self.to_device(np.arange(N, dtype=np.int32)), 0, N, (H, W))[0]

    def clip_table(self, bucket):
        """The (offset, length) table of clip_by_norm_bucket for every array of a train.ParamBucket, in parameter order -> int64 device [n_vars,2]."""
        rows, o = [], 0
        for shapes in bucket.shapes.values():
            for shape in shapes:
                size = int(np.prod(shape))
                rows.append((o, size))
                o += size
        return self.to_device(np.asarray(rows, np.int64))

    def clip_by_norm_bucket(self, flat_g, table, clipnorm, scales_out=None):
        """tf.clip_by_norm per variable of the flat fp32 gradient bucket, in place (sr_clip_by_norm_bucket) -> the factors, fp32 device [n_vars]
        (1 where a variable's norm was within clipnorm)."""
        _check_tensor(self, flat_g, "clip_by_norm bucket")
        _check_tensor(self, table, "clip_by_norm table", (torch.int64,))
        if flat_g.dim() != 1 or table.dim() != 2 or table.shape[1] != 2 or table.shape[0] < 1:
            raise ValueError("clip_by_norm_bucket: a flat bucket and an int64 [n_vars,2] table (clip_table)")
        n_vars = int(table.shape[0])
        if scales_out is None:
            scales_out = self.empty((n_vars,), torch.float32)
        _check_tensor(self, scales_out, "clip_by_norm scales")
        if scales_out.numel() != n_vars:
            raise ValueError("clip_by_norm_bucket: scales_out holds one fp32 per variable")
        self.check(self.lib.sr_clip_by_norm_bucket(self.h, flat_g.data_ptr(), flat_g.numel(), table.data_ptr(), n_vars, float(clipnorm), scales_out.data_ptr(),
                                                   self.stream()))
        return scales_out

    DISC_HEAD_PARAMS = 256 * 256 + 256 + 256 + 1

    def disc_head_step(self, h, params, target, loss, grads=None, accumulate=False):
        """The discriminator's head on the last conv's map (sr_disc_head_step): h fp32 [B,H,W,256]; params the head's 66 049 values as they lie
        in the bucket (disc_dense1 kernel, bias, disc_output kernel, bias); target 0 or 1; loss a one-element fp32 view that receives the mean
        binary cross-entropy.  With grads (fp32, the same 66 049 positions of the flat gradient bucket) the parameter gradients are stored
        there, or added onto it with accumulate.  -> (p [B], dh [B,H,W,256] = d loss / d h)."""
        _check_tensor(self, h, "disc_head map")
        _check_tensor(self, params, "disc_head params")
        _check_tensor(self, loss, "disc_head loss")
        if h.dim() != 4 or h.shape[0] < 1 or h.shape[1] < 1 or h.shape[2] < 1:
            raise ValueError(f"disc_head_step: the map must be [B,H,W,256], got {tuple(h.shape)}")
        B, H, W, Cx = h.shape
        if params.dim() != 1 or loss.numel() != 1:
            raise ValueError("disc_head_step: params must be flat and loss one element")
        if Cx != 256 or params.numel() != self.DISC_HEAD_PARAMS:
            raise ValueError(f"disc_head_step: the head is 256 -> 256 -> 1: a 256-channel map and {self.DISC_HEAD_PARAMS} parameters expected")
        if float(target) not in (0.0, 1.0):
            raise ValueError("disc_head_step: the target is 0 or 1")
        if grads is not None:
            _check_tensor(self, grads, "disc_head grads")
            if grads.dim() != 1 or grads.numel() != params.numel():
                raise ValueError("disc_head_step: grads must match params")
        elif accumulate:
            raise ValueError("disc_head_step: accumulate needs grads")
        p, dh = self.empty((B,)), torch.empty_like(h)
        self.check(self.lib.sr_disc_head_step(self.h, h.data_ptr(), B, H, W, 256, 256, 1, params.data_ptr(), float(target), loss.data_ptr(), p.data_ptr(),
                                              dh.data_ptr(), None if grads is None else grads.data_ptr(), int(bool(accumulate)), self.stream()))
        return p, dh

    def softmax_rows_(self, s):
        """softmax over the last axis, in place."""
        _check_tensor(self, s, "softmax input")
        self.check(self.lib.sr_softmax_rows(self.h, s.data_ptr(), s.numel() // s.shape[-1], s.shape[-1], self.stream()))
        return s

    def softmax_bwd(self, p, dp):
        _check_tensor(self, p, "softmax_bwd p")
        _check_tensor(self, dp, "softmax_bwd dp")
        ds = torch.empty_like(p)
        self.check(self.lib.sr_softmax_bwd(self.h, p.data_ptr(), dp.data_ptr(), ds.data_ptr(), p.numel() // p.shape[-1], p.shape[-1], self.stream()))
        return ds

    def _attention_operand(self, t, name, channels, B=None, N=None):
        """q / k / v of the streamed attention: fp32 [B, N, channels], dense or a channel range of a wider [B, N, C] buffer (e.g. one of a fused
        f | g | h tensor) -> its row stride in elements."""
        if not isinstance(t, torch.Tensor) or t.device != self.torch_device or t.dtype != torch.float32:
            raise ValueError(f"{name}: expected a float32 tensor on {self.torch_device}")
        if t.dim() != 3 or t.shape[2] != channels or t.numel() == 0 or (B is not None and tuple(t.shape[:2]) != (B, N)):
            raise ValueError(f"{name}: expected shape [B, N, {channels}]" + ("" if B is None else f" with B = {B}, N = {N}") + f", got {tuple(t.shape)}")
        rs = t.stride(1)
        if t.stride(2) != 1 or rs < channels or (t.shape[0] > 1 and t.stride(0) != t.shape[1] * rs):
            raise ValueError(f"{name}: rows must be unit-stride channel ranges of one [B, N, C] buffer")
        return rs

    def attention_fwd_lse(self, q, k, v):
        """The SelfAttention core o = softmax(q k^T) v (ESRGAN_model.py:57-65; q = g, k = f: [B, N, 8], v = h: [B, N, 32], fp32) by the streaming
        kernel, plus lse [B, N] = log sum_j exp(q_i . k_j), what attention_bwd needs to recompute the softmax: -> (o [B, N, 32], lse).  The operands
        may be channel ranges of one fused buffer."""
        q_rs = self._attention_operand(q, "attention q", 8)
        B, N = q.shape[:2]
        k_rs, v_rs = self._attention_operand(k, "attention k", 8, B, N), self._attention_operand(v, "attention v", 32, B, N)
        o, lse = self.empty((B, N, 32)), self.empty((B, N))
        self.check(self.lib.sr_attention_fwd_lse(self.h, q.data_ptr(), k.data_ptr(), v.data_ptr(), q_rs, k_rs, v_rs, B, N, o.data_ptr(), lse.data_ptr(),
                                                 self.stream()))
        return o, lse

    def attention_bwd(self, q, k, v, o, do, lse):
        """Gradients of attention_fwd_lse's o with respect to q, k, v given do = dL/do, streamed over key / query tiles (no [B, N, N] tensor, no
        atomics: the same bits every run) -> (dq [B, N, 8], dk [B, N, 8], dv [B, N, 32])."""
        q_rs = self._attention_operand(q, "attention q", 8)
        B, N = q.shape[:2]
        k_rs, v_rs = self._attention_operand(k, "attention k", 8, B, N), self._attention_operand(v, "attention v", 32, B, N)
        for t, name, shape in ((o, "attention o", (B, N, 32)), (do, "attention do", (B, N, 32)), (lse, "attention lse", (B, N))):
            _check_tensor(self, t, name)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        dq, dk, dv = self.empty((B, N, 8)), self.empty((B, N, 8)), self.empty((B, N, 32))
        self.check(self.lib.sr_attention_bwd(self.h, q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), q_rs, k_rs,
                                             v_rs, B, N, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), self.stream()))
        return dq, dk, dv

    def maxpool2_bwd(self, x, dy):
        _check_tensor(self, x, "maxpool_bwd x")
        _check_tensor(self, dy, "maxpool_bwd dy")
        B, H, W, Cx = x.shape
        dx = torch.empty_like(x)
        self.check(self.lib.sr_maxpool2_bwd(self.h, x.data_ptr(), dy.data_ptr(), B, H, W, Cx, dx.data_ptr(), self.stream()))
        return dx

    def zero_insert2(self, dy, H, W):
        """Adjoint of SP_PICK2: dy [B,ceil(H/2),ceil(W/2),C] -> [B,H,W,C]."""
        _check_tensor(self, dy, "zero_insert dy")
        B, _, _, Cx = dy.shape
        out = self.empty((B, H, W, Cx), torch.float32)
        self.check(self.lib.sr_zero_insert2(self.h, dy.data_ptr(), B, int(H), int(W), Cx, out.data_ptr(), self.stream()))
        return out

    def spectral_l1_bwd(self, a, b, scale=1.0):
        _check_tensor(self, a, "spectral_bwd a")
        _check_tensor(self, b, "spectral_bwd b")
        B, H, W, Cx = a.shape
        da = torch.empty_like(a)
        self.check(self.lib.sr_spectral_l1_bwd(self.h, a.data_ptr(), b.data_ptr(), B, H, W, Cx, float(scale), da.data_ptr(), self.stream()))
        return da

    def l1(self, a, b):
        """mean |a - b| (ESRGAN _pixel_loss) -> [1] tensor."""
        _check_tensor(self, a, "l1 input a")
        _check_tensor(self, b, "l1 input b")
        if a.shape != b.shape:
            raise ValueError("l1 inputs must have the same shape")
        out = self.empty((1,), torch.float32)
        self.check(self.lib.sr_l1(self.h, a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), self.stream()))
        return out

    def spectral_l1(self, a, b):
        """mean | |fft2(a)| - |fft2(b)| | over the (W, C) axes of [B,H,W,3] tensors (ESRGAN _spectral_loss) -> [1] tensor."""
        _check_tensor(self, a, "spectral input a")
        _check_tensor(self, b, "spectral input b")
        if a.shape != b.shape or a.dim() != 4:
            raise ValueError("spectral loss inputs must be two [B,H,W,3] tensors of the same shape")
        B, H, W, Cx = a.shape
        out = self.empty((1,), torch.float32)
        self.check(self.lib.sr_spectral_l1(self.h, a.data_ptr(), b.data_ptr(), B, H, W, Cx, out.data_ptr(), self.stream()))
        return out

    def num_patches(self, H, W, C_, patch, stride):
        n = C.c_int()
        self.check(self.lib.sr_extract_patches(self.h, None, H, W, C_, patch, stride, 1.0, 0.0, L.DTYPE_F32, None, 0, C.byref(n), None))
        return n.value

    def extract_patches(self, img, patch, stride, mul=1.0, add=0.0, out_dtype=torch.float32):
        _check_tensor(self, img, "extract_patches image")
        H, W, Cx = img.shape
        n = self.num_patches(H, W, Cx, patch, stride)
        out = self.empty((n, patch, patch, Cx), out_dtype)
        cnt = C.c_int()
        self.check(self.lib.sr_extract_patches(self.h, img.data_ptr(), H, W, Cx, patch, stride, float(mul), float(add),
                                               dtype_code(out_dtype), out.data_ptr(), out.numel(), C.byref(cnt), self.stream()))
        return out

    def extract_patches_batch(self, imgs, patch, stride, mul=1.0, add=0.0, out_dtype=torch.float32):
        """extract_patches for a stack: imgs [F,H,W,C] fp32 or uint8 (the value float(u8)) -> [F*P,patch,patch,C], frame-major, one launch.
        Frame f's slice is bit for bit extract_patches(imgs[f].float(), ...)."""
        _check_tensor(self, imgs, "extract_patches_batch images", (torch.float32, torch.uint8))
        if imgs.dim() != 4:
            raise ValueError("extract_patches_batch images: expected [F,H,W,C]")
        F, H, W, Cx = imgs.shape
        if F == 0:
            raise ValueError("extract_patches_batch images: empty stack")
        n = C.c_int()
        args = (self.h, imgs.data_ptr(), dtype_code(imgs.dtype), F, H, W, Cx, int(patch), int(stride), float(mul), float(add), dtype_code(out_dtype))
        self.check(self.lib.sr_extract_patches_batch(*args, None, 0, C.byref(n), None))
        out = self.empty((F * n.value, patch, patch, Cx), out_dtype)
        self.check(self.lib.sr_extract_patches_batch(*args, out.data_ptr(), out.numel(), C.byref(n), self.stream()))
        return out

    def patch_vote(self, probs, F, P, raw=False):
        """The majority vote of VGG16_model.py:252-268 for F frames of P patches: probs [F*P,K] device tensor (1 <= K <= 64) ->
        (classes [F], confidences [F], votes [F,K]).  raw=True: the int32 / fp32 / int32 device tensors, nothing is read; otherwise NumPy
        int64 / float64 / int64 (one synchronising read each).  The confidence is the winner's fp64 mean rounded once to fp32."""
        _check_tensor(self, probs, "patch_vote probs", (torch.float32, torch.bfloat16))
        if probs.dtype != torch.float32:
            probs = probs.float()
        F, P = int(F), int(P)
        if probs.dim() != 2 or F < 1 or P < 1 or probs.shape[0] != F * P:
            raise ValueError("patch_vote probs: expected [F*P,K] with F, P >= 1")
        K = int(probs.shape[1])
        cls, conf, votes = self.empty((F,), torch.int32), self.empty((F,), torch.float32), self.empty((F, max(K, 1)), torch.int32)
        self.check(self.lib.sr_patch_vote(self.h, probs.data_ptr(), F, P, K, cls.data_ptr(), conf.data_ptr(), votes.data_ptr(), self.stream()))
        if raw:
            return cls, conf, votes
        return cls.cpu().numpy().astype(np.int64), conf.cpu().numpy().astype(np.float64), votes.cpu().numpy().astype(np.int64)

    def _labels(self, a, name, num_classes):
        """int32 device labels; labels the host supplies are checked against [0, num_classes) here, device labels are taken as they are."""
        if isinstance(a, torch.Tensor) and a.device == self.torch_device:
            return _check_tensor(self, a if a.dtype == torch.int32 else a.to(torch.int32), name, (torch.int32,))
        h = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
        if h.size and (h.min() < 0 or h.max() >= num_classes):
            raise ValueError(f"{name}: labels must lie in [0, {num_classes})")
        return self.to_device(h.astype(np.int32))

    def classification_counts(self, y_true, preds, conf=None, num_classes=None):
        """y_true [N], preds [A,N] (and conf [A,N]) -> (confusion int64 [A,K,K], rows = true class; conf_sums float64 [A,2] = sum of conf, sum
        of conf over the correct predictions), both device tensors (nothing is read here: sr355.study gathers them with the labels into one read).  Host arrays are validated against [0,K) and uploaded; device tensors (as sr_patch_vote writes them) are
        used in place.  num_classes may be omitted only when y_true and preds are host arrays (1 + their largest label)."""
        on_dev = lambda t: isinstance(t, torch.Tensor) and t.device == self.torch_device
        if num_classes is None:
            if on_dev(y_true) or on_dev(preds):
                raise ValueError("classification_counts: num_classes is required with device labels (finding it would need a read)")
            num_classes = 1 + max(int(np.max(np.asarray(y_true), initial=0)), int(np.max(np.asarray(preds), initial=0)))
        K = int(num_classes)
        y = self._labels(y_true, "classification_counts y_true", K).reshape(-1)
        p = self._labels(preds, "classification_counts preds", K)
        p = p.reshape(1, -1) if p.dim() == 1 else p
        A, N = int(p.shape[0]), int(y.shape[0])
        if p.dim() != 2 or p.shape[1] != N or A < 1 or N < 1 or K < 1:
            raise ValueError("classification_counts: y_true [N] and preds [A,N] with A, N, K >= 1")
        cf = None
        if conf is not None:
            cf = conf if on_dev(conf) else self.to_device(np.asarray(conf.cpu() if isinstance(conf, torch.Tensor) else conf, np.float32))
            cf = _check_tensor(self, cf.reshape(p.shape) if cf.numel() == p.numel() else cf, "classification_counts conf")
            if cf.shape != p.shape:
                raise ValueError("classification_counts: conf must have the shape of preds")
        words = self.empty((A * K * K + 2 * A,), torch.int64)
        cm, sums = words[:A * K * K].view(A, K, K), words[A * K * K:].view(torch.float64).view(A, 2)
        self.check(self.lib.sr_classification_counts(self.h, y.data_ptr(), p.data_ptr(), None if cf is None else cf.data_ptr(), A, N, K,
                                                     cm.data_ptr(), sums.data_ptr(), self.stream()))
        return cm, sums

    def overlap_add(self, patches, H, W, patch, stride, scale=1, mul=1.0, add=0.0):
        _check_tensor(self, patches, "overlap_add patches", (torch.float32, torch.bfloat16))
        Cx = patches.shape[-1]
        out = self.empty((H * scale, W * scale, Cx), torch.float32)
        self.check(self.lib.sr_overlap_add(self.h, patches.data_ptr(), dtype_code(patches.dtype), H, W, Cx, patch, stride, scale,
                                           float(mul), float(add), out.data_ptr(), self.stream()))
        return out


class Model:
    """sr_model wrapper: build from the reference's setup_model() hyper-parameters, load Keras-named
    weights, run forward on device tensors."""
    KINDS = {"srcnn": L.MODEL_SRCNN, "edsr": L.MODEL_EDSR, "esrgan_g": L.MODEL_ESRGAN_G, "vgg16": L.MODEL_VGG16,
             "esrgan_d": L.MODEL_ESRGAN_D, "vgg19_features": L.MODEL_VGG19_FEATURES}

    def __init__(self, kind, compute_dtype="f32", scale_factor=1, channels=3, num_blocks=0, num_filters=64,
                 growth_channels=32, res_scaling=0.1, num_classes=2, use_attention=True, ctx=None, dense_block_stream=0):
        self.ctx = ctx or Context.get()
        self.kind = kind
        self.dense_block_stream = int(dense_block_stream)
        self.compute_dtype = _DT2TORCH[dtype_code(compute_dtype)]
        cfg = L.ModelCfg(dtype_code(compute_dtype), int(scale_factor), int(channels), int(num_blocks), int(num_filters),
                         int(growth_channels), float(res_scaling), int(num_classes), int(bool(use_attention)))
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.sr_model_create(self.ctx.h, self.KINDS[kind], C.byref(cfg), C.byref(h)))
        self.h = h
        self.finalized = False

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.ctx.lib.sr_model_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def param_specs(self):
        """[(keras_layer_name, 'kernel'|'bias', shape)] in graph order."""
        lib = self.ctx.lib
        out = []
        for i in range(lib.sr_model_num_params(self.h)):
            name, which, nd = C.c_char_p(), C.c_int(), C.c_int()
            shape = (C.c_int64 * 4)()
            self.ctx.check(lib.sr_model_param_info(self.h, i, C.byref(name), C.byref(which), shape, C.byref(nd)))
            out.append((name.value.decode(), "bias" if which.value else "kernel", tuple(shape[:nd.value])))
        return out

    def layer_shapes(self):
        """[(layer_name, kernel_shape)] -- one entry per Keras layer."""
        return [(n, s) for n, w, s in self.param_specs() if w == "kernel"]

    def count_params(self):
        return int(sum(int(np.prod(s)) for _, _, s in self.param_specs()))

    def set_weights(self, weights):
        """weights: {layer_name: (kernel, bias)} (conv HWIO, dense [in,out]).  Missing layers -> KeyError."""
        lib = self.ctx.lib
        for name, kshape in self.layer_shapes():
            if name not in weights:
                raise KeyError(f"weights for layer '{name}' missing")
            k, b = weights[name]
            for which, arr in ((L.WEIGHT_KERNEL, k), (L.WEIGHT_BIAS, b)):
                a = _np32(arr)
                shp = (C.c_int64 * a.ndim)(*a.shape)
                self.ctx.check(lib.sr_model_set_weight(self.h, name.encode(), which, _fptr(a), shp, a.ndim))
        self.ctx.check(lib.sr_model_finalize(self.h))
        self.finalized = True
        if self.dense_block_stream:
            self.set_dense_block_stream(self.dense_block_stream)

    def set_dense_block_stream(self, mode):
        """When forwards of this bf16 ESRGAN generator of 8 growth channels run a dense block as the streamed kernel dense_block_stream<bf16,g8>: 0 never (the
        default), 1 where the LDS-resident kernel does not fit and the row ring does (48 x 48 patches), 2 wherever the ring fits (diagnostic).  ValueError for
        any other model (sr_model_set_dense_block_stream)."""
        self.ctx.check(self.ctx.lib.sr_model_set_dense_block_stream(self.h, int(mode)))
        self.dense_block_stream = int(mode)

    def output_shape(self, B, H, W, Cx):
        s = (C.c_int64 * 4)()
        self.ctx.check(self.ctx.lib.sr_model_output_shape(self.h, B, H, W, Cx, s))
        return tuple(s) if self.kind not in ("vgg16", "esrgan_d") else (s[0], s[1])

    def forward(self, x, out=None):
        """x [B,H,W,C] device tensor (f32, or bf16 for a bf16 model) -> output tensor of the same dtype."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError("expected a [B,H,W,C] tensor")
        x = x.contiguous()
        _check_tensor(self.ctx, x, "forward input", (torch.float32, torch.bfloat16))
        B, H, W, Cx = x.shape
        oshape = self.output_shape(B, H, W, Cx)
        if out is not None:
            _check_tensor(self.ctx, out, "forward out=", (x.dtype,))
            if tuple(out.shape) != tuple(oshape):
                raise ValueError(f"forward out= has shape {tuple(out.shape)}, the model produces {tuple(oshape)}")
        y = out if out is not None else self.ctx.empty(oshape, x.dtype)
        self.ctx.check(self.ctx.lib.sr_forward(self.h, x.data_ptr(), dtype_code(x.dtype), B, H, W, Cx, y.data_ptr(), y.numel(),
                                               self.ctx.stream()))
        return y

    # ------------------------------------------------------------------ workspaces / diagnostics
    def release_workspace(self):
        """Free the activation workspaces (grow-only otherwise); weights stay loaded."""
        self.ctx.check(self.ctx.lib.sr_model_release_workspace(self.h))

    def ops(self):
        """[(name, channels, mul, shift, ceil_halvings)] per graph op: Keras layer name of a conv, else the op kind; the op's output is
        [B, h, w, channels] with h = (H*mul)>>shift, then ceil-halved ceil_halvings times (channels 0: no activation output)."""
        lib, out = self.ctx.lib, []
        for i in range(lib.sr_model_num_ops(self.h)):
            name, ch, mul, sh, cs = C.c_char_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
            self.ctx.check(lib.sr_model_op_info(self.h, i, C.byref(name), C.byref(ch), C.byref(mul), C.byref(sh), C.byref(cs)))
            out.append((name.value.decode(), ch.value, mul.value, sh.value, cs.value))
        return out

    @staticmethod
    def _op_hw(op, H, W):
        h, w = (H * op[2]) >> op[3], (W * op[2]) >> op[3]
        for _ in range(op[4]):
            h, w = (h + 1) // 2, (w + 1) // 2
        return h, w

    def forward_with_taps(self, x, names):
        """Diagnostic forward: -> (y, {name: fp32 NHWC tensor}) with the output of the LAST op called `name` for every name
        (stage-by-stage parity traces; the taps are removed again before returning)."""
        ops = self.ops()
        B, H, W, _ = x.shape
        taps, idx = {}, {}
        for n in names:
            hits = [i for i, o in enumerate(ops) if o[0] == n and o[1] > 0]
            if not hits:
                raise KeyError(f"no op named '{n}' with an activation output")
            idx[n] = hits[-1]
        try:
            for n, i in idx.items():
                th, tw = self._op_hw(ops[i], H, W)
                t = self.ctx.empty((B, th, tw, ops[i][1]), torch.float32)
                self.ctx.check(self.ctx.lib.sr_model_set_tap(self.h, i, t.data_ptr(), t.numel()))
                taps[n] = t
            y = self.forward(x)
        finally:
            for i in idx.values():
                self.ctx.lib.sr_model_set_tap(self.h, i, None, 0)
        return y, taps

    def predict(self, x, batch_size=32):
        """keras Model.predict(x, batch_size): forward in chunks, outputs concatenated.  Accepts NumPy
        (returns NumPy, as Keras does) or a device tensor (returns a device tensor)."""
        is_np = not isinstance(x, torch.Tensor)
        xt = self.ctx.to_device(x, torch.float32) if is_np else x
        n = xt.shape[0]
        oshape = self.output_shape(n, *xt.shape[1:])
        y = self.ctx.empty(oshape, xt.dtype)
        for i in range(0, n, max(1, int(batch_size))):
            self.forward(xt[i:i + batch_size], out=y[i:i + batch_size])
        if is_np:
            return y.float().cpu().numpy()
        return y
