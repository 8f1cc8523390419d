"""Thin tensor-level wrappers over the C ABI: weight packing, forward, simulator and metrics.

All compute runs in libraman_mi355x.so on the caller's current HIP stream; these functions only
check shapes/devices, allocate outputs through the PyTorch caching allocator and pass raw
pointers.  Nothing here has a CPU or PyTorch-op fallback.

Every call enqueues on ``torch.cuda.current_stream(x.device)`` -- the stream of the device that holds the
tensors, whichever device is current -- and returns without waiting.  The calls that wait on the host are the
ones that read a status word back: ``check=True`` of forward() / forward_metrics(), Workspace.check() and
Workspace.read_status().  A filter given host taps copies them to the device first, which also waits.
(tests/test_launch_contract_gpu.py)
"""
import ctypes
import math
import os
import statistics

import torch

from . import _lib

ARCHS = ("DenoiseCNN", "RRCDNet", "DSDN", "ADSDN", "PIDN", "APIDN")
ARCH_ID = {a: i for i, a in enumerate(ARCHS)}
CBAM_ARCHS = ("ADSDN", "APIDN")
CBAM_IDS = tuple(ARCH_ID[a] for a in CBAM_ARCHS)
# dtypes whose e4m3 correction planes bound the activations (|v| <= 1792): their forwards report a
# saturated tile through the workspace's status word (RangeError) and write NaN for it
RANGE_CODES = (3, 5)
# a fused network's 16-bit forward keeps a status word in its workspace (common.hpp STATUS_*): bit 0 an
# e4m3 activation saturated (RANGE_CODES only), bit 1 an input left [-4, 4] (the stems' input gate,
# models.INPUT_GATE: the 16-bit modes' domain; informational, rdn_forward_status does not fail on it)
STATUS_RANGE, STATUS_GATE, STATUS_TIMEOUT = 1, 2, 4
# Engine arithmetic modes (include/raman_mi355x.h rdn_dtype).  Every name here except
# "bf16-unsafe" meets its north-star tolerance on every golden fixture (fp32: 1e-5 max-relative;
# 16-bit modes: 2e-2 max-abs).  Single-rounding bf16 does NOT (0.24 on trained RRCDNet),
# so it is reachable only under that explicit name; plain "bf16" / torch.bfloat16 is refused with a
# pointer to the tolerance-meeting 16-bit modes instead of silently returning out-of-contract results.
DTYPE_ID = {"fp32": 0, "float32": 0, "bf16-unsafe": 1, "bf16_unsafe": 1, "bf16x3": 2, "f16f8": 3, "f16-plain": 4,
            "f16mix": 5}
DTYPE_NAME = {0: "fp32", 1: "bf16-unsafe", 2: "bf16x3", 3: "f16f8", 4: "f16-plain", 5: "f16mix"}
SAFE_16BIT = ("f16", "f16f8", "bf16x3")
F16, F16MIX = 4, 5
# every spelling of "f16" means one thing: the fastest arithmetic within the 2e-2 bar for the network
_F16_SPELLINGS = ("f16", "float16", "half")


def default_correction_mask(arch):
    """The layers RDN_F16MIX corrects for ``arch`` (0: plain f16 already meets the 2e-2 bar there)."""
    m = ctypes.c_uint64()
    _lib.check(_lib.lib().rdn_default_correction_mask(_arch(arch), ctypes.byref(m)), "rdn_default_correction_mask")
    return m.value


def correction_mask(arch, dtype, host_blob):
    """Correction mask recorded in a packed (host) blob."""
    m = ctypes.c_uint64()
    _lib.check(_lib.lib().rdn_get_correction_mask(_arch(arch), resolve_dtype(arch, dtype),
                                                  ctypes.c_void_p(host_blob.data_ptr()), host_blob.numel(),
                                                  ctypes.byref(m)), "rdn_get_correction_mask")
    return m.value


def check_blob(arch, dtype, host_blob):
    """Raise unless ``host_blob`` (a CPU uint8 tensor) was packed by rdn_pack for (arch, dtype)."""
    _lib.check(_lib.lib().rdn_check_blob(_arch(arch), resolve_dtype(arch, dtype), ctypes.c_void_p(host_blob.data_ptr()),
                                         host_blob.numel()), "rdn_check_blob")


def resolve_dtype(arch, dtype):
    """ABI dtype code (rdn_dtype) for a user dtype.  'f16' (also 'float16' and torch.float16) is the
    fastest arithmetic within the 2e-2 bar: plain f16 (RDN_F16) where that suffices, f16 with the
    compiled-in e4m3-corrected layers (RDN_F16MIX) where it does not (RRCDNet).  'f16-plain' forces
    RDN_F16 everywhere, 'f16mix' RDN_F16MIX.  An integer is taken as an ABI code unchanged."""
    if isinstance(dtype, int) and not isinstance(dtype, bool):
        if dtype not in DTYPE_NAME:
            raise ValueError(f"unknown engine dtype code {dtype}")
        return dtype
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}.get(dtype, str(dtype))
    if dtype in _F16_SPELLINGS:
        return F16MIX if default_correction_mask(arch) else F16
    return _dtype(dtype)


def dtype_name(dtype, arch=None):
    """User-level name of a dtype: 'f16' for every f16 spelling (the network's fastest mode within
    2e-2), else the name of its ABI code ('f16-plain' = RDN_F16, 'f16mix' = RDN_F16MIX)."""
    if isinstance(dtype, torch.dtype) and dtype == torch.float16:
        return "f16"
    if isinstance(dtype, str) and dtype in _F16_SPELLINGS:
        return "f16"
    return DTYPE_NAME[resolve_dtype(arch, dtype) if arch is not None else _dtype(dtype)]


def _arch(arch):
    if isinstance(arch, int):
        return arch
    try:
        return ARCH_ID[arch]
    except KeyError:
        raise ValueError(f"unknown network {arch!r}; expected one of {ARCHS}") from None


def _dtype(dtype):
    """Code of an arch-independent dtype name ('f16' depends on the network: resolve_dtype)."""
    if isinstance(dtype, int) and dtype in DTYPE_NAME:
        return dtype
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "f16"}.get(dtype, str(dtype))
    if dtype in _F16_SPELLINGS:
        raise ValueError("engine dtype 'f16' resolves per network: use resolve_dtype(arch, 'f16')")
    if dtype in ("bf16", "bfloat16"):
        raise ValueError("engine dtype 'bf16' (one bf16 rounding per operand) does not meet the 2e-2 bf16 "
                         "tolerance on trained weights (0.24 on trained RRCDNet); use 'f16', 'f16f8' or 'bf16x3' "
                         f"({', '.join(SAFE_16BIT)}: within 2e-2), or opt in explicitly with 'bf16-unsafe'")
    try:
        return DTYPE_ID[dtype]
    except (KeyError, TypeError):
        raise ValueError(f"unknown engine dtype {dtype!r}; expected one of 'fp32', 'f16', 'f16-plain', 'f16f8', "
                         "'bf16x3', 'bf16-unsafe'") from None


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def param_names(arch):
    """The state_dict keys the packer consumes, in order (folded BN stats included)."""
    L = _lib.lib()
    need = ctypes.c_size_t()
    _lib.check(L.rdn_param_names(_arch(arch), None, 0, ctypes.byref(need)), "rdn_param_names")
    buf = ctypes.create_string_buffer(need.value)
    _lib.check(L.rdn_param_names(_arch(arch), buf, need.value, ctypes.byref(need)), "rdn_param_names")
    return [s for s in buf.value.decode().split("\n") if s]


def packed_size(arch, dtype):
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().rdn_packed_size(_arch(arch), resolve_dtype(arch, dtype), ctypes.byref(n)), "rdn_packed_size")
    return n.value


def pack(arch, state_dict, dtype, device):
    """Fold BN + lay out MFMA fragments on the host, then copy the blob to ``device``."""
    names = param_names(arch)
    missing = [k for k in names if k not in state_dict]
    if missing:
        raise KeyError(f"state_dict lacks {len(missing)} tensors the engine needs, e.g. {missing[:3]}")
    host = [state_dict[k].detach().to("cpu", torch.float32).contiguous() for k in names]
    ptrs = (ctypes.c_void_p * len(host))(*[t.data_ptr() for t in host])
    numels = (ctypes.c_int64 * len(host))(*[t.numel() for t in host])
    code = resolve_dtype(arch, dtype)
    size = packed_size(arch, code)
    blob = torch.empty(size, dtype=torch.uint8)
    _lib.check(_lib.lib().rdn_pack(_arch(arch), code, ptrs, numels, len(host),
                                   ctypes.c_void_p(blob.data_ptr()), size), "rdn_pack")
    return blob.to(device)


def _check_cuda_f32(t, name):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"raman_mi355x runs on the GPU only: {name} must be a CUDA (HIP) tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")


def _check_clean(clean):
    """The clean reference of the meters: a CUDA tensor, float32 (the device simulator) or float64."""
    if not (torch.is_tensor(clean) and clean.is_cuda):
        raise RuntimeError("raman_mi355x runs on the GPU only: clean must be a CUDA (HIP) tensor")
    if clean.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"clean must be float32 or float64, got {clean.dtype}")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _rows(t):
    """(N, L) or (N, 1, L) -> contiguous (N, L) (N = 0 included: no -1 in the shape)."""
    return t.reshape(t.shape[0], t.shape[-1] if t.dim() > 1 else 1).contiguous()


def _check_out(t, name, shape, device, dtype=torch.float32):
    """A caller-supplied output buffer the kernels write through a raw pointer: it must be exactly
    the size, type and device the launch assumes, and contiguous."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda or t.device != torch.device(device):
        raise ValueError(f"{name} must live on {device}, got {t.device}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _no_overlap(a, b, what):
    """ValueError(``what``) if the bytes of tensors ``a`` and ``b`` overlap (the kernels take raw pointers)."""
    if (a.data_ptr() < b.data_ptr() + b.numel() * b.element_size()
            and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()):
        raise ValueError(what)


def _check_rows_input(x):
    """x as the filters take it: a float32 CUDA tensor, (N, L) or (N, 1, L), contiguous."""
    _check_cuda_f32(x, "input")
    if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
        raise ValueError(f"expected (N, L) or (N, 1, L) input, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("input must be contiguous")


def _out_like(x, out):
    """The output of a launch that reads x: ``out``, checked to be x's shape and apart from it, or a new tensor."""
    if out is None:
        return torch.empty_like(x)
    _check_out(out, "out", x.shape, x.device)
    _no_overlap(out, x, "out must not overlap the input (tiles re-read input halos while outputs are written)")
    return out


def needs_workspace(arch, code):
    """A forward of (arch, code) takes a workspace: the CBAM team kernels (required) and the fused
    networks' 16-bit dtypes (their status word: range and input gate)."""
    return _arch(arch) in CBAM_IDS or code != 0


def has_status_word(arch, code):
    """Whether a workspace of (arch, code) starts with the fused networks' status word."""
    return _arch(arch) not in CBAM_IDS and code != 0


class Workspace:
    """Device scratch of a forward for (arch, dtype, L) on one device and stream, reused across
    forwards: the CBAM team kernels' slots and hand-off error word, and the fused networks' 16-bit status
    word (the range bit of RDN_F16F8 / RDN_F16MIX, the input-gate bit).  The status words are sticky: ``check()`` waits for the stream once and raises
    EngineError if any forward since the last check timed out, RangeError if one saturated the e4m3
    planes (rdn_forward_status), so a batched driver checks once at the end instead of host-syncing
    every batch."""

    def __init__(self, arch, dtype, n, L, device, stream=None):
        self.arch, self.code, self.L = _arch(arch), resolve_dtype(arch, dtype), int(L)
        self.device = torch.device(device)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.n = int(n)
        sz = ctypes.c_size_t()
        lib_ = _lib.lib()
        sp = ctypes.c_void_p(self.stream.cuda_stream)
        _lib.check(lib_.rdn_workspace_size(self.arch, self.code, self.n, self.L, ctypes.byref(sz), sp),
                   "rdn_workspace_size")
        self.bytes = sz.value
        self._fit_memo = {}
        self.buf = torch.empty(self.bytes, dtype=torch.uint8, device=self.device) if self.bytes else None
        _lib.check(lib_.rdn_workspace_init(self.arch, self.code, self.n, self.L, self.ptr, self.bytes, sp),
                   "rdn_workspace_init")

    @property
    def ptr(self):
        return _ptr(self.buf)

    def fits(self, arch, code, n, L, device):
        """Made for this network, dtype, length and device, large enough for n spectra, and bound to the
        stream the forward launches on (torch's current stream): check() waits for self.stream only, and
        rdn_workspace_init's reset is ordered on it."""
        if not ((self.arch, self.code, self.L, self.device) == (_arch(arch), code, int(L), torch.device(device))
                and torch.cuda.current_stream(self.device).cuda_stream == self.stream.cuda_stream):
            return False
        if self.arch in CBAM_IDS:
            # the CBAM layout (team or segment geometry) is the one the device and environment give now:
            # the size it had when made, and room for n spectra (memoised per batch size and the
            # RDN_CBAM_SEGMENTS switch: the batch-1 loop asks once per call)
            key = (int(n), os.environ.get("RDN_CBAM_SEGMENTS"))
            ok = self._fit_memo.get(key)
            if ok is None:
                ok = self.bytes_for(self.n) == self.bytes and self.bytes_for(n) <= self.bytes
                self._fit_memo[key] = ok
            return ok
        return self.n >= n or self.bytes_for(n) <= self.bytes

    def bytes_for(self, n):
        sz = ctypes.c_size_t()
        _lib.check(_lib.lib().rdn_workspace_size(self.arch, self.code, int(n), self.L, ctypes.byref(sz),
                                                 ctypes.c_void_p(self.stream.cuda_stream)), "rdn_workspace_size")
        return sz.value

    def status_word(self):
        """The status word of a fused network's 16-bit workspace (its first 4 bytes, rdn_forward_status's
        word: STATUS_RANGE | STATUS_GATE bits) as a device int32 tensor, without waiting.  A caller that
        reads it this way (models._EngineNet.forward: the call's one 4-byte host read) clears it with
        clear_status_word() (rdn_forward_status reads and clears)."""
        if not has_status_word(self.arch, self.code):
            raise ValueError("status_word: only the fused networks' 16-bit workspaces")
        return self.buf[:4].view(torch.int32)

    def clear_status_word(self):
        self.buf[:4].zero_()                       # on the current stream = the forwards' (fits())

    def read_status(self):
        """Wait for the workspace's stream and return its status word (0 for a CBAM workspace) without
        clearing it (check() clears it)."""
        if not has_status_word(self.arch, self.code):
            return 0
        with torch.cuda.stream(self.stream):
            return int(self.status_word().item())

    def check(self):
        """Wait for the stream, read and clear the status words of every forward since the last check, and
        return their flags (STATUS_RANGE | STATUS_GATE | STATUS_TIMEOUT, rdn_forward_status_ex).  Raises
        EngineError if a CBAM hand-off timed out, RangeError if a tile saturated the e4m3 planes; the
        input gate (an input beyond the 16-bit modes' domain) is only reported in the flags."""
        flags = ctypes.c_uint(0)
        _lib.check(_lib.lib().rdn_forward_status_ex(self.arch, self.code, self.n, self.L, self.ptr, self.bytes,
                                                    ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(flags)),
                   "rdn_forward_status_ex")
        return int(flags.value)


def _forward_args(arch, dtype, x, out, check, workspace, _ws_checked):
    """Shared argument checks of forward / forward_metrics: (n, L, arch id, code, y, workspace)."""
    _check_cuda_f32(x, "input")
    if x.dim() == 3 and x.shape[1] != 1:
        raise ValueError(f"expected (N, 1, L) input, got {tuple(x.shape)}")
    if x.dim() not in (2, 3):
        raise ValueError(f"expected (N, 1, L) input, got {tuple(x.shape)}")
    n, L = x.shape[0], x.shape[-1]
    a, code = _arch(arch), resolve_dtype(arch, dtype)
    y = _out_like(x, out)
    ws = workspace
    if ws is None and (a in CBAM_IDS or (check and code in RANGE_CODES)):
        ws = Workspace(a, code, n, L, x.device)
    elif ws is not None and not _ws_checked and not ws.fits(a, code, n, L, x.device):
        raise ValueError("workspace was made for another network, dtype, length, device, stream or a smaller batch")
    return n, L, a, code, y, ws


def forward(arch, dtype, packed, x, out=None, check=True, workspace=None, _ws_checked=False):
    """y = Model(x) for x float32 (N, 1, L) (or (N, L)) on the GPU.

    ``dtype`` is an engine dtype name or ABI code (resolve_dtype).  The CBAM networks run one
    team-persistent kernel whose workgroups hand off statistics; RDN_F16F8 / RDN_F16MIX tiles whose
    activations leave the e4m3 planes' range write NaN.  With ``check`` (default) the call waits for
    the kernel and raises EngineError if a hand-off timed out, RangeError if a tile saturated
    (rdn_forward_status).  A batched caller passes one ``Workspace`` to every forward with
    ``check=False`` and calls ``workspace.check()`` once at the end (the status words are sticky);
    (``_ws_checked``: the caller has just verified ``workspace.fits`` for this input.)
    ``check=False`` without a workspace keeps the launch asynchronous and unchecked (benchmarks: the
    affected outputs are NaN).  On the CBAM networks (ADSDN / APIDN) a saturated tile's clamped CBAM
    statistics reach the other tiles of its spectrum through the team hand-off, so the whole spectrum
    is NaN, not just the tile: the team kernel's saturated tile publishes +inf maxima that taint its
    team (cbam.hip publish_stats / apply_cbam), and a segment-path launch (spectra longer than the
    co-resident teams hold) NaNs every spectrum of the chunk.  On the walk geometry (large 'f16' batches
    of RRCDNet) a saturated tile NaNs the rest of its spectrum, since its clamped values reach the next
    tiles through the carried rows.  The status word (RangeError from ``check`` or
    ``Workspace.check()``) remains the authoritative signal."""
    _check_cuda_f32(x, "input")
    x = x.contiguous()
    n, L, a, code, y, ws = _forward_args(arch, dtype, x, out, check, workspace, _ws_checked)
    _lib.check(_lib.lib().rdn_forward(a, code, _ptr(packed), _ptr(x), _ptr(y), n, L,
                                      ws.ptr if ws is not None else _ptr(None), ws.bytes if ws is not None else 0,
                                      _stream(x.device)), "rdn_forward")
    if check and ws is not None:
        ws.check()
    return y


def forward_metrics(arch, dtype, packed, x, clean, out=None, sums=None, per_spectrum=False, acc=None, check=True,
                    workspace=None):
    """forward() and metrics() in one call (rdn_forward_metrics): y = Model(x), then each spectrum's MSE,
    SSIM, Smoothness and Peak2Peak against ``clean`` (float32 or float64, (N, L) or (N, 1, L)), added to
    ``sums`` / ``acc`` as metrics() does.  On the walk geometry (large batches of the f16 modes) the
    forward kernel computes the metrics itself after each spectrum's walk, so y is not read again by a
    second pass.  Returns (y, per (n, 4) or None, sums, fused)."""
    _check_cuda_f32(x, "input")
    x = x.contiguous()
    _check_clean(clean)
    n, L, a, code, y, ws = _forward_args(arch, dtype, x, out, check, workspace, False)
    clean = _rows(clean)
    if tuple(clean.shape) != (n, L):
        raise ValueError(f"clean must be ({n}, {L}), got {tuple(clean.shape)}")
    if clean.device != x.device:
        raise ValueError(f"input on {x.device} but clean on {clean.device}")
    per = torch.empty((n, 4), dtype=torch.float64, device=x.device) if per_spectrum else None
    if sums is None:
        sums = torch.zeros(5, dtype=torch.float64, device=x.device)
    else:
        _check_out(sums, "sums", (5,), x.device, torch.float64)
    if acc is not None:
        _check_out(acc, "acc", (_lib.ACC_WORDS,), x.device, torch.int64)
    fused = ctypes.c_int(0)
    _lib.check(_lib.lib().rdn_forward_metrics(
        a, code, _ptr(packed), _ptr(x), _ptr(y), n, L, _ptr(clean), int(clean.dtype == torch.float64), _ptr(per),
        _ptr(sums), _ptr(acc), ws.ptr if ws is not None else _ptr(None), ws.bytes if ws is not None else 0,
        _stream(x.device), ctypes.byref(fused)), "rdn_forward_metrics")
    if check and ws is not None:
        ws.check()
    return y, per, sums, bool(fused.value)


GEN_SCAN = 256                 # segment lengths the simulator sums per pass, in int32 (generator.hip phase A)
_INT32_MAX = 2 ** 31 - 1


def check_generate_args(n, seed, first_index, signal_length, snr_range, extreme_noise_prob, max_repeat):
    """ValueError for what rdn_generate refuses (include/raman_mi355x.h) and for a seed or index that
    ctypes would wrap into uint64 silently; returns the values as the ABI takes them.  Needs no device."""
    n, seed, first, L, mr = int(n), int(seed), int(first_index), int(signal_length), int(max_repeat)
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    if not 0 <= first < 2 ** 64:
        raise ValueError(f"first_index must be in [0, 2^64), got {first}")
    if first + n > 2 ** 64:
        raise ValueError(f"first_index + n = {first + n} passes 2^64: the 64-bit spectrum index would wrap onto 0")
    if not 1 <= L <= _INT32_MAX:
        raise ValueError(f"signal_length must be in [1, 2^31), got {L}")
    if mr < 1 or L + GEN_SCAN * mr > _INT32_MAX:
        raise ValueError(f"max_repeat must be >= 1 with signal_length + {GEN_SCAN} * max_repeat <= {_INT32_MAX} "
                         f"(at most {(_INT32_MAX - L) // GEN_SCAN} here), got {mr}")
    lo, hi, prob = (ctypes.c_float(float(v)).value for v in (snr_range[0], snr_range[1], extreme_noise_prob))
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"snr_range must be finite in float32 with lo <= hi, got {tuple(snr_range)}")
    if math.isnan(prob):
        raise ValueError("extreme_noise_prob must not be NaN")
    return n, seed, first, L, lo, hi, prob, mr


def generate(n, seed, first_index=0, signal_length=10000, snr_range=(20.0, 37.0), extreme_noise_prob=0.05,
             max_repeat=40, device="cuda", out=None):
    """Device simulator (数据集产生.py:5-64 contract): returns clean, noisy (n, L), snr, noise_std (n,).

    ``seed`` and ``first_index`` are unsigned 64-bit with first_index + n <= 2^64; out-of-range values and
    the parameters rdn_generate refuses raise ValueError before anything touches the device."""
    n, seed, first_index, L, snr_lo, snr_hi, extreme_noise_prob, max_repeat = check_generate_args(
        n, seed, first_index, signal_length, snr_range, extreme_noise_prob, max_repeat)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("raman_mi355x runs on the GPU only: the simulator needs a CUDA device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if out is None:
        clean = torch.empty((n, L), dtype=torch.float32, device=device)
        noisy = torch.empty((n, L), dtype=torch.float32, device=device)
    else:
        clean, noisy = out
        _check_out(clean, "out[0] (clean)", (n, L), device)
        _check_out(noisy, "out[1] (noisy)", (n, L), device)
        if clean.data_ptr() == noisy.data_ptr():
            raise ValueError("clean and noisy output buffers must be distinct")
    snr = torch.empty(n, dtype=torch.float32, device=device)
    nstd = torch.empty(n, dtype=torch.float32, device=device)
    prm = _lib.GenParams(L, snr_lo, snr_hi, extreme_noise_prob, max_repeat)
    _lib.check(_lib.lib().rdn_generate(seed, first_index, n, ctypes.byref(prm),
                                       ctypes.c_void_p(clean.data_ptr()), ctypes.c_void_p(noisy.data_ptr()),
                                       ctypes.c_void_p(snr.data_ptr()), ctypes.c_void_p(nstd.data_ptr()),
                                       _stream(device)), "rdn_generate")
    return clean, noisy, snr, nstd


def metrics(y, clean, sums=None, per_spectrum=True, acc=None):
    """Per-spectrum [MSE, SSIM, Smoothness, Peak2Peak] (fp64, (n, 4)) and accumulated fp64 sums [5].

    ``clean`` may be float32 (the device simulator) or float64 (a test.npz as evaulate.py:61-62 loads
    it; the metrics then see the same float64 clean values as evaulate.py:34-35).  ``acc``: an
    exact accumulator (new_acc) that this batch is added to (rdn_metrics_ex)."""
    _check_cuda_f32(y, "denoised")
    _check_clean(clean)
    y = _rows(y)
    clean = _rows(clean)
    if y.shape != clean.shape:
        raise ValueError(f"shape mismatch {tuple(y.shape)} vs {tuple(clean.shape)}")
    n, L = y.shape
    if clean.device != y.device:
        raise ValueError(f"denoised on {y.device} but clean on {clean.device}")
    per = torch.empty((n, 4), dtype=torch.float64, device=y.device) if per_spectrum else None
    if sums is None:
        sums = torch.zeros(5, dtype=torch.float64, device=y.device)
    else:
        _check_out(sums, "sums", (5,), y.device, torch.float64)   # fp64 atomics into sums[0..4]
    if acc is not None:
        _check_out(acc, "acc", (_lib.ACC_WORDS,), y.device, torch.int64)
    _lib.check(_lib.lib().rdn_metrics_ex(_ptr(y), _ptr(clean), int(clean.dtype == torch.float64), n, L, _ptr(per),
                                         _ptr(sums), _ptr(acc), _stream(y.device)), "rdn_metrics_ex")
    return per, sums


def new_acc(device):
    """A zeroed exact metric accumulator (RDN_ACC_WORDS int64) on ``device``."""
    return torch.zeros(_lib.ACC_WORDS, dtype=torch.int64, device=device)


def acc_value(acc):
    """{ΣMSE, ΣSSIM, ΣSmoothness, ΣPeak2Peak, count} (float64 [5], CPU) of an exact accumulator: each
    sum is the exact total rounded once (rdn_acc_value)."""
    h = acc.detach().to("cpu", torch.int64).contiguous()
    if h.numel() != _lib.ACC_WORDS:
        raise ValueError(f"accumulator must have {_lib.ACC_WORDS} words")
    out = torch.empty(5, dtype=torch.float64)
    _lib.check(_lib.lib().rdn_acc_value(ctypes.cast(h.data_ptr(), ctypes.POINTER(ctypes.c_int64)),
                                        ctypes.cast(out.data_ptr(), ctypes.POINTER(ctypes.c_double))), "rdn_acc_value")
    return out


# ---- binned reports (rdn_snr, rdn_physics; definitions, bin formula and report layouts: include/raman_mi355x.h) ----
REPORT_QUANTITIES = ("MSE", "SSIM", "Smoothness", "Peak2Peak", "SNR_in", "SNR_out", "SNR_gain")
PHYS_QUANTITIES = ("MSE", "Smooth", "Peak", "Noise", "Total", "PeakCount")
PHYS_WEIGHTS = (0.1, 0.05, 0.01)          # PIDN/train.py:112 alpha, beta, gamma


def _bins(bins):
    """(lo, hi, nbins) as rdn_snr takes them: finite fp32 lo < hi, 1 <= nbins <= 64."""
    try:
        lo, hi, nbins = bins
    except (TypeError, ValueError):
        raise ValueError(f"bins must be (lo, hi, nbins), got {bins!r}") from None
    if isinstance(nbins, bool) or int(nbins) != nbins or not 1 <= int(nbins) <= _lib.REPORT_MAX_BINS:
        raise ValueError(f"nbins must be an integer in [1, {_lib.REPORT_MAX_BINS}], got {nbins!r}")
    lo, hi = ctypes.c_float(lo).value, ctypes.c_float(hi).value      # the fp32 edges the kernel bins by
    if not (lo < hi and abs(lo) != float("inf") and abs(hi) != float("inf")):
        raise ValueError(f"bins need finite lo < hi, got ({lo}, {hi})")
    return lo, hi, int(nbins)


def _weights(weights):
    """(alpha, beta, gamma) as rdn_physics takes them: three finite floats."""
    try:
        a, b, g = (float(w) for w in weights)
    except (TypeError, ValueError):
        raise ValueError(f"weights must be (alpha, beta, gamma), got {weights!r}") from None
    if not all(abs(w) < float("inf") for w in (a, b, g)):          # NaN fails the comparison too
        raise ValueError(f"weights must be finite, got {(a, b, g)}")
    return a, b, g


def _new_report(nbins, device, words):
    """A zeroed report of words(nbins) int64 on ``device``."""
    if isinstance(nbins, bool) or int(nbins) != nbins or not 1 <= int(nbins) <= _lib.REPORT_MAX_BINS:
        raise ValueError(f"nbins must be an integer in [1, {_lib.REPORT_MAX_BINS}], got {nbins!r}")
    return torch.zeros(words(int(nbins)), dtype=torch.int64, device=device)


def new_report(nbins, device):
    """A zeroed SNR report (RDN_REPORT_WORDS(nbins) int64: nbins + 2 rows) on ``device``."""
    return _new_report(nbins, device, _lib.report_words)


def new_physics_report(nbins, device):
    """A zeroed PhysicsAwareLoss report (RDN_PHYS_WORDS(nbins) int64: nbins + 2 rows) on ``device``."""
    return _new_report(nbins, device, _lib.phys_words)


def report_bin(key, bins):
    """Report row (0 underflow, 1 .. nbins, nbins + 1 overflow / NaN) of a key: rdn_report_bin, the
    kernel's own fp32 formula evaluated on the host."""
    lo, hi, nbins = _bins(bins)
    row = ctypes.c_int(-1)
    _lib.check(_lib.lib().rdn_report_bin(float(key), lo, hi, nbins, ctypes.byref(row)), "rdn_report_bin")
    return row.value


def _report_value(report, nbins, what, words, values, fn):
    """Doubles of a report (float64 (nbins + 3, values), CPU) through the ABI's ``fn``."""
    nbins = int(nbins)
    if not 1 <= nbins <= _lib.REPORT_MAX_BINS:
        raise ValueError(f"nbins must be in [1, {_lib.REPORT_MAX_BINS}], got {nbins}")
    h = report.detach().to("cpu", torch.int64).contiguous()
    if h.numel() != words(nbins):
        raise ValueError(f"a {what} of {nbins} bins has {words(nbins)} words, got {h.numel()}")
    out = torch.empty((_lib.report_rows(nbins) + 1, values), dtype=torch.float64)
    _lib.check(getattr(_lib.lib(), fn)(ctypes.cast(h.data_ptr(), ctypes.POINTER(ctypes.c_int64)), nbins,
                                       ctypes.cast(out.data_ptr(), ctypes.POINTER(ctypes.c_double))), fn)
    return out


def report_value(report, nbins):
    """Doubles of a report (float64 (nbins + 3, 9), CPU): one row per report row -- underflow, the bins,
    overflow -- then the totals over all of them; columns {count, ΣMSE, ΣSSIM, ΣSmoothness, ΣPeak2Peak,
    ΣSNR_in, ΣSNR_out, ΣSNR_gain, count of spectra whose four metrics were supplied}.  Each sum is the
    exact total rounded once, NaN where a value was out of range (rdn_report_value)."""
    return _report_value(report, nbins, "report", _lib.report_words, _lib.REPORT_VALUES, "rdn_report_value")


def physics_value(report, nbins):
    """Doubles of a PhysicsAwareLoss report (float64 (nbins + 3, 7), CPU): one row per report row --
    underflow, the bins, overflow -- then the totals over all of them; columns {count, ΣMSE, ΣSmooth, ΣPeak,
    ΣNoise, ΣTotal, ΣPeakCount}.  Each sum is the exact total rounded once, NaN where a value was out of
    range (rdn_physics_value)."""
    return _report_value(report, nbins, "physics report", _lib.phys_words, _lib.PHYS_VALUES, "rdn_physics_value")


def _report_args(x, y, clean, short, key, bins, report, words, unbinned, per_spectrum):
    """What snr() and physics() do with their (type-checked) arguments before the launch: x, y, clean as
    (n, L) rows of one shape on one device, and -- with ``bins`` -- the fp32 edges, the report of
    ``words``(nbins) int64 (made when None) and the key.  ``short`` = (least L, its message);
    ``unbinned``: the message if report inputs were given without ``bins``, else None.
    Returns (x, y, clean, n, L, device, lo, hi, nbins, report)."""
    x, y, clean = _rows(x), _rows(y), _rows(clean)
    if x.shape != y.shape or y.shape != clean.shape:
        raise ValueError(f"shape mismatch {tuple(x.shape)} vs {tuple(y.shape)} vs {tuple(clean.shape)}")
    n, L = y.shape
    if L < short[0]:
        raise ValueError(short[1])
    dev = y.device
    if x.device != dev or clean.device != dev:
        raise ValueError(f"denoised on {dev} but input on {x.device} and clean on {clean.device}")
    if bins is None:
        if unbinned is not None:
            raise ValueError(unbinned)
        if not per_spectrum:
            raise ValueError("nothing to compute: per_spectrum=False and no bins")
        return x, y, clean, n, L, dev, 0.0, 0.0, 0, None
    lo, hi, nbins = _bins(bins)
    if report is None:
        report = _new_report(nbins, dev, words)
    else:
        _check_out(report, "report", (words(nbins),), dev, torch.int64)
    if key is not None:
        _check_out(key, "key", (n,), dev, torch.float32)
    return x, y, clean, n, L, dev, lo, hi, nbins, report


def snr(x, y, clean, key=None, bins=None, per4=None, report=None, per_spectrum=True):
    """Per-spectrum [SNR_in, SNR_out, SNR_gain] in dB (fp64, (n, 3)) of the noisy input ``x`` and the
    denoised ``y`` (float32) against ``clean`` (float32 or float64), with P = mean(clean²), and -- with
    ``bins`` = (lo, hi, nbins) -- the stratified report this batch is added to (rdn_snr).

    ``key``: float32 (n,), the value each spectrum is binned by (the nominal SNR of generate() or of a
    dataset's ``snrs``); None bins by the measured SNR_in.  ``per4``: the float64 (n, 4) per-spectrum
    output of metrics() / forward_metrics() for the same spectra, added to the bins' first four
    accumulators.  ``report``: a report of new_report(nbins) to accumulate into (made when None).
    Returns (per (n, 3) or None, report or None)."""
    _check_cuda_f32(x, "input")
    _check_cuda_f32(y, "denoised")
    _check_clean(clean)
    fed = key is not None or per4 is not None or report is not None
    x, y, clean, n, L, dev, lo, hi, nbins, report = _report_args(
        x, y, clean, (1, "spectra must have at least one sample"), key, bins, report, _lib.report_words,
        "key, per4 and report feed the binned report: pass bins=(lo, hi, nbins)" if fed else None, per_spectrum)
    if per4 is not None:
        _check_out(per4, "per4", (n, 4), dev, torch.float64)
    per = torch.empty((n, 3), dtype=torch.float64, device=dev) if per_spectrum else None
    _lib.check(_lib.lib().rdn_snr(_ptr(x), _ptr(y), _ptr(clean), int(clean.dtype == torch.float64), n, L, _ptr(per),
                                  _ptr(key), lo, hi, nbins, _ptr(per4), _ptr(report), _stream(dev)), "rdn_snr")
    return per, report


def physics(x, y, clean, weights=PHYS_WEIGHTS, key=None, bins=None, report=None, per_spectrum=True):
    """Per-spectrum [MSE, Smooth, Peak, Noise, Total, PeakCount] (fp64, (n, 6)) of PhysicsAwareLoss
    (PIDN/train.py:109-146) for the denoised ``y`` and the noisy input ``x`` (float32) against ``clean``
    (float32 or float64), Total weighted by ``weights`` = (alpha, beta, gamma); the reference's loss over
    the batch is the mean of Total.  With ``bins`` = (lo, hi, nbins) the batch is also added to a report
    binned by ``key`` (float32 (n,), e.g. the nominal or measured SNR; None puts every spectrum into row 1:
    an unbinned report is bins=(0, 1, 1) without a key).  ``report``: a report of
    new_physics_report(nbins) to accumulate into (made when None).  Returns (per (n, 6) or None, report or
    None)."""
    _check_cuda_f32(x, "input")
    _check_cuda_f32(y, "denoised")
    _check_clean(clean)
    alpha, beta, gamma = _weights(weights)
    fed = key is not None or report is not None
    x, y, clean, n, L, dev, lo, hi, nbins, report = _report_args(
        x, y, clean, (3, "spectra must have at least three samples (the peak term is a mean over L - 2)"), key, bins,
        report, _lib.phys_words, "key and report belong to the binned report: pass bins=(lo, hi, nbins)" if fed else None,
        per_spectrum)
    per = torch.empty((n, 6), dtype=torch.float64, device=dev) if per_spectrum else None
    _lib.check(_lib.lib().rdn_physics(_ptr(x), _ptr(y), _ptr(clean), int(clean.dtype == torch.float64), n, L, alpha, beta,
                                      gamma, _ptr(per), _ptr(key), lo, hi, nbins, _ptr(report), _stream(dev)), "rdn_physics")
    return per, report


def physics_grad(x, y, clean, weights=PHYS_WEIGHTS, scale=None, per_spectrum=True, out=None):
    """Value and gradient of PhysicsAwareLoss from one launch (rdn_physics_grad): the per-spectrum
    [MSE, Smooth, Peak, Noise, Total, PeakCount] of physics() -- the same bits -- and ``grad`` = ``scale`` *
    d Total / d ``y`` (float32, the shape of ``y``: (N, L) or (N, 1, L)).  ``scale`` = None means 1 / n: the
    gradient of the reference's loss, the mean of Total over the batch.  ``per_spectrum`` = False computes
    the gradient alone (no reduction, no noise passes); the noisy input ``x`` is then not read and may be
    None.  ``out``: a float32 tensor of ``y``'s shape to write the gradient into (made when None); it must
    not overlap x, y or clean.  Returns (per (n, 6) or None, grad)."""
    if x is None:
        if per_spectrum:
            raise ValueError("the per-spectrum values need the noisy input: x=None goes with per_spectrum=False")
    else:
        _check_cuda_f32(x, "input")
    _check_cuda_f32(y, "denoised")
    _check_clean(clean)
    alpha, beta, gamma = _weights(weights)
    shape = tuple(y.shape)
    x, y, clean, n, L, dev, _, _, _, _ = _report_args(
        y if x is None else x, y, clean, (3, "spectra must have at least three samples (the peak term is a mean over L - 2)"),
        None, None, None, _lib.phys_words, None, True)
    if scale is None:
        scale = 1.0 / n if n else 1.0
    scale = float(scale)
    if not abs(scale) < float("inf"):
        raise ValueError(f"scale must be finite, got {scale}")
    grad = torch.empty(shape, dtype=torch.float32, device=dev) if out is None else out
    if out is not None:
        _check_out(grad, "out", shape, dev)
    per = torch.empty((n, 6), dtype=torch.float64, device=dev) if per_spectrum else None
    _lib.check(_lib.lib().rdn_physics_grad(_ptr(x if per_spectrum else None), _ptr(y), _ptr(clean),
                                           int(clean.dtype == torch.float64), n, L, alpha, beta, gamma, scale, _ptr(per),
                                           _ptr(grad), _stream(dev)), "rdn_physics_grad")
    return per, grad


# ---- classical baseline filters (rdn_fir, rdn_median; the arithmetic contract: include/raman_mi355x.h) ----
FILTER_TILE = _lib.FILTER_TILE                  # outputs per workgroup
FILTER_MAX_WINDOW = _lib.FILTER_MAX_WINDOW


def _filter_args(x, window, out):
    """What fir() and median() do with x, the window and ``out`` before the launch: (x, y, n, L)."""
    _check_rows_input(x)
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= FILTER_MAX_WINDOW or window % 2 == 0:
        raise ValueError(f"the window must be an odd integer in [1, {FILTER_MAX_WINDOW}], got {window!r}")
    n, L = x.shape[0], x.shape[-1]
    if L < window:
        raise ValueError(f"spectra of {L} samples are shorter than the window {window}")
    return x, _out_like(x, out), n, L


def _device_taps(t, name, shape, device):
    """Filter coefficients as the kernel reads them: a contiguous float64 tensor of ``shape`` on ``device``
    (a CUDA tensor is taken as it is; anything else is copied there)."""
    if not (torch.is_tensor(t) and t.is_cuda):
        t = torch.as_tensor(t, dtype=torch.float64).to(device)
    _check_out(t, name, shape, device, torch.float64)
    return t


def fir(x, taps, edge_taps=None, out=None):
    """FIR filter of every spectrum of ``x`` (float32 (N, L) or (N, 1, L), contiguous, CUDA) with the odd
    number w = len(taps) of float64 ``taps``: y[i] = Σ_k taps[k] x[i - h + k], h = (w - 1) / 2, summed
    sequentially in fp64 and rounded once to fp32 (rdn_fir).  The ends use mirror indexing (scipy's
    mode='mirror'), or -- with ``edge_taps``, float64 (w - 1, w) -- the first and last h outputs are
    row j of the table applied to the first / last w samples (savgol_filter's mode='interp').  Taps that
    are not CUDA tensors are copied to the device on every call: a caller in a loop keeps them there.
    ``out``: a float32 tensor of x's shape to write into (made when None); it must not overlap x."""
    w = int(taps.shape[0]) if hasattr(taps, "shape") and len(taps.shape) == 1 else len(taps)
    x, y, n, L = _filter_args(x, w, out)
    taps = _device_taps(taps, "taps", (w,), x.device)
    if edge_taps is not None:
        edge_taps = _device_taps(edge_taps, "edge_taps", (w - 1, w), x.device)
    _lib.check(_lib.lib().rdn_fir(_ptr(x), _ptr(y), n, L, _ptr(taps), w, _ptr(edge_taps), _stream(x.device)), "rdn_fir")
    return y


def median(x, window, out=None):
    """Running median of every spectrum of ``x`` (float32 (N, L) or (N, 1, L), contiguous, CUDA) over the
    odd ``window``, mirror indexing at the ends (scipy.ndimage.median_filter's mode='mirror'): each output
    is bit for bit one of the inputs, ordered by the monotone key of their bits (-0 < +0); a window that
    holds a NaN gives the quiet NaN (rdn_median).  ``out`` as in fir()."""
    x, y, n, L = _filter_args(x, window, out)
    _lib.check(_lib.lib().rdn_median(_ptr(x), _ptr(y), n, L, int(window), _stream(x.device)), "rdn_median")
    return y


# ---- translation-invariant Haar shrinkage (rdn_haar_shrink; the arithmetic contract: include/raman_mi355x.h) ----
HAAR_TILE = _lib.HAAR_TILE                      # outputs per workgroup
HAAR_MAX_LEVELS = _lib.HAAR_MAX_LEVELS
HAAR_SELECT_LDS_L = _lib.HAAR_SELECT_LDS_L      # longer spectra: the median's select passes re-read them through L2
HAAR_MODES = {"soft": _lib.HAAR_SOFT, "hard": _lib.HAAR_HARD}


def haar_shrink(x, k, mode="hard", out=None, med=None):
    """Translation-invariant Haar shrinkage of every spectrum of ``x`` (float32 (N, L) or (N, 1, L), contiguous,
    CUDA) over J = len(k) levels, 1 <= J <= 7, 2^J <= L: the undecimated Haar transform with periodic indexing,
    detail plane j thresholded (``mode`` 'hard' or 'soft') at k[j - 1] * m, m the spectrum's median |d_1|, and
    the inverse transform, all in fp64 and rounded once to fp32 (rdn_haar_shrink).  ``k``: J host floats, finite
    and >= 0 (wavelets.haar_thresholds).  Returns (y, med): y float32 of x's shape, med float64 (N,), m per
    spectrum; a spectrum with a NaN or an infinity gives NaN in both.  ``out`` / ``med``: buffers to write into
    (made when None); out must not overlap x, and med neither of them."""
    _check_rows_input(x)
    if mode not in HAAR_MODES:
        raise ValueError(f"mode must be 'soft' or 'hard', got {mode!r}")
    k = [float(v) for v in (k.tolist() if hasattr(k, "tolist") else k)]
    J = len(k)
    if not 1 <= J <= HAAR_MAX_LEVELS:
        raise ValueError(f"need 1 to {HAAR_MAX_LEVELS} levels, got {J} thresholds")
    if not all(0.0 <= v < float("inf") for v in k):
        raise ValueError(f"every threshold factor must be finite and >= 0, got {k}")
    n, L = x.shape[0], x.shape[-1]
    if L < 2 ** J:
        raise ValueError(f"spectra of {L} samples are shorter than 2^{J}, the reach of {J} levels")
    y = _out_like(x, out)
    m = torch.empty(n, dtype=torch.float64, device=x.device) if med is None else med
    if med is not None:
        _check_out(m, "med", (n,), x.device, torch.float64)
        for t, name in ((x, "the input"), (y, "out")):
            _no_overlap(m, t, f"med must not overlap {name}")
    _lib.check(_lib.lib().rdn_haar_shrink(_ptr(x), _ptr(y), _ptr(m), n, L, J, (ctypes.c_double * J)(*k), HAAR_MODES[mode],
                                          _stream(x.device)), "rdn_haar_shrink")
    return y, m


def noise_mad(x, out=None):
    """m of haar_shrink alone: the median of |0.5 (x[i] - x[i - 1])| over each periodic spectrum of ``x``
    (float32 (N, L) or (N, 1, L), contiguous, CUDA; L >= 1), float64 (N,), the bits of haar_shrink's ``med``; NaN for a
    spectrum with a NaN or an infinity (rdn_noise_mad).  ``out``: a float64 (N,) buffer to write into (made when
    None); it must not overlap x."""
    _check_rows_input(x)
    n, L = x.shape[0], x.shape[-1]
    if L < 1:
        raise ValueError("spectra must have at least one sample")
    m = torch.empty(n, dtype=torch.float64, device=x.device) if out is None else out
    if out is not None:
        _check_out(m, "out", (n,), x.device, torch.float64)
        _no_overlap(m, x, "out must not overlap the input")
    _lib.check(_lib.lib().rdn_noise_mad(_ptr(x), _ptr(m), n, L, _stream(x.device)), "rdn_noise_mad")
    return m


# ---- exact piecewise-constant (Potts) fit (rdn_potts; the arithmetic contract: include/raman_mi355x.h) ----
POTTS_MAX_LEN = _lib.POTTS_MAX_LEN              # the longest segment: one candidate per lane of a wave


def potts(x, gamma, max_len=POTTS_MAX_LEN, out=None, nseg=None, work=None):
    """The jump-penalised least-squares fit of every spectrum of ``x`` (float32 (N, L) or (N, 1, L), contiguous,
    CUDA): the segmentation into runs of at most ``max_len`` (1 to 64) samples and the run means that minimise
    Σ (x - fit)² + gamma · #runs exactly, by dynamic programming in fp64, rounded once to fp32 (rdn_potts).
    ``gamma``: a float64 CUDA tensor (N,), one penalty per spectrum, or a Python float for all of them.  Returns
    (y, nseg): y float32 of x's shape, nseg int32 (N,), the number of runs.  A spectrum with a NaN or an infinity,
    or with a negative, NaN or infinite gamma, gives NaN and 0.  ``out`` / ``nseg``: buffers to write into;
    ``work``: uint8 scratch of at least N · L elements (each made when None).  None of them may overlap another
    or x."""
    _check_rows_input(x)
    if isinstance(max_len, bool) or int(max_len) != max_len or not 1 <= int(max_len) <= POTTS_MAX_LEN:
        raise ValueError(f"max_len must be an integer in [1, {POTTS_MAX_LEN}], got {max_len!r}")
    n, L = x.shape[0], x.shape[-1]
    if L < 1:
        raise ValueError("spectra must have at least one sample")
    if torch.is_tensor(gamma):
        _check_out(gamma, "gamma", (n,), x.device, torch.float64)
    else:
        if isinstance(gamma, bool):
            raise TypeError(f"gamma must be a float64 tensor or a float, got {gamma!r}")
        gamma = torch.full((n,), float(gamma), dtype=torch.float64, device=x.device)
    y = _out_like(x, out)
    segs = torch.empty(n, dtype=torch.int32, device=x.device) if nseg is None else nseg
    if nseg is not None:
        _check_out(segs, "nseg", (n,), x.device, torch.int32)
    if work is None:
        work = torch.empty(n * L, dtype=torch.uint8, device=x.device)
    else:
        if not torch.is_tensor(work):
            raise TypeError("work must be a tensor")
        if work.dtype != torch.uint8:
            raise TypeError(f"work must be torch.uint8, got {work.dtype}")
        if not work.is_cuda or work.device != x.device:
            raise ValueError(f"work must live on {x.device}, got {work.device}")
        if not work.is_contiguous():
            raise ValueError("work must be contiguous")
        if work.numel() < n * L:
            raise ValueError(f"work must have at least N * L = {n * L} elements, got {work.numel()}")
    named = ((x, "the input"), (y, "out"), (work, "work"), (segs, "nseg"), (gamma, "gamma"))
    for i in range(2, len(named)):               # out against the input: _out_like
        for b, bn in named[:i]:
            _no_overlap(named[i][0], b, f"{named[i][1]} must not overlap {bn}")
    if n == 0:                                   # nothing to launch (an empty gamma has no address to pass)
        return y, segs
    _lib.check(_lib.lib().rdn_potts(_ptr(x), _ptr(y), _ptr(segs), _ptr(gamma), n, L, int(max_len), _ptr(work),
                                    work.numel(), _stream(x.device)), "rdn_potts")
    return y, segs


# ---- Bayesian change-point smoother (rdn_bayes_steps; the arithmetic contract: include/raman_mi355x.h) ----
BAYES_MAX_LEN = _lib.BAYES_MAX_LEN              # the longest run: one candidate per lane of a wave


def bayes_steps(x, sigma, max_len=40, level_range=1.0, out=None, jump=None, logz=None, work=None):
    """The posterior mean of every spectrum of ``x`` (float32 (N, L) or (N, 1, L), contiguous, CUDA) under the
    simulator's signal model -- runs of 1 to ``max_len`` (at most 64) equal samples, levels uniform on a range of
    width ``level_range``, white Gaussian noise of standard deviation ``sigma`` -- by an exact forward-backward
    recursion in fp64, rounded once to fp32 (rdn_bayes_steps).  ``sigma``: a float64 CUDA tensor (N,), one per
    spectrum, or a Python float for all of them.  Returns (y, jump, logz): y float32 of x's shape; jump float32 of
    x's shape, the posterior probability that a run starts at each sample (1 at the first); logz float64 (N,),
    the log evidence.  A spectrum with a NaN or an infinity, or with a NaN, infinite, zero or negative sigma,
    gives NaN in all three.  ``out`` / ``jump`` / ``logz``: buffers to write into; ``work``: float64 scratch of at
    least N · (L + 1) elements (each made when None).  None of them may overlap another, x or sigma."""
    _check_rows_input(x)
    if isinstance(max_len, bool) or int(max_len) != max_len or not 1 <= int(max_len) <= BAYES_MAX_LEN:
        raise ValueError(f"max_len must be an integer in [1, {BAYES_MAX_LEN}], got {max_len!r}")
    if isinstance(level_range, bool) or not 0.0 < float(level_range) < float("inf"):
        raise ValueError(f"level_range must be positive and finite, got {level_range!r}")
    n, L = x.shape[0], x.shape[-1]
    if L < 1:
        raise ValueError("spectra must have at least one sample")
    if torch.is_tensor(sigma):
        _check_out(sigma, "sigma", (n,), x.device, torch.float64)
    else:
        if isinstance(sigma, bool):
            raise TypeError(f"sigma must be a float64 tensor or a float, got {sigma!r}")
        sigma = torch.full((n,), float(sigma), dtype=torch.float64, device=x.device)
    y = _out_like(x, out)
    jmp = torch.empty_like(x) if jump is None else jump
    if jump is not None:
        _check_out(jmp, "jump", tuple(x.shape), x.device, torch.float32)
    lz = torch.empty(n, dtype=torch.float64, device=x.device) if logz is None else logz
    if logz is not None:
        _check_out(lz, "logz", (n,), x.device, torch.float64)
    if work is None:
        work = torch.empty(n * (L + 1), dtype=torch.float64, device=x.device)
    else:
        if not torch.is_tensor(work):
            raise TypeError("work must be a tensor")
        if work.dtype != torch.float64:
            raise TypeError(f"work must be torch.float64, got {work.dtype}")
        if not work.is_cuda or work.device != x.device:
            raise ValueError(f"work must live on {x.device}, got {work.device}")
        if not work.is_contiguous():
            raise ValueError("work must be contiguous")
        if work.numel() < n * (L + 1):
            raise ValueError(f"work must have at least N * (L + 1) = {n * (L + 1)} elements, got {work.numel()}")
    named = ((x, "the input"), (y, "out"), (work, "work"), (jmp, "jump"), (lz, "logz"))
    for i in range(2, len(named)):               # out against the input: _out_like
        for b, bn in named[:i]:
            _no_overlap(named[i][0], b, f"{named[i][1]} must not overlap {bn}")
    for b, bn in named[1:]:                      # sigma is only read: it may share bytes with the input alone
        _no_overlap(sigma, b, f"sigma must not overlap {bn}")
    if n == 0:                                   # nothing to launch (an empty sigma has no address to pass)
        return y, jmp, lz
    _lib.check(_lib.lib().rdn_bayes_steps(_ptr(x), _ptr(y), _ptr(jmp), _ptr(lz), _ptr(sigma), n, L, int(max_len),
                                          float(level_range), _ptr(work), work.numel() * 8, _stream(x.device)),
               "rdn_bayes_steps")
    return y, jmp, lz


# ---- blind residual report (rdn_blind; definitions and report layout: include/raman_mi355x.h) ----
BLIND_QUANTITIES = ("Mean", "RMS", "Ratio", "Rho1", "RhoMax", "Q", "SNR_est")
BLIND_MAX_LAGS = _lib.BLIND_MAX_LAGS
BLIND_LDS_L = _lib.BLIND_LDS_L                  # longer spectra: pass 2 recomputes the residual through L2
_SIGMA_PER_MAD = math.sqrt(2.0) / 0.6744897501960817  # noise_mad's m -> the noise's standard deviation


def blind_q_crit(lags, alpha=0.01):
    """The 1 - ``alpha`` quantile of χ² with ``lags`` degrees of freedom by Wilson and Hilferty's cube,
    K (1 - 2/(9K) + z sqrt(2/(9K)))³ with z the normal quantile: the value a white residual's Ljung-Box Q
    exceeds with probability ``alpha`` (within 0.2 % of the tables for 5 <= K <= 32 at alpha = 0.01)."""
    if isinstance(lags, bool) or int(lags) != lags or not 1 <= int(lags) <= BLIND_MAX_LAGS:
        raise ValueError(f"lags must be an integer in [1, {BLIND_MAX_LAGS}], got {lags!r}")
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
    k = float(int(lags))
    z = statistics.NormalDist().inv_cdf(1.0 - float(alpha))
    return k * (1.0 - 2.0 / (9.0 * k) + z * math.sqrt(2.0 / (9.0 * k))) ** 3


def new_blind_report(nbins, device):
    """A zeroed blind report (RDN_BLIND_WORDS(nbins) int64: nbins + 2 rows) on ``device``."""
    return _new_report(nbins, device, _lib.blind_words)


def blind_value(report, nbins):
    """Doubles of a blind report (float64 (nbins + 3, 9), CPU): one row per report row -- underflow, the bins,
    overflow -- then the totals over all of them; columns {count, ΣMean, ΣRMS, ΣRatio, ΣRho1, ΣRhoMax, ΣQ,
    ΣSNR_est, count of flagged spectra}.  Each sum is the exact total rounded once, NaN where a value was out
    of range (rdn_blind_value)."""
    return _report_value(report, nbins, "blind report", _lib.blind_words, _lib.BLIND_VALUES, "rdn_blind_value")


def blind(x, y, sigma=None, lags=16, q_crit=None, key=None, bins=None, report=None, per_spectrum=True, rho=False):
    """What the residual r = x - y says about the denoised ``y`` without a clean reference (rdn_blind): per
    spectrum [Mean, RMS, Ratio = RMS / sigma, Rho1, RhoMax, Q, SNR_est] (fp64, (n, 7)), with rho_k the
    autocorrelation of the centred residual at lags 1 .. ``lags``, Q its Ljung-Box statistic and SNR_est =
    10 log10((mean(x²) - sigma²) / sigma²) dB.  A spectrum is flagged when Q > ``q_crit`` (None:
    blind_q_crit(lags), the χ² 0.99 quantile).  If y is the signal, Mean is 0, Ratio 1 and Q about ``lags``.

    ``x``, ``y``: float32 CUDA, (N, L) or (N, 1, L), L > lags.  ``sigma``: float64 CUDA (N,), each spectrum's
    noise level, a Python float for all of them, or None: the blind estimate noise_mad(x) · sqrt(2) /
    0.6744897501960817 (what PottsFit.noise_std returns).  With ``bins`` = (lo, hi, nbins) the batch is also
    added to a report binned by ``key`` (float32 (N,)), or by SNR_est when key is None; ``report``: a report
    of new_blind_report(nbins) to accumulate into (made when None).  ``rho``: also return the (N, lags)
    autocorrelations.  Returns (per (N, 7) or None, rho (N, lags) or None, report or None)."""
    _check_cuda_f32(x, "input")
    _check_cuda_f32(y, "denoised")
    if isinstance(lags, bool) or int(lags) != lags or not 1 <= int(lags) <= BLIND_MAX_LAGS:
        raise ValueError(f"lags must be an integer in [1, {BLIND_MAX_LAGS}], got {lags!r}")
    lags = int(lags)
    q_crit = blind_q_crit(lags) if q_crit is None else float(q_crit)
    if not q_crit >= 0.0:
        raise ValueError(f"q_crit must be >= 0 (inf flags nothing), got {q_crit!r}")
    x, y = _rows(x), _rows(y)
    if x.shape != y.shape:
        raise ValueError(f"shape mismatch {tuple(x.shape)} vs {tuple(y.shape)}")
    n, L = x.shape
    dev = x.device
    if y.device != dev:
        raise ValueError(f"input on {dev} but denoised on {y.device}")
    if L <= lags:
        raise ValueError(f"spectra must be longer than lags = {lags}, got L = {L}")
    if bins is None:
        if key is not None or report is not None:
            raise ValueError("key and report belong to the binned report: pass bins=(lo, hi, nbins)")
        if not (per_spectrum or rho):
            raise ValueError("nothing to compute: per_spectrum=False, rho=False and no bins")
        lo, hi, nbins = 0.0, 0.0, 0
    else:
        lo, hi, nbins = _bins(bins)
        if report is None:
            report = _new_report(nbins, dev, _lib.blind_words)
        else:
            _check_out(report, "report", (_lib.blind_words(nbins),), dev, torch.int64)
        if key is not None:
            _check_out(key, "key", (n,), dev, torch.float32)
    if sigma is None:
        sigma = noise_mad(x) * _SIGMA_PER_MAD
    elif torch.is_tensor(sigma):
        _check_out(sigma, "sigma", (n,), dev, torch.float64)
    else:
        if isinstance(sigma, bool):
            raise TypeError(f"sigma must be a float64 tensor, a float or None, got {sigma!r}")
        sigma = torch.full((n,), float(sigma), dtype=torch.float64, device=dev)
    per = torch.empty((n, len(BLIND_QUANTITIES)), dtype=torch.float64, device=dev) if per_spectrum else None
    rhos = torch.empty((n, lags), dtype=torch.float64, device=dev) if rho else None
    if n == 0:                                   # nothing to launch (an empty sigma has no address to pass)
        return per, rhos, report
    _lib.check(_lib.lib().rdn_blind(_ptr(x), _ptr(y), _ptr(sigma), n, L, lags, q_crit, _ptr(per), _ptr(rhos), _ptr(key),
                                    lo, hi, nbins, _ptr(report), _stream(dev)), "rdn_blind")
    return per, rhos, report
