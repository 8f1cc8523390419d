"""ctypes binding of libraman_mi355x.so (the C ABI declared in include/raman_mi355x.h).

torch is imported first on purpose: the library is linked against the HIP runtime that
PyTorch-ROCm bundles (torch/lib/libamdhip64.so) and must resolve to that already-loaded copy so
that device pointers and streams are shared with torch.  There is no fallback: if the library is
missing the import fails loudly.
"""
import ctypes
import glob
import hashlib
import os

import torch  # noqa: F401  (must be loaded before the library, see module docstring)

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libraman_mi355x.so")
CSRC = os.path.join(os.path.dirname(PKG), "csrc")
HEADER = os.path.join(os.path.dirname(os.path.dirname(PKG)), "include", "raman_mi355x.h")

RDN_OK = 0
ABI_VERSION = 6
# exact metric accumulator words (include/raman_mi355x.h RDN_ACC_*)
ACC_LIMBS = 6
ACC_STRIDE = ACC_LIMBS + 1
ACC_COUNT = 4 * ACC_STRIDE
ACC_WORDS = ACC_COUNT + 1
ACC_FRAC_BITS = 128
# SNR report words (include/raman_mi355x.h RDN_REPORT_*)
REPORT_QUANTITIES = 7
REPORT_MAX_BINS = 64
REPORT_COUNT = REPORT_QUANTITIES * ACC_STRIDE
REPORT_COUNT4 = REPORT_COUNT + 1
REPORT_ROW_WORDS = REPORT_COUNT4 + 1
REPORT_VALUES = REPORT_QUANTITIES + 2


def report_rows(nbins):
    return nbins + 2


def report_words(nbins):
    return report_rows(nbins) * REPORT_ROW_WORDS


# PhysicsAwareLoss report words (include/raman_mi355x.h RDN_PHYS_*)
PHYS_QUANTITIES = 6
PHYS_COUNT = PHYS_QUANTITIES * ACC_STRIDE
PHYS_ROW_WORDS = PHYS_COUNT + 1
PHYS_VALUES = PHYS_QUANTITIES + 1


def phys_words(nbins):
    return report_rows(nbins) * PHYS_ROW_WORDS


# baseline filters (include/raman_mi355x.h RDN_FILTER_*)
FILTER_MAX_WINDOW = 255
FILTER_TILE = 2048
# translation-invariant Haar shrinkage (include/raman_mi355x.h RDN_HAAR_*)
HAAR_MAX_LEVELS = 7
HAAR_TILE = 512
HAAR_SELECT_LDS_L = 12288
HAAR_SOFT, HAAR_HARD = 0, 1
# exact piecewise-constant (Potts) fit (include/raman_mi355x.h RDN_POTTS_*)
POTTS_MAX_LEN = 64
# Bayesian change-point smoother (include/raman_mi355x.h RDN_BAYES_*)
BAYES_MAX_LEN = 64
# blind residual report (include/raman_mi355x.h RDN_BLIND_*)
BLIND_MAX_LAGS = 32
BLIND_QUANTITIES = 7
BLIND_COUNT = BLIND_QUANTITIES * ACC_STRIDE
BLIND_FLAGGED = BLIND_COUNT + 1
BLIND_ROW_WORDS = BLIND_FLAGGED + 1
BLIND_VALUES = BLIND_QUANTITIES + 2
BLIND_LDS_L = 20000


def blind_words(nbins):
    return report_rows(nbins) * BLIND_ROW_WORDS



def source_hash():
    """sha256 prefix of the sources the library is built from -- the same files, in the same order,
    as csrc/Makefile's STAMP_SRC (None when the sources are not beside the package)."""
    if not os.path.isdir(CSRC):
        return None
    files = sorted(os.path.basename(p) for pat in ("*.hip", "*.cpp", "*.hpp")
                   for p in glob.glob(os.path.join(CSRC, pat)))
    paths = [os.path.join(CSRC, f) for f in files] + [os.path.join(CSRC, "Makefile"), HEADER]
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]

c_float_p = ctypes.POINTER(ctypes.c_float)
c_double_p = ctypes.POINTER(ctypes.c_double)


class GenParams(ctypes.Structure):
    _fields_ = [("signal_length", ctypes.c_int64), ("snr_lo", ctypes.c_float), ("snr_hi", ctypes.c_float),
                ("extreme_noise_prob", ctypes.c_float), ("max_repeat", ctypes.c_int32)]


_SIGNATURES = {
    "rdn_version": ([], ctypes.c_int),
    "rdn_build_id": ([], ctypes.c_char_p),
    "rdn_default_correction_mask": ([ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "rdn_get_correction_mask": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "rdn_forward_status": ([ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                            ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    "rdn_last_error": ([], ctypes.c_char_p),
    "rdn_param_names": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "rdn_packed_size": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "rdn_pack": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64),
                  ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int),
    "rdn_workspace_size": ([ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                            ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p], ctypes.c_int),
    "rdn_workspace_init": ([ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                            ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    "rdn_check_blob": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int),
    "rdn_forward": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    "rdn_forward_metrics": ([ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                             ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "rdn_forward_status_ex": ([ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                               ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)], ctypes.c_int),
    "rdn_generate": ([ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(GenParams), ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_metrics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                     ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_metrics_ex": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_acc_value": ([ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    # the SNR report: added to ABI v6 without a version bump, detected by symbol (lib())
    "rdn_snr": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p,
                 ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_report_bin": ([ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
                       ctypes.c_int),
    "rdn_report_value": ([ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    # the PhysicsAwareLoss report: likewise added to ABI v6 and detected by symbol
    "rdn_physics": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                     ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                     ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_physics_value": ([ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    # value and gradient of PhysicsAwareLoss from one launch: likewise added to ABI v6 and detected by symbol
    "rdn_physics_grad": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                          ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    # the classical baseline filters: likewise added to ABI v6 and detected by symbol
    "rdn_fir": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
                 ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_median": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p],
                   ctypes.c_int),
    # translation-invariant Haar shrinkage: likewise added to ABI v6 and detected by symbol
    "rdn_haar_shrink": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                         c_double_p, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    # the blind noise estimate alone and the exact piecewise-constant (Potts) fit: likewise
    "rdn_noise_mad": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p], ctypes.c_int),
    "rdn_potts": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                   ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    # the Bayesian change-point smoother: likewise
    "rdn_bayes_steps": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                         ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p,
                         ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
    # the blind residual report: likewise added to ABI v6 and detected by symbol
    "rdn_blind": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                   ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float,
                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
    "rdn_blind_value": ([ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
}

EXPORTED = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load (once) and return the native library.  Raises ImportError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"raman_mi355x native library not built: {LIB_PATH} is missing "
                              "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C csrc`)")
        handle = ctypes.CDLL(LIB_PATH)
        missing = [name for name in _SIGNATURES if not hasattr(handle, name)]
        if missing:
            raise ImportError(f"libraman_mi355x.so lacks {', '.join(missing)}: it was built from older sources; "
                              "rebuild it (make -C csrc, or __graft_entry__.build())")
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = res
        if handle.rdn_version() != ABI_VERSION:
            raise ImportError(f"libraman_mi355x ABI {handle.rdn_version()} != expected {ABI_VERSION}")
        built, tree = handle.rdn_build_id().decode(), source_hash()
        if tree is not None and built != tree and os.environ.get("RDN_ALLOW_STALE_LIB") != "1":
            raise ImportError(f"stale libraman_mi355x.so: built from sources {built}, this tree's sources hash to "
                              f"{tree}; rebuild it (make -C csrc, or __graft_entry__.build())")
        _lib = handle
    return _lib


RDN_ERANGE = -6


class EngineError(RuntimeError):
    pass


class RangeError(EngineError):
    """RDN_ERANGE: an RDN_F16F8 / RDN_F16MIX activation left the e4m3 correction planes' range (the
    affected tiles' outputs are NaN); RDN_F32 / RDN_BF16X3 have no such bound."""


def check(rc, what):
    if rc != RDN_OK:
        msg = lib().rdn_last_error().decode(errors="replace")
        raise (RangeError if rc == RDN_ERANGE else EngineError)(f"{what} failed (code {rc}): {msg}")
