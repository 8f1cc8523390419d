// C ABI (include/raman_mi355x.h): argument checking, error reporting and dispatch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>

#include "../../include/raman_mi355x.h"
#include "common.hpp"
#include "netspec.hpp"
#include "host_util.hpp"
#include "geometry.hpp"
#include "snr.hpp"
#include "physics.hpp"
#include "filters.hpp"
#include "haar.hpp"
#include "potts.hpp"
#include "bayes.hpp"
#include "blind.hpp"

namespace rdn {
std::string pack(int arch, int dtype, const float* const* tensors, const int64_t* numels, int n, void* dst, size_t cap);
size_t packed_bytes(const std::vector<Op>& spec, int dtype);
void set_corr_mask(void* blob, uint64_t mask);
uint64_t get_corr_mask(const void* blob);
uint32_t get_blob_tag(const void* blob);
uint64_t f16mix_default_mask(int arch);
hipError_t launch_fused16(int arch, const uint8_t* blob, const float* x, float* y, int64_t n, int L, unsigned* status,
                          hipStream_t s);
hipError_t launch_fused16_f16(int arch, const uint8_t* blob, const float* x, float* y, int64_t n, int L, unsigned* status,
                              hipStream_t s);
hipError_t launch_fused16_f16_walk(int arch, const uint8_t* blob, const float* x, float* y, int64_t n, int L,
                                   unsigned* status, const met::MetricOut* mo, hipStream_t s);
hipError_t launch_fused16_f16_small(int arch, const uint8_t* blob, const float* x, float* y, int64_t n, int L,
                                   unsigned* status, hipStream_t s);
hipError_t launch_fused_inplace_walk(const uint8_t* blob, const float* x, float* y, int64_t n, int L, unsigned* status,
                                     const met::MetricOut* mo, hipStream_t s);
hipError_t launch_fused_inplace_short(const uint8_t* blob, const float* x, float* y, int64_t n, int L, unsigned* status,
                                      hipStream_t s);
hipError_t launch_fused_inplace(int arch, int dtype, const uint8_t* blob, const float* x, float* y, int64_t n, int L,
                                unsigned* status, hipStream_t s);

hipError_t launch_cbam_forward(int arch, int dtype, const uint8_t* blob, const float* x, float* y, int64_t n, int L,
                               void* ws, size_t ws_bytes, hipStream_t s);
size_t cbam_workspace_bytes(int arch, int dtype, int64_t n, int64_t L, hipStream_t s);
hipError_t cbam_status(int arch, int dtype, int64_t L, void* ws, size_t ws_bytes, hipStream_t s, int* timed_out,
                       int* out_of_range, int* gate);
hipError_t cbam_workspace_init(int arch, int dtype, int64_t L, void* ws, size_t ws_bytes, hipStream_t s);
hipError_t launch_generate(uint64_t seed, uint64_t first, int64_t n, int L, float snr_lo, float snr_hi, float extreme_prob,
                           int max_repeat, float* clean, float* noisy, float* snr, float* nstd, hipStream_t s);
hipError_t launch_metrics(const float* y, const void* clean, bool clean_f64, int64_t n, int L, double* per, double* sums,
                          long long* acc, hipStream_t s);
hipError_t launch_snr(const float* x, const float* y, const void* clean, bool clean_f64, int64_t n, int L,
                      const snr::SnrOut& so, hipStream_t s);
hipError_t launch_physics(const float* x, const float* y, const void* clean, bool clean_f64, int64_t n, int L,
                          const phys::PhysOut& po, hipStream_t s);
}  // namespace rdn

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return RDN_OK;
  return fail(RDN_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

bool valid_arch(int a) { return a >= RDN_DENOISECNN && a <= RDN_APIDN; }
bool valid_dtype(int d) { return d >= RDN_F32 && d <= RDN_F16MIX; }
// a batch of n rows of L samples, lo <= L: not (n >= 0 and lo <= L < 2^31)
bool bad_rows(int64_t n, int64_t L, int64_t lo) { return n < 0 || L < lo || L > 0x7fffffff; }
// bytes of n (>= 0) float32 rows of L samples; 0 for an empty batch, which overlaps nothing
size_t row_bytes(int64_t n, int64_t L) { return (size_t)n * (size_t)L * sizeof(float); }
bool is_cbam(int a) { return a == RDN_ADSDN || a == RDN_APIDN; }
// the dtypes whose e4m3 correction planes bound the activations (RDN_ERANGE, inplace.hpp range_vote)
bool range_checked(int d) { return d == RDN_F16F8 || d == RDN_F16MIX; }
// the fused networks' 16-bit forwards keep a status word in the first 4 bytes of a RANGE_WS_BYTES
// workspace (common.hpp STATUS_*): the range bit of the range-checked dtypes and, for every 16-bit
// dtype, the input gate bit raised by the stems
bool status_word(int d) { return d != RDN_F32; }
constexpr size_t RANGE_WS_BYTES = 256;
const char* range_msg() {
  return "an activation left the range of the e4m3 correction planes (|v| > 1792, RDN_F16F8 / RDN_F16MIX): the "
         "affected tiles' outputs are NaN; inputs this large need RDN_F32 or RDN_BF16X3";
}
// RDN_F16MIX exists for RRCDNet only (checked before any per-network dispatch)
bool unsupported(int arch, int dtype) { return dtype == RDN_F16MIX && arch != RDN_RRCDNET; }
int fail_unsupported(const char* fn) {
  return fail(RDN_EUNSUPPORTED, std::string(fn) + ": RDN_F16MIX is built for RRCDNet; the other networks run RDN_F16");
}

static_assert(rdn::BLOB_MAGIC == RDN_BLOB_MAGIC, "blob tag magic");
static_assert(sizeof(long long) == sizeof(int64_t), "accumulator words");

}  // namespace

#define RDN_GUARD_BEGIN try {
#define RDN_GUARD_END                                     \
  }                                                       \
  catch (const std::exception& ex) {                      \
    return fail(RDN_EINVAL, std::string("exception: ") + ex.what()); \
  }                                                       \
  catch (...) {                                           \
    return fail(RDN_EINVAL, "unknown exception");         \
  }

extern "C" {

#ifndef RDN_SOURCE_HASH
#define RDN_SOURCE_HASH "unstamped"
#endif

int rdn_version(void) { return RDN_ABI_VERSION; }

const char* rdn_build_id(void) { return RDN_SOURCE_HASH; }

const char* rdn_last_error(void) { return g_err.c_str(); }

int rdn_param_names(int arch, char* buf, size_t cap, size_t* needed) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch)) return fail(RDN_EINVAL, "unknown arch " + std::to_string(arch));
  std::string all;
  for (const std::string& s : rdn::param_names(rdn::net_spec(arch))) {
    all += s;
    all += '\n';
  }
  if (needed) *needed = all.size() + 1;
  if (buf && cap) {
    const size_t n = all.size() + 1 <= cap ? all.size() + 1 : cap;
    std::memcpy(buf, all.c_str(), n);
    buf[n - 1] = '\0';
    if (n < all.size() + 1) return fail(RDN_ESIZE, "buffer too small for parameter names");
  }
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_packed_size(int arch, int dtype, size_t* bytes) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || !bytes) return fail(RDN_EINVAL, "rdn_packed_size: bad argument");
  *bytes = rdn::packed_bytes(rdn::net_spec(arch), dtype);
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_pack(int arch, int dtype, const float* const* tensors, const int64_t* numels, int n_tensors, void* dst,
             size_t cap) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || !tensors || !numels || !dst || n_tensors < 0)
    return fail(RDN_EINVAL, "rdn_pack: bad argument");
  const std::string err = rdn::pack(arch, dtype, tensors, numels, n_tensors, dst, cap);
  if (!err.empty()) {
    const bool shape = err.find("expected") != std::string::npos || err.find("tensors") != std::string::npos;
    return fail(err.find("too small") != std::string::npos ? RDN_ESIZE : shape ? RDN_ESHAPE : RDN_EINVAL, err);
  }
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_check_blob(int arch, int dtype, const void* host_blob, size_t bytes) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || !host_blob) return fail(RDN_EINVAL, "rdn_check_blob: bad argument");
  if (unsupported(arch, dtype)) return fail_unsupported("rdn_check_blob");
  const size_t need = rdn::packed_bytes(rdn::net_spec(arch), dtype);
  if (bytes < need) return fail(RDN_ESIZE, "rdn_check_blob: blob of " + std::to_string(bytes) + " bytes, the layout needs " +
                                               std::to_string(need));
  const uint32_t tag = rdn::get_blob_tag(host_blob);
  if (tag != rdn::blob_tag(arch, dtype)) {
    if ((tag & 0xffff0000u) != RDN_BLOB_MAGIC) return fail(RDN_EINVAL, "rdn_check_blob: not an rdn_pack blob (no layout tag)");
    return fail(RDN_EINVAL, "rdn_check_blob: blob packed for arch " + std::to_string((tag >> 8) & 0xff) + " dtype " +
                                std::to_string(tag & 0xff) + ", not arch " + std::to_string(arch) + " dtype " +
                                std::to_string(dtype));
  }
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_default_correction_mask(int arch, uint64_t* mask) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !mask) return fail(RDN_EINVAL, "rdn_default_correction_mask: bad argument");
  *mask = rdn::f16mix_default_mask(arch);
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_get_correction_mask(int arch, int dtype, const void* host_blob, size_t bytes, uint64_t* mask) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || !host_blob || !mask)
    return fail(RDN_EINVAL, "rdn_get_correction_mask: bad argument");
  if (dtype != RDN_F16F8 && dtype != RDN_F16MIX) return fail(RDN_EINVAL, "rdn_get_correction_mask: not a correction layout");
  const int chk = rdn_check_blob(arch, dtype, host_blob, bytes);
  if (chk != RDN_OK) return chk;
  *mask = rdn::get_corr_mask(host_blob);
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_workspace_size(int arch, int dtype, int64_t n, int64_t L, size_t* bytes, void* stream) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || !bytes || n < 0 || L < 1)
    return fail(RDN_EINVAL, "rdn_workspace_size: bad argument");
  if (unsupported(arch, dtype)) return fail_unsupported("rdn_workspace_size");
  *bytes = is_cbam(arch) ? rdn::cbam_workspace_bytes(arch, dtype, n, L, (hipStream_t)stream)
                          : status_word(dtype) ? RANGE_WS_BYTES : 0;
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_workspace_init(int arch, int dtype, int64_t n, int64_t L, void* ws, size_t ws_bytes, void* stream) {
  RDN_GUARD_BEGIN
  if (!valid_arch(arch) || !valid_dtype(dtype) || bad_rows(n, L, 1))
    return fail(RDN_EINVAL, "rdn_workspace_init: bad argument");
  if (unsupported(arch, dtype)) return fail_unsupported("rdn_workspace_init");
  const hipStream_t s = (hipStream_t)stream;
  if (!is_cbam(arch)) {
    if (!status_word(dtype)) return RDN_OK;
    if (!ws || ws_bytes < RANGE_WS_BYTES)
      return fail(RDN_ESIZE, "rdn_workspace_init: workspace too small, need " + std::to_string(RANGE_WS_BYTES) + " bytes");
    return hip_check(hipMemsetAsync(ws, 0, 4, s), "rdn_workspace_init");
  }
  const size_t need = rdn::cbam_workspace_bytes(arch, dtype, n, L, s);
  if (ws_bytes < need || (need && !ws))
    return fail(RDN_ESIZE, "rdn_workspace_init: workspace too small, need " + std::to_string(need) + " bytes");
  return hip_check(rdn::cbam_workspace_init(arch, dtype, L, ws, ws_bytes, s), "rdn_workspace_init");
  RDN_GUARD_END
}

// RDN_SHORT_TILES / RDN_WALK = 0 / 1 force either answer of forward_geometry (geometry.hpp); -1: not set
static int env_override(const char* name) {
  const char* env = std::getenv(name);
  return env && (env[0] == '0' || env[0] == '1') ? env[0] - '0' : -1;
}

// The forward of rdn_forward / rdn_forward_metrics.  mo (may be NULL): metrics of y against mo->clean;
// on the walk geometry the forward kernel computes them (each spectrum's workgroup after its walk,
// *fused = true), otherwise the metrics kernel runs after the forward on the same stream.
static int forward_impl(const char* who, int arch, int dtype, const void* packed, const float* x, float* y, int64_t n,
                        int64_t L, void* ws, size_t ws_bytes, const rdn::met::MetricOut* mo, hipStream_t s, bool* fused) {
  if (!valid_arch(arch) || !valid_dtype(dtype)) return fail(RDN_EINVAL, std::string(who) + ": unknown arch/dtype");
  // x / y may be NULL for an empty batch (an empty torch tensor's data pointer); the blob may not
  if (!packed || (n > 0 && (!x || !y))) return fail(RDN_EINVAL, std::string(who) + ": null pointer");
  if (bad_rows(n, L, 1)) return fail(RDN_EINVAL, std::string(who) + ": need n >= 0 and 1 <= L < 2^31");
  if (mo && L < 7) return fail(RDN_EINVAL, std::string(who) + ": need L >= 7 (SSIM window)");
  if (n == 0) return RDN_OK;
  // tiles re-read their input halos while other tiles' outputs (and parked head rows) land in y
  if (rdn::overlaps(x, row_bytes(n, L), y, row_bytes(n, L))) return fail(RDN_EINVAL, std::string(who) + ": x and y overlap");
  if (unsupported(arch, dtype)) return fail_unsupported(who);
  const uint8_t* blob = (const uint8_t*)packed;
  hipError_t e = hipSuccess;
  bool done = false;          // metrics computed by the forward kernel
  if (is_cbam(arch)) {
    const size_t need = rdn::cbam_workspace_bytes(arch, dtype, n, L, s);
    if (ws_bytes < need || (need && !ws))
      return fail(RDN_ESIZE, std::string(who) + ": workspace too small, need " + std::to_string(need) + " bytes");
    e = rdn::launch_cbam_forward(arch, dtype, blob, x, y, n, (int)L, ws, ws_bytes, s);
  } else {
    // status word of the 16-bit dtypes (optional: without a workspace a saturated tile still writes NaN,
    // and the input gate is not reported)
    unsigned* status = status_word(dtype) && ws && ws_bytes >= RANGE_WS_BYTES ? (unsigned*)ws : nullptr;
    // the epilogue's direct path (spectra too long for the LDS, metrics.hpp walk_metrics_t) addresses y
    // with 32-bit byte counts: from L = 2^29 on the walk runs without it (kmo) and the metrics kernel follows
    const rdn::met::MetricOut* kmo = L < ((int64_t)1 << 29) ? mo : nullptr;
    const bool f16 = dtype == RDN_F16;     // else, off the Tiled geometry, RDN_F16MIX
    switch (rdn::forward_geometry(arch, dtype, n, L, rdn::device_cus(rdn::stream_device(s)),
                                  env_override("RDN_SHORT_TILES"), env_override("RDN_WALK"))) {
      case rdn::Geometry::Walk:
        e = f16 ? rdn::launch_fused16_f16_walk(arch, blob, x, y, n, (int)L, status, kmo, s)
                : rdn::launch_fused_inplace_walk(blob, x, y, n, (int)L, status, kmo, s), done = kmo != nullptr;
        break;
      case rdn::Geometry::Short:
        e = f16 ? rdn::launch_fused16_f16_small(arch, blob, x, y, n, (int)L, status, s)
                : rdn::launch_fused_inplace_short(blob, x, y, n, (int)L, status, s);
        break;
      case rdn::Geometry::Tiled:
        e = dtype == RDN_BF16 ? rdn::launch_fused16(arch, blob, x, y, n, (int)L, status, s)
            : f16             ? rdn::launch_fused16_f16(arch, blob, x, y, n, (int)L, status, s)
                              : rdn::launch_fused_inplace(arch, dtype, blob, x, y, n, (int)L, status, s);
        break;
    }
  }
  if (e != hipSuccess) return hip_check(e, who);
  done = done && mo;
  if (fused) *fused = done;
  if (mo && !done) e = rdn::launch_metrics(y, mo->clean, mo->clean_f64 != 0, n, (int)L, mo->per, mo->sums, mo->acc, s);
  return hip_check(e, who);
}

int rdn_forward(int arch, int dtype, const void* packed, const float* x, float* y, int64_t n, int64_t L, void* ws,
                size_t ws_bytes, void* stream) {
  RDN_GUARD_BEGIN
  return forward_impl("rdn_forward", arch, dtype, packed, x, y, n, L, ws, ws_bytes, nullptr, (hipStream_t)stream, nullptr);
  RDN_GUARD_END
}

int rdn_forward_metrics(int arch, int dtype, const void* packed, const float* x, float* y, int64_t n, int64_t L,
                        const void* clean, int clean_is_f64, double* per_spectrum, double* sums, int64_t* acc, void* ws,
                        size_t ws_bytes, void* stream, int* fused) {
  RDN_GUARD_BEGIN
  if (!clean && n > 0) return fail(RDN_EINVAL, "rdn_forward_metrics: null clean pointer");
  if (clean_is_f64 != 0 && clean_is_f64 != 1) return fail(RDN_EINVAL, "rdn_forward_metrics: clean_is_f64 must be 0 or 1");
  const rdn::met::MetricOut mo{clean, clean_is_f64, per_spectrum, sums, (long long*)acc};
  bool f = false;
  const int rc = forward_impl("rdn_forward_metrics", arch, dtype, packed, x, y, n, L, ws, ws_bytes, &mo, (hipStream_t)stream, &f);
  if (fused) *fused = rc == RDN_OK && f ? 1 : 0;
  return rc;
  RDN_GUARD_END
}

// rdn_forward_status / rdn_forward_status_ex: wait for the stream, read and clear every sticky status
// word, report all of them through *flags, fail on a hand-off timeout (RDN_EHIP) or a saturated
// activation (RDN_ERANGE); the input gate is informational (flags only).
static int forward_status(const char* who, int arch, int dtype, int64_t n, int64_t L, void* ws, size_t ws_bytes,
                          hipStream_t s, unsigned* flags) {
  if (flags) *flags = 0;
  if (!valid_arch(arch) || !valid_dtype(dtype)) return fail(RDN_EINVAL, std::string(who) + ": unknown arch/dtype");
  if (bad_rows(n, L, 1)) return fail(RDN_EINVAL, std::string(who) + ": bad n / L");
  if (unsupported(arch, dtype)) return fail_unsupported(who);
  if (!is_cbam(arch)) {
    if (!status_word(dtype) || !ws || ws_bytes < RANGE_WS_BYTES) return hip_check(hipStreamSynchronize(s), who);
    // the word's copy is ordered behind the forwards on their stream: one wait covers both
    unsigned w = 0;
    int rc = hip_check(rdn::read_words(&w, ws, sizeof(w), s), who);
    if (rc != RDN_OK) return rc;
    if (!w) return RDN_OK;
    if (flags) *flags = w & (RDN_STATUS_RANGE | RDN_STATUS_GATE);
    // cleared on the forwards' stream: ordered before the next forward enqueued there
    rc = hip_check(hipMemsetAsync(ws, 0, 4, s), who);
    // the input-gate bit is informational (the module's fp32 re-run decision): only the range bit fails
    return rc != RDN_OK || !(w & rdn::STATUS_RANGE) ? rc : fail(RDN_ERANGE, range_msg());
  }
  // n = 0 with no workspace: nothing ran.  With one, its sticky words may hold earlier forwards' bits
  // (a workspace made for an empty batch and reused for larger ones): read them
  if (n == 0 && !ws) return hip_check(hipStreamSynchronize(s), who);
  const size_t need = rdn::cbam_workspace_bytes(arch, dtype, n, L, s);
  if (ws_bytes < need || (need && !ws))
    return fail(RDN_ESIZE, std::string(who) + ": workspace smaller than this device's CBAM geometry needs (" +
                               std::to_string(need) + " bytes)");
  int timed_out = 0, out_of_range = 0, gate = 0;
  const int rc = hip_check(rdn::cbam_status(arch, dtype, L, ws, ws_bytes, s, &timed_out, &out_of_range, &gate), who);
  if (rc != RDN_OK) return rc;
  if (flags)
    *flags = (out_of_range ? RDN_STATUS_RANGE : 0u) | (gate ? RDN_STATUS_GATE : 0u) | (timed_out ? RDN_STATUS_TIMEOUT : 0u);
  if (timed_out)
    return fail(RDN_EHIP, "CBAM team hand-off timed out: a workgroup of a spectrum's team never arrived (the "
                          "grid's co-residency was broken, e.g. by a concurrent kernel on the device); the "
                          "affected spectra's outputs are NaN");
  if (out_of_range) return fail(RDN_ERANGE, range_msg());
  return RDN_OK;
}

int rdn_forward_status(int arch, int dtype, int64_t n, int64_t L, void* ws, size_t ws_bytes, void* stream) {
  RDN_GUARD_BEGIN
  return forward_status("rdn_forward_status", arch, dtype, n, L, ws, ws_bytes, (hipStream_t)stream, nullptr);
  RDN_GUARD_END
}

int rdn_forward_status_ex(int arch, int dtype, int64_t n, int64_t L, void* ws, size_t ws_bytes, void* stream,
                          unsigned* flags) {
  RDN_GUARD_BEGIN
  return forward_status("rdn_forward_status_ex", arch, dtype, n, L, ws, ws_bytes, (hipStream_t)stream, flags);
  RDN_GUARD_END
}

int rdn_generate(uint64_t seed, uint64_t first_index, int64_t n, const rdn_gen_params* p, float* clean, float* noisy,
                 float* snr_db, float* noise_std, void* stream) {
  RDN_GUARD_BEGIN
  if (!p || (n > 0 && (!clean || !noisy))) return fail(RDN_EINVAL, "rdn_generate: null pointer");
  if (n < 0 || p->signal_length < 1 || p->signal_length > 0x7fffffff || p->max_repeat < 1 || !(p->snr_hi >= p->snr_lo))
    return fail(RDN_EINVAL, "rdn_generate: bad parameters");
  // the kernel scans 256 segment lengths per pass in int: a pass starts below L and adds at most 256 * max_repeat
  if (p->signal_length + 256 * (int64_t)p->max_repeat > 0x7fffffff)
    return fail(RDN_EINVAL, "rdn_generate: signal_length + 256 * max_repeat exceeds INT32_MAX");
  if (!std::isfinite(p->snr_lo) || !std::isfinite(p->snr_hi) || std::isnan(p->extreme_noise_prob))
    return fail(RDN_EINVAL, "rdn_generate: non-finite snr_lo / snr_hi or NaN extreme_noise_prob");
  if (n == 0) return RDN_OK;
  return hip_check(rdn::launch_generate(seed, first_index, n, (int)p->signal_length, p->snr_lo, p->snr_hi,
                                        p->extreme_noise_prob, p->max_repeat, clean, noisy, snr_db, noise_std,
                                        (hipStream_t)stream),
                   "generate");
  RDN_GUARD_END
}

int rdn_metrics(const float* y, const float* clean, int64_t n, int64_t L, double* per_spectrum, double* sums,
                void* stream) {
  RDN_GUARD_BEGIN
  if (n > 0 && (!y || !clean)) return fail(RDN_EINVAL, "rdn_metrics: null pointer");
  if (bad_rows(n, L, 7)) return fail(RDN_EINVAL, "rdn_metrics: need L >= 7 (SSIM window)");
  if (n == 0) return RDN_OK;
  return hip_check(rdn::launch_metrics(y, clean, false, n, (int)L, per_spectrum, sums, nullptr, (hipStream_t)stream),
                   "metrics");
  RDN_GUARD_END
}

int rdn_metrics_ex(const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L, double* per_spectrum,
                   double* sums, int64_t* acc, void* stream) {
  RDN_GUARD_BEGIN
  if (n > 0 && (!y || !clean)) return fail(RDN_EINVAL, "rdn_metrics_ex: null pointer");
  if (clean_is_f64 != 0 && clean_is_f64 != 1) return fail(RDN_EINVAL, "rdn_metrics_ex: clean_is_f64 must be 0 or 1");
  if (bad_rows(n, L, 7)) return fail(RDN_EINVAL, "rdn_metrics_ex: need L >= 7 (SSIM window)");
  if (n == 0) return RDN_OK;
  return hip_check(rdn::launch_metrics(y, clean, clean_is_f64 == 1, n, (int)L, per_spectrum, sums, (long long*)acc,
                                       (hipStream_t)stream),
                   "metrics");
  RDN_GUARD_END
}

// Exact accumulator -> doubles: the limbs are carried into base-2^32 digits of the signed total
// (sign-magnitude after one negation), whose leading 64 bits with a sticky bit for the rest
// convert to double with one round-to-nearest-even.
static double acc_to_double(const int64_t* limb) {
  int64_t l[RDN_ACC_LIMBS];
  for (int j = 0; j < RDN_ACC_LIMBS; ++j) l[j] = limb[j];
  auto carry = [&](uint32_t (&d)[RDN_ACC_LIMBS + 2]) {
    __int128 c = 0;
    for (int j = 0; j < RDN_ACC_LIMBS; ++j) {
      const __int128 t = (__int128)l[j] + c;
      d[j] = (uint32_t)(t & 0xffffffff);
      c = (t - (__int128)d[j]) / ((__int128)1 << 32);
    }
    d[RDN_ACC_LIMBS] = (uint32_t)(c & 0xffffffff);
    d[RDN_ACC_LIMBS + 1] = (uint32_t)((c >> 32) & 0xffffffff);
    return c < 0;
  };
  uint32_t d[RDN_ACC_LIMBS + 2];
  bool neg = carry(d);
  if (neg) {
    for (int j = 0; j < RDN_ACC_LIMBS; ++j) l[j] = -l[j];
    carry(d);
  }
  int top = RDN_ACC_LIMBS + 1;
  while (top >= 0 && d[top] == 0) --top;
  if (top < 0) return 0.0;
  const int hb = 32 * top + (31 - __builtin_clz(d[top]));     // highest set bit
  auto bit = [&](int i) -> uint64_t { return i < 0 ? 0 : (d[i >> 5] >> (i & 31)) & 1u; };
  uint64_t u = 0;
  const int lo = hb - 63;
  for (int i = hb; i >= lo; --i) u = (u << 1) | bit(i);
  bool sticky = false;
  for (int i = lo - 1; i >= 0 && !sticky; --i) sticky = bit(i);
  const double v = std::ldexp((double)(u | (sticky ? 1u : 0u)), lo - RDN_ACC_FRAC_BITS);
  return neg ? -v : v;
}

// Rows of accumulators -> doubles (rdn_acc_value, rdn_report_value, rdn_physics_value).  A row of
// row_words words is `quantities` accumulators of RDN_ACC_STRIDE words and then `counts` count words; it
// becomes quantities + counts doubles: the first `lead` counts, the quantities (NaN where the out-of-range
// word is set), the other counts.  With `totals` one more row follows: the integer sums of the rows'
// words (at most 66 rows of |limb| < 2^63 / 66: a report holds up to 2^31 spectra of 32-bit chunks),
// added without sign overflow in unsigned arithmetic.
static void acc_rows_value(const int64_t* words, int rows, int row_words, int quantities, int counts, int lead,
                           bool totals, double* out) {
  const int values = quantities + counts;
  int64_t total[RDN_REPORT_ROW_WORDS] = {};
  auto row_value = [&](const int64_t* r, double* o) {
    const int64_t* c = r + quantities * RDN_ACC_STRIDE;
    for (int i = 0; i < lead; ++i) o[i] = (double)c[i];
    for (int k = 0; k < quantities; ++k) {
      const int64_t* a = r + k * RDN_ACC_STRIDE;
      o[lead + k] = a[RDN_ACC_LIMBS] ? std::nan("") : acc_to_double(a);
    }
    for (int i = lead; i < counts; ++i) o[quantities + i] = (double)c[i];
  };
  for (int b = 0; b < rows; ++b) {
    const int64_t* r = words + (size_t)b * row_words;
    row_value(r, out + (size_t)b * values);
    for (int w = 0; w < row_words; ++w) total[w] = (int64_t)((uint64_t)total[w] + (uint64_t)r[w]);
  }
  if (totals) row_value(total, out + (size_t)rows * values);
}
static_assert(RDN_ACC_WORDS <= RDN_REPORT_ROW_WORDS && RDN_PHYS_ROW_WORDS <= RDN_REPORT_ROW_WORDS &&
                  RDN_BLIND_ROW_WORDS <= RDN_REPORT_ROW_WORDS,
              "total[]");

int rdn_acc_value(const int64_t* acc, double* sums) {
  RDN_GUARD_BEGIN
  if (!acc || !sums) return fail(RDN_EINVAL, "rdn_acc_value: null pointer");
  acc_rows_value(acc, 1, RDN_ACC_WORDS, 4, 1, 0, false, sums);
  return RDN_OK;
  RDN_GUARD_END
}

static bool valid_bins(float lo, float hi, int nbins) {
  return nbins >= 1 && nbins <= RDN_REPORT_MAX_BINS && std::isfinite(lo) && std::isfinite(hi) && lo < hi &&
         std::isfinite(hi - lo);
}
static const char* bins_msg() { return "need 1 <= nbins <= 64 and finite lo < hi"; }

// The arguments rdn_snr and rdn_physics share, checked in the order their errors have always been
// reported in.  rows: x, y and clean are all given; weights_ok: rdn_physics's weights are finite;
// fed: NULL, or the inputs given that only a report reads ("key feeds"); per_name: the per-spectrum output.
static int check_report_call(const std::string& fn, int64_t min_L, bool rows, int clean_is_f64, int64_t n, int64_t L,
                             bool weights_ok, const void* report, float lo, float hi, int nbins, const char* fed,
                             const void* per, const char* per_name) {
  if (n > 0 && !rows) return fail(RDN_EINVAL, fn + ": null pointer");
  if (clean_is_f64 != 0 && clean_is_f64 != 1) return fail(RDN_EINVAL, fn + ": clean_is_f64 must be 0 or 1");
  if (bad_rows(n, L, min_L)) return fail(RDN_EINVAL, fn + ": need n >= 0 and " + std::to_string(min_L) + " <= L < 2^31");
  if (!weights_ok) return fail(RDN_EINVAL, fn + ": the weights alpha, beta, gamma must be finite");
  if (report && !valid_bins(lo, hi, nbins)) return fail(RDN_EINVAL, fn + ": " + bins_msg());
  if (!report && fed) return fail(RDN_EINVAL, fn + ": " + fed + " the report, which is NULL");
  if (!report && !per) return fail(RDN_EINVAL, fn + ": neither " + per_name + " nor report to write");
  return RDN_OK;
}
static int check_report_value(const std::string& fn, const int64_t* report, int nbins, const double* out) {
  if (!report || !out) return fail(RDN_EINVAL, fn + ": null pointer");
  if (nbins < 1 || nbins > RDN_REPORT_MAX_BINS) return fail(RDN_EINVAL, fn + ": need 1 <= nbins <= 64");
  return RDN_OK;
}

int rdn_snr(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
            double* per_spectrum3, const float* key, float lo, float hi, int nbins, const double* per4,
            int64_t* report, void* stream) {
  RDN_GUARD_BEGIN
  const int rc = check_report_call("rdn_snr", 1, x && y && clean, clean_is_f64, n, L, true, report, lo, hi, nbins,
                                   key || per4 ? "key / per4 feed" : nullptr, per_spectrum3, "per_spectrum3");
  if (rc != RDN_OK || n == 0) return rc;
  const rdn::snr::SnrOut so{per_spectrum3, key, per4, (long long*)report,
                            report ? rdn::make_bins(lo, hi, nbins) : rdn::Bins{0.f, 0.f, 0.f, 0}};
  return hip_check(rdn::launch_snr(x, y, clean, clean_is_f64 == 1, n, (int)L, so, (hipStream_t)stream), "snr");
  RDN_GUARD_END
}

int rdn_report_bin(float key, float lo, float hi, int nbins, int* row) {
  RDN_GUARD_BEGIN
  if (!row) return fail(RDN_EINVAL, "rdn_report_bin: null pointer");
  if (!valid_bins(lo, hi, nbins)) return fail(RDN_EINVAL, std::string("rdn_report_bin: ") + bins_msg());
  *row = rdn::bin_row(key, rdn::make_bins(lo, hi, nbins));
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_report_value(const int64_t* report, int nbins, double* out) {
  RDN_GUARD_BEGIN
  const int rc = check_report_value("rdn_report_value", report, nbins, out);
  if (rc != RDN_OK) return rc;
  acc_rows_value(report, RDN_REPORT_ROWS(nbins), RDN_REPORT_ROW_WORDS, RDN_REPORT_QUANTITIES, 2, 1, true, out);
  return RDN_OK;
  RDN_GUARD_END
}

int rdn_physics(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
                double alpha, double beta, double gamma, double* per_spectrum6, const float* key, float lo,
                float hi, int nbins, int64_t* report, void* stream) {
  RDN_GUARD_BEGIN
  const int rc = check_report_call("rdn_physics", 3, x && y && clean, clean_is_f64, n, L,
                                   std::isfinite(alpha) && std::isfinite(beta) && std::isfinite(gamma), report, lo, hi,
                                   nbins, key ? "key feeds" : nullptr, per_spectrum6, "per_spectrum6");
  if (rc != RDN_OK || n == 0) return rc;
  const rdn::phys::PhysOut po{per_spectrum6, key, (long long*)report,
                              report ? rdn::make_bins(lo, hi, nbins) : rdn::Bins{0.f, 0.f, 0.f, 0},
                              alpha, beta, gamma, nullptr, 0.0};
  return hip_check(rdn::launch_physics(x, y, clean, clean_is_f64 == 1, n, (int)L, po, (hipStream_t)stream), "physics");
  RDN_GUARD_END
}

int rdn_physics_grad(const float* x, const float* y, const void* clean, int clean_is_f64, int64_t n, int64_t L,
                     double alpha, double beta, double gamma, double scale, double* per_spectrum6, float* grad,
                     void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_physics_grad";
  if (n > 0 && !(y && clean && grad)) return fail(RDN_EINVAL, fn + ": null pointer");
  if (n > 0 && per_spectrum6 && !x) return fail(RDN_EINVAL, fn + ": per_spectrum6 needs x, which is NULL");
  if (clean_is_f64 != 0 && clean_is_f64 != 1) return fail(RDN_EINVAL, fn + ": clean_is_f64 must be 0 or 1");
  if (bad_rows(n, L, 3)) return fail(RDN_EINVAL, fn + ": need n >= 0 and 3 <= L < 2^31");
  if (!(std::isfinite(alpha) && std::isfinite(beta) && std::isfinite(gamma)))
    return fail(RDN_EINVAL, fn + ": the weights alpha, beta, gamma must be finite");
  if (!std::isfinite(scale)) return fail(RDN_EINVAL, fn + ": scale must be finite");
  if (n == 0) return RDN_OK;
  const size_t bytes = row_bytes(n, L);  // every position reads its neighbours while other lanes' gradients land
  if ((x && rdn::overlaps(x, bytes, grad, bytes)) || rdn::overlaps(y, bytes, grad, bytes) ||
      rdn::overlaps(clean, clean_is_f64 ? 2 * bytes : bytes, grad, bytes))
    return fail(RDN_EINVAL, fn + ": grad overlaps x, y or clean");
  const rdn::phys::PhysOut po{per_spectrum6, nullptr, nullptr, rdn::Bins{0.f, 0.f, 0.f, 0}, alpha, beta, gamma, grad, scale};
  return hip_check(rdn::launch_physics(per_spectrum6 ? x : nullptr, y, clean, clean_is_f64 == 1, n, (int)L, po,
                                       (hipStream_t)stream),
                   "physics_grad");
  RDN_GUARD_END
}

int rdn_physics_value(const int64_t* report, int nbins, double* out) {
  RDN_GUARD_BEGIN
  const int rc = check_report_value("rdn_physics_value", report, nbins, out);
  if (rc != RDN_OK) return rc;
  acc_rows_value(report, RDN_REPORT_ROWS(nbins), RDN_PHYS_ROW_WORDS, RDN_PHYS_QUANTITIES, 1, 1, true, out);
  return RDN_OK;
  RDN_GUARD_END
}

// The arguments rdn_fir and rdn_median share (taps_ok: rdn_fir's taps pointer is given).
static int check_filter_call(const std::string& fn, const float* x, const float* y, int64_t n, int64_t L, int w,
                             bool taps_ok) {
  if (!taps_ok || (n > 0 && !(x && y))) return fail(RDN_EINVAL, fn + ": null pointer");
  if (n < 0) return fail(RDN_EINVAL, fn + ": need n >= 0");
  if (w < 1 || w > RDN_FILTER_MAX_WINDOW || w % 2 == 0)
    return fail(RDN_EINVAL, fn + ": the window must be odd, 1 <= w <= " + std::to_string(RDN_FILTER_MAX_WINDOW));
  if (bad_rows(0, L, w)) return fail(RDN_EINVAL, fn + ": need w <= L < 2^31");
  // tiles re-read their neighbours' samples (the halo) while other tiles' outputs land in y
  if (rdn::overlaps(x, row_bytes(n, L), y, row_bytes(n, L))) return fail(RDN_EINVAL, fn + ": x and y overlap");
  return RDN_OK;
}

int rdn_fir(const float* x, float* y, int64_t n, int64_t L, const double* taps, int w, const double* edge_taps,
            void* stream) {
  RDN_GUARD_BEGIN
  const int rc = check_filter_call("rdn_fir", x, y, n, L, w, taps != nullptr);
  if (rc != RDN_OK || n == 0) return rc;
  return hip_check(rdn::launch_fir(x, y, n, (int)L, taps, w, edge_taps, (hipStream_t)stream), "fir");
  RDN_GUARD_END
}

int rdn_median(const float* x, float* y, int64_t n, int64_t L, int w, void* stream) {
  RDN_GUARD_BEGIN
  const int rc = check_filter_call("rdn_median", x, y, n, L, w, true);
  if (rc != RDN_OK || n == 0) return rc;
  return hip_check(rdn::launch_median(x, y, n, (int)L, w, (hipStream_t)stream), "median");
  RDN_GUARD_END
}

int rdn_haar_shrink(const float* x, float* y, double* med, int64_t n, int64_t L, int levels, const double* k, int mode,
                    void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_haar_shrink";
  if (!k || (n > 0 && !(x && y && med))) return fail(RDN_EINVAL, fn + ": null pointer");
  if (n < 0) return fail(RDN_EINVAL, fn + ": need n >= 0");
  if (levels < 1 || levels > RDN_HAAR_MAX_LEVELS)
    return fail(RDN_EINVAL, fn + ": need 1 <= levels <= " + std::to_string(RDN_HAAR_MAX_LEVELS));
  if (mode != RDN_HAAR_SOFT && mode != RDN_HAAR_HARD) return fail(RDN_EINVAL, fn + ": unknown mode " + std::to_string(mode));
  if (bad_rows(0, L, (int64_t)1 << levels)) return fail(RDN_EINVAL, fn + ": need 2^levels <= L < 2^31");
  rdn::haar::Factors f = {};
  for (int j = 0; j < levels; ++j) {
    if (!std::isfinite(k[j]) || k[j] < 0.0) return fail(RDN_EINVAL, fn + ": every k must be finite and >= 0");
    f.k[j] = k[j];
  }
  const size_t bytes = row_bytes(n, L), mbytes = (size_t)n * sizeof(double);
  // tiles re-read their neighbours' samples (the halo) while other tiles' outputs land in y
  if (rdn::overlaps(x, bytes, y, bytes)) return fail(RDN_EINVAL, fn + ": x and y overlap");
  // med is written by the select kernel while x is still to be read, and read while y is written
  if (rdn::overlaps(med, mbytes, x, bytes) || rdn::overlaps(med, mbytes, y, bytes))
    return fail(RDN_EINVAL, fn + ": med overlaps x or y");
  if (n == 0) return RDN_OK;
  return hip_check(rdn::launch_haar_shrink(x, y, med, n, (int)L, levels, f, mode, (hipStream_t)stream), "haar_shrink");
  RDN_GUARD_END
}

int rdn_noise_mad(const float* x, double* med, int64_t n, int64_t L, void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_noise_mad";
  if (n > 0 && !(x && med)) return fail(RDN_EINVAL, fn + ": null pointer");
  if (bad_rows(n, L, 1)) return fail(RDN_EINVAL, fn + ": need n >= 0 and 1 <= L < 2^31");
  // med is written while other spectra of x are still to be read
  if (rdn::overlaps(med, (size_t)n * sizeof(double), x, row_bytes(n, L))) return fail(RDN_EINVAL, fn + ": med overlaps x");
  if (n == 0) return RDN_OK;
  return hip_check(rdn::launch_noise_mad(x, med, n, (int)L, (hipStream_t)stream), "noise_mad");
  RDN_GUARD_END
}

int rdn_potts(const float* x, float* y, int32_t* nseg, const double* gamma, int64_t n, int64_t L, int max_len,
              uint8_t* work, size_t work_bytes, void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_potts";
  if (!gamma) return fail(RDN_EINVAL, fn + ": null gamma");
  if (n < 0) return fail(RDN_EINVAL, fn + ": need n >= 0");
  if (max_len < 1 || max_len > RDN_POTTS_MAX_LEN)
    return fail(RDN_EINVAL, fn + ": need 1 <= max_len <= " + std::to_string(RDN_POTTS_MAX_LEN));
  if (bad_rows(0, L, 1)) return fail(RDN_EINVAL, fn + ": need 1 <= L < 2^31");
  if (n == 0) return RDN_OK;
  if (!(x && y && work)) return fail(RDN_EINVAL, fn + ": null pointer");
  if ((uint64_t)n > (uint64_t)SIZE_MAX / (uint64_t)L / sizeof(float) || work_bytes < (size_t)n * (size_t)L)
    return fail(RDN_EINVAL, fn + ": work_bytes is below n * L");
  const size_t bytes = row_bytes(n, L), sbytes = (size_t)n * sizeof(int32_t);
  if (rdn::overlaps(x, bytes, y, bytes)) return fail(RDN_EINVAL, fn + ": x and y overlap");
  // the back-pointers land in work while x is still to be read, and are read while y is written
  if (rdn::overlaps(work, work_bytes, x, bytes) || rdn::overlaps(work, work_bytes, y, bytes))
    return fail(RDN_EINVAL, fn + ": work overlaps x or y");
  if (nseg && (rdn::overlaps(nseg, sbytes, x, bytes) || rdn::overlaps(nseg, sbytes, y, bytes) ||
               rdn::overlaps(nseg, sbytes, work, work_bytes)))
    return fail(RDN_EINVAL, fn + ": nseg overlaps x, y or work");
  return hip_check(rdn::launch_potts(x, y, nseg, gamma, n, (int)L, max_len, work, (hipStream_t)stream), "potts");
  RDN_GUARD_END
}

int rdn_bayes_steps(const float* x, float* y, float* jump, double* logz, const double* sigma, int64_t n, int64_t L,
                    int max_len, double level_range, double* work, size_t work_bytes, void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_bayes_steps";
  if (!sigma) return fail(RDN_EINVAL, fn + ": null sigma");
  if (n < 0) return fail(RDN_EINVAL, fn + ": need n >= 0");
  if (max_len < 1 || max_len > RDN_BAYES_MAX_LEN)
    return fail(RDN_EINVAL, fn + ": need 1 <= max_len <= " + std::to_string(RDN_BAYES_MAX_LEN));
  if (!std::isfinite(level_range) || level_range <= 0.0)
    return fail(RDN_EINVAL, fn + ": level_range must be finite and > 0");
  if (bad_rows(0, L, 1)) return fail(RDN_EINVAL, fn + ": need 1 <= L < 2^31");
  if (n == 0) return RDN_OK;
  if (!(x && y && work)) return fail(RDN_EINVAL, fn + ": null pointer");
  if ((uintptr_t)work % sizeof(double)) return fail(RDN_EINVAL, fn + ": work is not 8-byte aligned");
  if ((uint64_t)n > (uint64_t)SIZE_MAX / ((uint64_t)L + 1) / sizeof(double) ||
      work_bytes < (size_t)n * ((size_t)L + 1) * sizeof(double))
    return fail(RDN_EINVAL, fn + ": work_bytes is below n * (L + 1) * 8");
  const size_t bytes = row_bytes(n, L), zbytes = (size_t)n * sizeof(double);
  if (rdn::overlaps(x, bytes, y, bytes)) return fail(RDN_EINVAL, fn + ": x and y overlap");
  // G lands in work while x is still to be read, and is read while y and jump are written
  if (rdn::overlaps(work, work_bytes, x, bytes) || rdn::overlaps(work, work_bytes, y, bytes))
    return fail(RDN_EINVAL, fn + ": work overlaps x or y");
  if (jump && (rdn::overlaps(jump, bytes, x, bytes) || rdn::overlaps(jump, bytes, y, bytes) ||
               rdn::overlaps(jump, bytes, work, work_bytes)))
    return fail(RDN_EINVAL, fn + ": jump overlaps x, y or work");
  if (logz && (rdn::overlaps(logz, zbytes, x, bytes) || rdn::overlaps(logz, zbytes, y, bytes) ||
               rdn::overlaps(logz, zbytes, work, work_bytes) || (jump && rdn::overlaps(logz, zbytes, jump, bytes))))
    return fail(RDN_EINVAL, fn + ": logz overlaps x, y, work or jump");
  // a spectrum's sigma is read when its wave starts: after other spectra's outputs have landed
  if (rdn::overlaps(sigma, zbytes, y, bytes) || rdn::overlaps(sigma, zbytes, work, work_bytes) ||
      (jump && rdn::overlaps(sigma, zbytes, jump, bytes)) || (logz && rdn::overlaps(sigma, zbytes, logz, zbytes)))
    return fail(RDN_EINVAL, fn + ": sigma overlaps y, work, jump or logz");
  return hip_check(rdn::launch_bayes_steps(x, y, jump, logz, sigma, n, (int)L, max_len, level_range, work,
                                           (hipStream_t)stream), "bayes_steps");
  RDN_GUARD_END
}

int rdn_blind(const float* x, const float* y, const double* sigma, int64_t n, int64_t L, int lags, double q_crit,
              double* per_spectrum7, double* rho, const float* key, float lo, float hi, int nbins, int64_t* report,
              void* stream) {
  RDN_GUARD_BEGIN
  const std::string fn = "rdn_blind";
  if (!sigma) return fail(RDN_EINVAL, fn + ": null sigma");
  if (lags < 1 || lags > RDN_BLIND_MAX_LAGS)
    return fail(RDN_EINVAL, fn + ": need 1 <= lags <= " + std::to_string(RDN_BLIND_MAX_LAGS));
  if (bad_rows(n, L, (int64_t)lags + 1)) return fail(RDN_EINVAL, fn + ": need n >= 0 and lags < L < 2^31");
  if (!(q_crit >= 0.0)) return fail(RDN_EINVAL, fn + ": q_crit must be >= 0 (+inf flags nothing)");
  if (!per_spectrum7 && !rho && !report) return fail(RDN_EINVAL, fn + ": none of per_spectrum7, rho and report to write");
  if (report && !valid_bins(lo, hi, nbins)) return fail(RDN_EINVAL, fn + ": " + bins_msg());
  if (!report && key) return fail(RDN_EINVAL, fn + ": key feeds the report, which is NULL");
  if (n == 0) return RDN_OK;
  if (!(x && y)) return fail(RDN_EINVAL, fn + ": null pointer");
  if ((uint64_t)n > (uint64_t)SIZE_MAX / (uint64_t)L / sizeof(double))
    return fail(RDN_EINVAL, fn + ": n * L does not fit a size");
  // every input is read while other spectra's outputs land: no output may share a byte with an input or
  // with another output
  const size_t un = (size_t)n;
  const struct { const void* p; size_t bytes; } in[] = {{x, row_bytes(n, L)}, {y, row_bytes(n, L)},
                                                        {sigma, un * sizeof(double)}, {key, un * sizeof(float)}},
      out[] = {{per_spectrum7, un * RDN_BLIND_QUANTITIES * sizeof(double)}, {rho, un * (size_t)lags * sizeof(double)},
               {report, report ? (size_t)RDN_BLIND_WORDS(nbins) * sizeof(int64_t) : 0}};
  for (int o = 0; o < 3; ++o) {
    if (!out[o].p) continue;
    for (const auto& i : in)
      if (i.p && rdn::overlaps(out[o].p, out[o].bytes, i.p, i.bytes))
        return fail(RDN_EINVAL, fn + ": an output overlaps x, y, sigma or key");
    for (int q = o + 1; q < 3; ++q)
      if (out[q].p && rdn::overlaps(out[o].p, out[o].bytes, out[q].p, out[q].bytes))
        return fail(RDN_EINVAL, fn + ": per_spectrum7, rho and report overlap");
  }
  const rdn::blind::BlindOut bo{per_spectrum7, rho, key, (long long*)report,
                                report ? rdn::make_bins(lo, hi, nbins) : rdn::Bins{0.f, 0.f, 0.f, 0}, q_crit, lags};
  return hip_check(rdn::launch_blind(x, y, sigma, n, (int)L, bo, (hipStream_t)stream), "blind");
  RDN_GUARD_END
}

int rdn_blind_value(const int64_t* report, int nbins, double* out) {
  RDN_GUARD_BEGIN
  const int rc = check_report_value("rdn_blind_value", report, nbins, out);
  if (rc != RDN_OK) return rc;
  acc_rows_value(report, RDN_REPORT_ROWS(nbins), RDN_BLIND_ROW_WORDS, RDN_BLIND_QUANTITIES, 2, 1, true, out);
  return RDN_OK;
  RDN_GUARD_END
}

}  // extern "C"
