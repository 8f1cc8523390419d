// SNR report on the device: one 512-thread workgroup per spectrum makes one pass over the noisy input
// x, the denoised y and clean, in fp64 (definitions, report layout and bin formula:
// include/raman_mi355x.h rdn_snr; report.hpp).  The reduction and the exact integer accumulators are the
// metrics kernel's (metrics.hpp block_reduce / acc_add): a report's words are the same bits whatever the
// batch split, the atomics' order or the number of ranks whose reports are summed.
//
// Reference: 数据集产生.py:43-45 (P = mean(clean^2) is the power the simulator scales its noise by); the
// reference's evaulate.py has no SNR, its datasets carry the nominal one (`snrs`, 数据集产生.py:78).
//
// Rows are addressed as pointer + 64-bit offset (no buffer descriptor), so any L < 2^31 runs.
#include "host_util.hpp"
#include "metrics.hpp"
#include "snr.hpp"

namespace rdn {
namespace snr {

using met::MET_THREADS;

template <typename TC>
__global__ __launch_bounds__(MET_THREADS) void snr_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const TC* __restrict__ clean, int L, SnrOut so) {
  __shared__ double red[MET_THREADS / 64];
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int64_t n = __builtin_amdgcn_workgroup_id_x();
  const float* xx = x + (size_t)n * L;
  const float* yy = y + (size_t)n * L;
  const TC* cc = clean + (size_t)n * L;
  const auto add = [](double a, double b) { return a + b; };

  double sp = 0.0, si = 0.0, sn = 0.0;
#pragma unroll 4
  for (int64_t p = tid; p < L; p += MET_THREADS) {
    const double c = cc[p], a = xx[p], b = yy[p];
    sp += c * c;
    si += (a - c) * (a - c);
    sn += (b - c) * (b - c);
  }
  sp = met::block_reduce(sp, red, add);
  si = met::block_reduce(si, red, add);
  sn = met::block_reduce(sn, red, add);

  const double P = sp / L, Ni = si / L, No = sn / L;
  const double s_in = 10.0 * log10(P / Ni), s_out = 10.0 * log10(P / No), gain = s_out - s_in;
  if (tid == 0 && so.per3) {
    so.per3[n * 3 + 0] = s_in;
    so.per3[n * 3 + 1] = s_out;
    so.per3[n * 3 + 2] = gain;
  }
  if (!so.report) return;

  const float k = so.key ? so.key[n] : (float)s_in;
  long long* row = so.report + (size_t)bin_row(k, so.bins) * RDN_REPORT_ROW_WORDS;
  // lanes 0..6 of wave 0 each own one quantity (integer atomics: order-free)
  if (tid < RDN_REPORT_QUANTITIES && (tid >= 4 || so.per4)) {
    const double v = tid < 4 ? so.per4[n * 4 + tid] : tid == 4 ? s_in : tid == 5 ? s_out : gain;
    met::acc_add(row, tid, v);
  }
  if (tid == 0) {
    atomicAdd((unsigned long long*)&row[RDN_REPORT_COUNT], 1ull);
    if (so.per4) atomicAdd((unsigned long long*)&row[RDN_REPORT_COUNT4], 1ull);
  }
}

}  // namespace snr

hipError_t launch_snr(const float* x, const float* y, const void* clean, bool clean_f64, int64_t n, int L,
                      const snr::SnrOut& so, hipStream_t stream) {
  return with_clean(clean, clean_f64, [&](auto* cc) {
    return launch_chunks(n, [&](int64_t n0, int64_t nn) {
      const snr::SnrOut c{so.per3 ? so.per3 + n0 * 3 : nullptr, so.key ? so.key + n0 : nullptr,
                          so.per4 ? so.per4 + n0 * 4 : nullptr, so.report, so.bins};
      hipLaunchKernelGGL(snr::snr_kernel, dim3((unsigned)nn), dim3(met::MET_THREADS), 0, stream, x + n0 * L,
                         y + n0 * L, cc + n0 * L, L, c);
    });
  });
}

}  // namespace rdn
