// Blind residual report on the device: what can be said about a denoised spectrum y from the noisy input x
// and a noise level sigma alone, with no clean reference.  One 512-thread workgroup per spectrum, fp64
// throughout (definitions, report layout: include/raman_mi355x.h rdn_blind; bin formula: report.hpp).
//
//   pass 1  reads x and y once (position p to thread p mod 512: coalesced), forms r = x - y and the sums
//           of r, r^2 and x^2, and -- for L <= RDN_BLIND_LDS_L -- stages r in LDS as fp64;
//   pass 2  gives thread t the C consecutive positions from t * C, C = ceil(L / 512) made odd (lane stride
//           of 2 C dwords: the 32 lanes of a ds_read_b64 group fall on 64 different banks).  The thread
//           keeps d_i .. d_{i+KT} (d = r - Mean) in a register window that slides one position per step, so
//           it reads C + KT staged values for its C positions and not C * (K + 1); the window is rotated
//           by unrolling KT + 1 steps, never by moving registers.  The last KT positions of a row, whose
//           lags run off its end, read their (bounded) partners directly.  Longer spectra recompute r
//           from x and y (through L2) in the same loops: the same numbers in the same order.
//
// The reduction and the exact integer accumulators are the metrics kernel's (metrics.hpp block_reduce /
// acc_add): no floating-point atomics, a spectrum's values depend on its own samples, sigma and K only,
// and a report's words are the same bits whatever the batch split or the atomics' order.  The kernel is
// instantiated for KT = 4, 16 and 32 lags and runs the smallest KT >= K: lag k's sum is formed the same
// way in each (the lags above K are computed and dropped).
//
// Built with -ffp-contract=off: every product and sum of the contract is rounded on its own.
// Rows are addressed as pointer + 64-bit offset (no buffer descriptor), so any L < 2^31 runs.
#include "blind.hpp"
#include "host_util.hpp"
#include "metrics.hpp"

namespace rdn {
namespace blind {

using met::MET_THREADS;

// acc[k] += sum over this thread's positions i of d_i * d_{i+k}, k = 0 .. KT, i + k < L; d(p) = r_p - Mean.
// Positions whose KT lags all exist (i + KT < L) go through the sliding window; the row's last KT positions
// follow, in the same ascending order, each lag product bounded by i + k < L.
template <int KT, class D>
__device__ __forceinline__ void lag_sums(D d, int64_t L, double (&acc)[KT + 1]) {
  constexpr int W = KT + 1;
  const int64_t C = ((L + MET_THREADS - 1) / MET_THREADS) | 1;
  const int64_t i0 = (int64_t)__builtin_amdgcn_workitem_id_x() * C;
  if (i0 >= L) return;
  const int64_t i1 = i0 + C < L ? i0 + C : L;
  const int64_t e1 = i1 < L - KT ? i1 : L - KT;    // end of the window's positions (may lie below i0)
  if (i0 < e1) {
    double w[W];                                   // at step s of a round: w[(s + k) % W] = d_{i+k}
#pragma unroll
    for (int j = 0; j < W; ++j) w[j] = d(i0 + j);  // i0 + KT < L
    for (int64_t ib = i0; ib < e1; ib += W) {
#pragma unroll
      for (int s = 0; s < W; ++s) {
        const int64_t i = ib + s;
        if (i < e1) {
          const double c = w[s];
          acc[0] += c * c;
#pragma unroll
          for (int k = 1; k <= KT; ++k) acc[k] += c * w[(s + k) % W];
          if (i + 1 < e1) w[s] = d(i + W);         // d_{(i+1)+KT}, the next step's last lag: (i + 1) + KT < L
        }
      }
    }
  }
  for (int64_t i = i0 > e1 ? i0 : e1; i < i1; ++i) {
    const double c = d(i);
    acc[0] += c * c;
#pragma unroll
    for (int k = 1; k <= KT; ++k)
      if (i + k < L) acc[k] += c * d(i + k);
  }
}

// lds_bytes: the dynamic LDS of this launch (the residual is staged iff its 8 L bytes fit into it)
template <int KT>
__global__ __launch_bounds__(MET_THREADS) void blind_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const double* __restrict__ sigma, int L, unsigned lds_bytes,
                                                            BlindOut bo) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ double red[MET_THREADS / 64];
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int64_t n = __builtin_amdgcn_workgroup_id_x();
  const float* xx = x + (size_t)n * L;
  const float* yy = y + (size_t)n * L;
  const auto add = [](double a, double b) { return a + b; };
  const bool staged = (size_t)L * sizeof(double) <= (size_t)lds_bytes;
  double* rs = (double*)lds;
  const int K = bo.lags;

  double sr = 0.0, sr2 = 0.0, sa2 = 0.0;
#pragma unroll 4
  for (int64_t p = tid; p < L; p += MET_THREADS) {
    const double a = xx[p], b = yy[p];
    const double r = a - b;
    if (staged) rs[p] = r;
    sr += r;
    sr2 += r * r;
    sa2 += a * a;
  }
  sr = met::block_reduce(sr, red, add);            // its barriers also publish the staged residual
  sr2 = met::block_reduce(sr2, red, add);
  sa2 = met::block_reduce(sa2, red, add);

  const double Ld = (double)L;
  const double mean = sr / Ld;
  double acc[KT + 1];
#pragma unroll
  for (int k = 0; k <= KT; ++k) acc[k] = 0.0;
  if (staged) lag_sums<KT>([&](int64_t p) { return rs[p] - mean; }, L, acc);
  else lag_sums<KT>([&](int64_t p) { return ((double)xx[p] - (double)yy[p]) - mean; }, L, acc);
#pragma unroll
  for (int k = 0; k <= KT; ++k)
    if (k <= K) acc[k] = met::block_reduce(acc[k], red, add);

  const double D = acc[0];
  double qs = 0.0, rmax = 0.0;
  bool rnan = false;
#pragma unroll
  for (int k = 1; k <= KT; ++k) {
    if (k <= K) {
      const double rho = acc[k] / D;
      acc[k] = rho;
      rnan |= met::nan_bits(rho);
      rmax = fmax(rmax, fabs(rho));
      qs += (rho * rho) / (double)(L - k);
    }
  }
  const double sg = sigma[n], s2 = sg * sg, S = sa2 / Ld;
  const double rms = sqrt(sr2 / Ld);
  const double Q = (Ld * (double)((int64_t)L + 2)) * qs;
  const double snr_est = 10.0 * log10((S - s2) / s2);
  const double v7[RDN_BLIND_QUANTITIES] = {
      mean, rms, rms / sg, acc[1], __longlong_as_double(rnan ? met::QNAN_BITS : __double_as_longlong(rmax)), Q, snr_est};
  const bool flagged = Q > bo.q_crit;              // false for a NaN Q

  if (tid == 0) {
    if (bo.per7) {
#pragma unroll
      for (int q = 0; q < RDN_BLIND_QUANTITIES; ++q) bo.per7[n * RDN_BLIND_QUANTITIES + q] = v7[q];
    }
    if (bo.rho) {
#pragma unroll
      for (int k = 1; k <= KT; ++k)
        if (k <= K) bo.rho[n * K + (k - 1)] = acc[k];
    }
  }
  if (!bo.report) return;

  const float key = bo.key ? bo.key[n] : (float)snr_est;
  long long* row = bo.report + (size_t)bin_row(key, bo.bins) * RDN_BLIND_ROW_WORDS;
  // lanes 0..6 of wave 0 each own one quantity (integer atomics: order-free)
  if (tid < RDN_BLIND_QUANTITIES) {
    double v = v7[0];
#pragma unroll
    for (int q = 1; q < RDN_BLIND_QUANTITIES; ++q) v = tid == q ? v7[q] : v;
    met::acc_add(row, tid, v);
  }
  if (tid == 0) {
    atomicAdd((unsigned long long*)&row[RDN_BLIND_COUNT], 1ull);
    if (flagged) atomicAdd((unsigned long long*)&row[RDN_BLIND_FLAGGED], 1ull);
  }
}

}  // namespace blind

hipError_t launch_blind(const float* x, const float* y, const double* sigma, int64_t n, int L,
                        const blind::BlindOut& bo, hipStream_t stream) {
  using kernel_t = void (*)(const float*, const float*, const double*, int, unsigned, blind::BlindOut);
  const kernel_t k = bo.lags <= 4 ? blind::blind_kernel<4> : bo.lags <= 16 ? blind::blind_kernel<16> : blind::blind_kernel<32>;
  // the launch's dynamic LDS: the whole residual (8 L bytes, rounded up to 16) or none; the kernel stages by
  // this number, not by a limit of its own
  const unsigned lds_bytes = L <= blind::LDS_L ? ((unsigned)L * 8u + 15u) & ~15u : 0u;
  if (lds_bytes) {
    const hipError_t e = ensure_dynamic_lds((const void*)k, (int)blind::LDS_MAX_BYTES, stream_device(stream));
    if (e != hipSuccess) return e;
  }
  const int K = bo.lags;
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    blind::BlindOut c = bo;
    c.per7 = bo.per7 ? bo.per7 + n0 * RDN_BLIND_QUANTITIES : nullptr;
    c.rho = bo.rho ? bo.rho + n0 * K : nullptr;
    c.key = bo.key ? bo.key + n0 : nullptr;
    hipLaunchKernelGGL(k, dim3((unsigned)nn), dim3(met::MET_THREADS), lds_bytes, stream, x + n0 * L, y + n0 * L,
                       sigma + n0, L, lds_bytes, c);
  });
}

}  // namespace rdn
