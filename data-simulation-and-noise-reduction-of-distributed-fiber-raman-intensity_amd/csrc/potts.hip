// The exact piecewise-constant (Potts) fit on the device: per spectrum the segmentation with parts of at most K
// samples and the per-segment means that minimise  sum (x - fit)^2 + g * #segments,  by dynamic programming.
// The arithmetic contract is in include/raman_mi355x.h (rdn_potts); this file is compiled with
// -ffp-contract=off so that each operation of the recurrence is rounded on its own.
//
// One kernel, 256-thread workgroups of four independent waves, one spectrum per wave, no LDS and no barrier.
// Three passes over the spectrum, all in the wave's own program order:
//
// 1. The recurrence.  Lane j keeps (S1, S2, B + g) of the latest position l = j (mod 64), so at position r the
//    64 lanes hold the 64 candidates l = r - 64 .. r - 1 without any cross-lane move: lane j's candidate has
//    len = ((r - 1 - j) & 63) + 1, and after the step lane r & 63 -- whose candidate was len = 64 -- takes
//    position r.  Every lane forms S1[r], S2[r] redundantly from the sample, which a 64-sample register chunk
//    hands out by v_readlane: the sequential sums are the contract's.  B[r] is a 6-step butterfly minimum of
//    the fp64 costs; the candidates that attain it are a ballot, rotated so that len = 1 is the top bit, and
//    the count of leading zeros is the smallest such len.  The back-pointers of a chunk gather in lane order
//    and leave as one 64-byte store into `work`.
// 2. Backtracking, wave-uniform: a 64-byte window of back-pointers below r is loaded once and walked with
//    v_readlane; the lanes whose position ends a segment set bit 7 of their byte.
// 3. The means.  S1 is summed again in the same order (nothing of it was kept: `work` is a byte per position);
//    where a byte is marked, the lanes < len store (float)((S1[r] - S1[r - len]) / len) in one vector store.
//
// Rows are addressed as pointer + 64-bit offset; a spectrum's output depends on its own samples and its own g
// only.
#include "potts.hpp"
#include "host_util.hpp"

namespace rdn {
namespace potts {

constexpr uint32_t QUIET_NAN = 0x7fc00000u;

__device__ inline double wave_min(double c) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double v = __shfl_xor(c, o);
    c = v < c ? v : c;
  }
  return c;
}

// lane t's value of a 32-bit register, t wave-uniform
__device__ inline int pick(int v, int t) { return __builtin_amdgcn_readlane(v, t); }
__device__ inline double pick_sample(float v, int t) { return (double)__int_as_float(pick(__float_as_int(v), t)); }

__global__ __launch_bounds__(THREADS) void potts_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        int32_t* __restrict__ nseg, const double* __restrict__ gamma,
                                                        int64_t n, int L, int K, uint8_t* work) {
  const int lane = (int)__builtin_amdgcn_workitem_id_x() & 63;
  const int64_t row = (int64_t)__builtin_amdgcn_workgroup_id_x() * WAVES + ((int)__builtin_amdgcn_workitem_id_x() >> 6);
  if (row >= n) return;
  const float* xr = x + row * L;
  float* yr = y + row * L;
  uint8_t* wr = work + row * L;

  const double g = gamma[row];
  bool bad = !(g >= 0.0) || __builtin_isinf(g);          // negative, NaN or infinite
  if (!bad) {
    double s1 = 0.0, s2 = 0.0;                           // S1[r], S2[r]: the same in every lane
    double S1 = 0.0, S2 = 0.0, Bg = 0.0 + g;             // of this lane's position; lane 0 starts at position 0
    for (int64_t base = 0; base < L; base += 64) {
      const int cnt = (int)(L - base < 64 ? L - base : 64);
      float xv = 0.f;
      if (lane < cnt) xv = xr[base + lane];
      bad |= (__float_as_uint(xv) & 0x7f800000u) == 0x7f800000u;
      int mine = 0;                                      // A[base + lane + 1]
      for (int t = 0; t < cnt; ++t) {                    // r = base + t + 1
        const double v = pick_sample(xv, t);
        s1 = s1 + v;
        s2 = s2 + v * v;
        const int len = ((t - lane) & 63) + 1;
        const double d1 = s1 - S1, d2 = s2 - S2;
        const double sse = d2 - (d1 * d1) / (double)len;
        double c = Bg + sse;
        if (len > K || len > base + t + 1) c = __builtin_huge_val();
        const double m = wave_min(c);
        const unsigned long long hit = __ballot(c == m);
        const int s = 63 - t;                            // lane t holds len = 1: to the top bit
        const unsigned long long rot = s ? (hit << s) | (hit >> (64 - s)) : hit;
        const int best = rot ? __clzll((long long)rot) + 1 : 1;
        if (lane == t) mine = best;
        if (lane == ((t + 1) & 63)) {
          S1 = s1;
          S2 = s2;
          Bg = m + g;
        }
      }
      if (lane < cnt) wr[base + lane] = (uint8_t)mine;
    }
    bad = __ballot(bad) != 0;
  }
  if (bad) {
    for (int64_t i = lane; i < L; i += 64) yr[i] = __uint_as_float(QUIET_NAN);
    if (nseg && lane == 0) nseg[row] = 0;
    return;
  }

  __threadfence();                                       // the back-pointers are read by other lanes than wrote them
  int segs = 0;
  for (int64_t r = L; r > 0;) {                          // lane j looks at position r - j
    const int lim = (int)(r < 64 ? r : 64);
    int b = 0;
    if (lane < lim) b = wr[r - 1 - lane];
    bool ends = false;
    int off = 0;
    while (off < lim) {
      ends |= lane == off;
      const int len = pick(b, off);
      off += len > 0 ? len : 1;                          // a back-pointer is never 0: the walk ends whatever it reads
      ++segs;
    }
    if (ends) wr[r - 1 - lane] = (uint8_t)(b | 0x80);
    r -= off;
  }
  if (nseg && lane == 0) nseg[row] = segs;

  __threadfence();
  double s1 = 0.0, s0 = 0.0;                             // S1[r], S1[start]
  int64_t start = 0;
  for (int64_t base = 0; base < L; base += 64) {
    const int cnt = (int)(L - base < 64 ? L - base : 64);
    float xv = 0.f;
    int b = 0;
    if (lane < cnt) {
      xv = xr[base + lane];
      b = wr[base + lane];
    }
    const unsigned long long ends = __ballot((b & 0x80) != 0);
    for (int t = 0; t < cnt; ++t) {
      s1 = s1 + pick_sample(xv, t);
      if ((ends >> t) & 1) {
        const int len = pick(b, t) & 0x7f;
        const double mean = (s1 - s0) / (double)len;
        if (lane < len && start + lane < L) yr[start + lane] = (float)mean;
        s0 = s1;
        start = base + t + 1;
      }
    }
  }
}

}  // namespace potts

hipError_t launch_potts(const float* x, float* y, int32_t* nseg, const double* gamma, int64_t n, int L, int max_len,
                        uint8_t* work, hipStream_t stream) {
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    const dim3 block(potts::THREADS), grid((unsigned)((nn + potts::WAVES - 1) / potts::WAVES));
    hipLaunchKernelGGL(potts::potts_kernel, grid, block, 0, stream, x + n0 * L, y + n0 * L, nseg ? nseg + n0 : nullptr,
                       gamma + n0, nn, L, max_len, work + n0 * L);
  }, (int64_t)0x7fffffff * potts::WAVES);
}

}  // namespace rdn
