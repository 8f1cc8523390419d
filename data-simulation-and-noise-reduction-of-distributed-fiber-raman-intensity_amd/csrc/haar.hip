// Translation-invariant Haar shrinkage on the device: the undecimated Haar transform of each spectrum, its
// detail planes thresholded in units of the spectrum's own median |d_1|, and the inverse transform.
// The arithmetic contract is in include/raman_mi355x.h (rdn_haar_shrink); this file is compiled with
// -ffp-contract=off so that each operation of the recurrence is rounded on its own.
//
// Two kernels per call, in stream order.
//
// select_kernel, one 256-thread workgroup per spectrum: m = median |d_1|.  |d_1[i]| is a non-negative fp64,
// so its bits order as a uint64; it is formed on the fly from the row (staged in LDS up to
// RDN_HAAR_SELECT_LDS_L samples, re-read through L2 beyond) and the middle rank is found by a radix select,
// one byte of the key per pass from the top: a 256-bin histogram in LDS of the keys that share the prefix
// found so far, a scan, the bin that holds the rank.  For an even L the upper middle rank is the lower one's
// key again, or the smallest key above it: one more pass.  A lane's increment goes through the wave first
// (the lanes that share the first pending lane's digit add once, twice over), since the top bytes of a
// spectrum's keys are nearly all equal.  A row with a NaN or an infinity is flagged while it is staged and
// gets NaN.
//
// shrink_kernel, one 256-thread workgroup per (spectrum, tile of RDN_HAAR_TILE outputs): the tile and a halo
// of H = 2^J - 1 samples on each side are staged as fp64 with periodic indexing; level j of the analysis
// reads plane a_{j-1} and writes a_j (two ping-pong planes) and the thresholded details e_j (a plane per
// level); the synthesis walks back through the e planes.  Staged position s holds a_j from s >= 2^j - 1 on
// and b_j up to s < C - (2^J - 2^j), so the outputs s in [H, H + TILE) are whole.  Consecutive lanes touch
// consecutive doubles: conflict-free 8-byte LDS accesses.  A spectrum whose m is NaN is written as quiet NaNs.
//
// Rows are addressed as pointer + 64-bit offset, so any L < 2^31 runs; a spectrum's output depends on its own
// samples only, not on n, its row index, the tiling or the launches a huge n is split into.
#include "haar.hpp"
#include "host_util.hpp"

namespace rdn {
namespace haar {

__device__ inline int lane_id() { return __builtin_amdgcn_workitem_id_x(); }

constexpr uint32_t QUIET_NAN = 0x7fc00000u;
constexpr unsigned long long QUIET_NAN64 = 0x7ff8000000000000ull;

// hist[digit] += 1 for every lane with `pending`.  Called by whole waves.
__device__ inline void count_digit(uint32_t* hist, bool pending, uint32_t digit) {
  const int lane = lane_id() & 63;
  for (int r = 0; r < 2; ++r) {
    const unsigned long long act = __ballot(pending);
    if (!act) return;
    const int leader = __ffsll(act) - 1;
    const uint32_t dg = __shfl(digit, leader);
    const bool same = pending && digit == dg;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[dg], (uint32_t)__popcll(m));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&hist[digit], 1u);
}

template <bool IN_LDS>
__global__ __launch_bounds__(THREADS) void select_kernel(const float* __restrict__ x, double* __restrict__ med, int L) {
  __shared__ float row[IN_LDS ? SELECT_LDS_L : 1];
  __shared__ uint32_t hist[256];
  __shared__ uint32_t wave_sum[THREADS / 64];
  __shared__ uint32_t pick[2];                 // the digit that holds the rank, the rank within it
  __shared__ uint32_t bad, upto;               // a non-finite sample; #(keys <= lo)
  __shared__ unsigned long long above;         // the smallest key > lo
  static_assert(THREADS == 256, "one thread per bin");
  const int tid = lane_id();
  const int64_t r = __builtin_amdgcn_workgroup_id_x();
  const float* xr = x + r * L;

  if (tid == 0) bad = 0;
  __syncthreads();
  bool nonfinite = false;
  for (int64_t i = tid; i < L; i += THREADS) {
    const float v = xr[i];
    nonfinite |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    if (IN_LDS) row[i] = v;
  }
  if (nonfinite) atomicOr(&bad, 1u);
  __syncthreads();
  if (bad) {
    if (tid == 0) med[r] = __longlong_as_double((long long)QUIET_NAN64);
    return;
  }

  const auto at = [&](int64_t i) { return IN_LDS ? row[i] : xr[i]; };
  // the bits of |d_1[i]| = |0.5 * (x[i] - x[idx(i - 1)])|
  const auto key = [&](int64_t i) {
    const double p = (double)at(i), q = (double)at(i == 0 ? L - 1 : i - 1);
    const double d = 0.5 * (p - q);
    return (unsigned long long)__double_as_longlong(fabs(d));
  };

  const uint32_t mid = (uint32_t)((L - 1) / 2);   // the median's rank, or the lower of its two
  unsigned long long prefix = 0;
  uint32_t rank = mid;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < L; i0 += THREADS) {
      const int64_t i = i0 + tid;
      bool match = false;
      uint32_t digit = 0;
      if (i < L) {
        const unsigned long long k = key(i);
        match = ((k >> shift) >> 8) == prefix;
        digit = (uint32_t)(k >> shift) & 255u;
      }
      count_digit(hist, match, digit);
    }
    __syncthreads();
    const uint32_t c = hist[tid];
    uint32_t inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o);
      if ((tid & 63) >= o) inc += v;
    }
    if ((tid & 63) == 63) wave_sum[tid >> 6] = inc;
    __syncthreads();
    for (int w = 0; w < (tid >> 6); ++w) inc += wave_sum[w];
    const uint32_t exc = inc - c;
    if (exc <= rank && rank < inc) {
      pick[0] = (uint32_t)tid;
      pick[1] = rank - exc;
    }
    __syncthreads();
    prefix = (prefix << 8) | pick[0];
    rank = pick[1];
  }

  const unsigned long long lo = prefix;
  if (L & 1) {
    if (tid == 0) med[r] = __longlong_as_double((long long)lo);
    return;
  }
  if (tid == 0) {
    upto = 0;
    above = ~0ull;
  }
  __syncthreads();
  uint32_t cnt = 0;
  unsigned long long mn = ~0ull;
  for (int64_t i = tid; i < L; i += THREADS) {
    const unsigned long long k = key(i);
    if (k <= lo) ++cnt;
    else if (k < mn) mn = k;
  }
  atomicAdd(&upto, cnt);
  atomicMin(&above, mn);
  __syncthreads();
  if (tid == 0) {
    const unsigned long long hi = upto >= mid + 2 ? lo : above;
    med[r] = 0.5 * (__longlong_as_double((long long)lo) + __longlong_as_double((long long)hi));
  }
}

template <int MODE>
__device__ inline double shrink(double d, double t) {
  if (MODE == RDN_HAAR_HARD) return fabs(d) > t ? d : 0.0;
  return d > t ? d - t : (d < -t ? d + t : 0.0);
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void shrink_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const double* __restrict__ med, int L, int tiles, int J,
                                                         Factors k) {
  extern __shared__ double planes[];           // a / b ping, a / b pong, e_1 .. e_J: C doubles each
  __shared__ double ts[MAX_LEVELS];
  const unsigned blk = __builtin_amdgcn_workgroup_id_x();
  const int64_t rowi = blk / (unsigned)tiles, t0 = (int64_t)(blk % (unsigned)tiles) * TILE;
  const float* xr = x + rowi * L;
  float* yr = y + rowi * L;
  const int tid = lane_id(), H = (1 << J) - 1, C = TILE + 2 * H;

  const double m = med[rowi];
  if (__builtin_isnan(m)) {                    // a NaN or an infinity in the row
    for (int o = tid; o < TILE; o += THREADS)
      if (t0 + o < L) yr[t0 + o] = __uint_as_float(QUIET_NAN);
    return;
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < MAX_LEVELS; ++j) ts[j] = k.k[j] * m;
  }

  double* in = planes;
  double* out = planes + C;
  double* const e = planes + 2 * C;
  // in[s] = x[idx(t0 - H + s)]
  if (t0 >= H && t0 + TILE + H <= L) {         // an interior tile: every staged sample exists where it stands
    const float* p = xr + (t0 - H);
    for (int s = tid; s < C; s += THREADS) in[s] = (double)p[s];
  } else {
    const uint32_t base = (uint32_t)(((t0 - H) % L + L) % L);
    for (int s = tid; s < C; s += THREADS) in[s] = (double)xr[(base + (uint32_t)s) % (uint32_t)L];
  }
  __syncthreads();

  for (int j = 1; j <= J; ++j) {               // a_{j-1} in `in` from staged position 2^(j-1) - 1 on
    const int s = 1 << (j - 1);
    const double t = ts[j - 1];
    double* ej = e + (j - 1) * C;
    for (int i = 2 * s - 1 + tid; i < C; i += THREADS) {
      const double p = in[i], q = in[i - s];
      out[i] = 0.5 * (p + q);
      ej[i] = shrink<MODE>(0.5 * (p - q), t);
    }
    __syncthreads();
    double* const tmp = in;
    in = out;
    out = tmp;
  }
  int upper = C;                               // b_j in `in` on [H, upper)
  for (int j = J; j >= 1; --j) {
    const int s = 1 << (j - 1);
    const double* ej = e + (j - 1) * C;
    upper -= s;
    for (int i = H + tid; i < upper; i += THREADS) out[i] = 0.5 * ((in[i] + ej[i]) + (in[i + s] - ej[i + s]));
    __syncthreads();
    double* const tmp = in;
    in = out;
    out = tmp;
  }
  for (int o = tid; o < TILE; o += THREADS)
    if (t0 + o < L) yr[t0 + o] = (float)in[H + o];
}

}  // namespace haar

hipError_t launch_haar_shrink(const float* x, float* y, double* med, int64_t n, int L, int levels,
                              const haar::Factors& k, int mode, hipStream_t stream) {
  const int tiles = (int)tiles_of(L, haar::TILE);
  const size_t lds = (size_t)haar::shrink_lds_bytes(levels);
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    const dim3 block(haar::THREADS), rows((unsigned)nn), grid((unsigned)(nn * tiles));
    const float* xx = x + n0 * L;
    float* yy = y + n0 * L;
    double* mm = med + n0;
    if (L <= haar::SELECT_LDS_L) hipLaunchKernelGGL(haar::select_kernel<true>, rows, block, 0, stream, xx, mm, L);
    else hipLaunchKernelGGL(haar::select_kernel<false>, rows, block, 0, stream, xx, mm, L);
    if (mode == RDN_HAAR_HARD)
      hipLaunchKernelGGL(haar::shrink_kernel<RDN_HAAR_HARD>, grid, block, lds, stream, xx, yy, mm, L, tiles, levels, k);
    else
      hipLaunchKernelGGL(haar::shrink_kernel<RDN_HAAR_SOFT>, grid, block, lds, stream, xx, yy, mm, L, tiles, levels, k);
  }, tiles_chunk(tiles));
}

// m alone (rdn_noise_mad): the select kernel of launch_haar_shrink, launched the same way
hipError_t launch_noise_mad(const float* x, double* med, int64_t n, int L, hipStream_t stream) {
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    const dim3 block(haar::THREADS), rows((unsigned)nn);
    if (L <= haar::SELECT_LDS_L) hipLaunchKernelGGL(haar::select_kernel<true>, rows, block, 0, stream, x + n0 * L, med + n0, L);
    else hipLaunchKernelGGL(haar::select_kernel<false>, rows, block, 0, stream, x + n0 * L, med + n0, L);
  });
}

}  // namespace rdn
