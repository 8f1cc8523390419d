// The Bayesian change-point smoother on the device: per spectrum the posterior mean under the simulator's signal
// model (runs of 1 .. K equal samples, flat level prior, white noise of known sigma), the posterior probability of
// a run start at every sample and the log evidence, by a forward-backward recursion over the run boundaries.
// The arithmetic contract is in include/raman_mi355x.h (rdn_bayes_steps); this file is compiled with
// -ffp-contract=off so that each operation of the recursion is rounded on its own.
//
// One kernel, potts.hip's layout: 256-thread workgroups of four independent waves, one spectrum per wave, no LDS
// and no barrier.  Lane j owns the boundary b = j (mod 64), so at every step the 64 lanes hold the 64 candidate
// runs that end (sweep 1: start) at the step's sample without any cross-lane move; the lane whose candidate has
// reached 64 samples takes the step's new boundary.  A lane carries the Welford (mean, M2) of its own candidate,
// started at the run's first sample in the sweep's direction; its run length n = 1 .. 64 follows from the lane and
// the step, and 1 / n and log(n) / 2 travel with it: one value per lane, rotated by a lane each step.  Samples
// arrive as one coalesced 64-sample register chunk handed out by v_readlane.
//
// 1. Right to left: G[s] = LSE_n (G[s + n] + log w(s, s + n)): a butterfly maximum, one exp per lane, a butterfly
//    sum, one log.  The G of a chunk gather in lane order and leave as one 512-byte store into `work`.
// 2. Left to right: F[t] by the same step.  The LSE's terms e_j = exp(a_j - M) are the run posteriors up to the
//    wave-uniform factor c = exp(M + G[t] - logZ), one more exp per step; jump[t] = (sum e) * c.  Sample i gets,
//    from the runs that end at t, the sum of P * mean over the candidates that start at or before i: an
//    inclusive scan over the lanes in start order, a circular order that begins one lane further each step.  The
//    lane that owns boundary i owns sample i and adds its scan value to a register for the 64 steps it keeps the
//    boundary; when it takes its next boundary the sum is complete, and a chunk's 64 results leave in one store.
//
// Rows are addressed as pointer + 64-bit offset; a spectrum's output depends on its own samples and sigma only.
#include "bayes.hpp"
#include "host_util.hpp"

namespace rdn {
namespace bayes {

constexpr uint32_t QUIET_NAN = 0x7fc00000u;
constexpr double SQRT_2PI = 2.5066282746310002;

__device__ inline double wave_max(double c) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double v = __shfl_xor(c, o);
    c = v > c ? v : c;
  }
  return c;
}

// every lane adds the same pairs at every level: the total has the same bits in all of them
__device__ inline double wave_sum(double c) {
#pragma unroll
  for (int o = 32; o; o >>= 1) c = c + __shfl_xor(c, o);
  return c;
}

// lane t's value of a register, t wave-uniform
__device__ inline int pick(int v, int t) { return __builtin_amdgcn_readlane(v, t); }
__device__ inline double pick_sample(float v, int t) { return (double)__int_as_float(pick(__float_as_int(v), t)); }
__device__ inline double pick_double(double v, int t) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)pick((int)(unsigned)b, t), hi = (unsigned)pick((int)(b >> 32), t);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__global__ __launch_bounds__(THREADS) void bayes_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        float* __restrict__ jump, double* __restrict__ logz,
                                                        const double* __restrict__ sigma, int64_t n, int L, int K,
                                                        double W, double* work) {
  const int lane = (int)__builtin_amdgcn_workitem_id_x() & 63;
  const int64_t row = (int64_t)__builtin_amdgcn_workgroup_id_x() * WAVES + ((int)__builtin_amdgcn_workitem_id_x() >> 6);
  if (row >= n) return;
  const float* xr = x + row * L;
  float* yr = y + row * L;
  float* jr = jump ? jump + row * L : nullptr;
  double* wr = work + row * ((int64_t)L + 1);
  const double NEG = -__builtin_huge_val();
  const int64_t top = ((int64_t)(L - 1) >> 6) << 6;       // the last chunk's first sample

  const double sg = sigma[row];
  const double h = 1.0 / ((2.0 * sg) * sg);
  bool bad = !(sg > 0.0) || __builtin_isinf(sg) || __builtin_isinf(h);
  double c0 = 0.0, logZ = 0.0;
  if (!bad) {
    c0 = log((SQRT_2PI * sg) / (W * (double)K));
    // sweep 1, s = L - 1 .. 0: this lane's boundary b > s with b = lane (mod 64); n = b - s
    double Gl = lane == (L & 63) ? 0.0 : NEG;              // G[b]; -inf: no such boundary yet (b > L)
    double mean = 0.0, M2 = 0.0;                           // of x[s .. b - 1], from b - 1 down
    const int n0 = ((lane - (int)((L - 1) & 63) - 1) & 63) + 1;
    double rn = 1.0 / (double)n0, hl = 0.5 * log((double)n0);
    if (lane == 0) wr[L] = 0.0;
    for (int64_t base = top; base >= 0; base -= 64) {
      const int cnt = (int)(L - base < 64 ? L - base : 64);
      float xv = 0.f;
      if (lane < cnt) xv = xr[base + lane];
      bad |= (__float_as_uint(xv) & 0x7f800000u) == 0x7f800000u;
      double mine = 0.0;                                   // G[base + lane]
      for (int t = cnt - 1; t >= 0; --t) {                 // s = base + t
        const double v = pick_sample(xv, t);
        const int len = ((lane - t - 1) & 63) + 1;
        const double d = v - mean;
        mean = mean + d * rn;
        M2 = M2 + d * (v - mean);
        double a = Gl + ((c0 - hl) - M2 * h);
        if (len > K) a = NEG;
        const double M = wave_max(a);
        const double S = wave_sum(exp(a - M));
        logZ = M + log(S);                                 // G[s]; the last one is G[0]
        if (lane == t) {                                   // its candidate was n = 64: it takes boundary s
          mine = logZ;
          Gl = logZ;
          mean = 0.0;
          M2 = 0.0;
        }
        rn = __shfl(rn, (lane + 1) & 63);                  // the next step's n is the next lane's of this step
        hl = __shfl(hl, (lane + 1) & 63);
      }
      if (lane < cnt) wr[base + lane] = mine;
    }
    bad = __ballot(bad) != 0;
  }
  if (bad) {
    for (int64_t i = lane; i < L; i += 64) {
      yr[i] = __uint_as_float(QUIET_NAN);
      if (jr) jr[i] = __uint_as_float(QUIET_NAN);
    }
    if (logz && lane == 0) logz[row] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  if (logz && lane == 0) logz[row] = logZ;
  if (jr && lane == 0) jr[0] = 1.0f;

  __threadfence();                                         // G is read by other lanes than wrote it
  // sweep 2, t = 1 .. L: this lane's boundary s < t with s = lane (mod 64); n = t - s
  double Fl = NEG, Ft = 0.0;                               // F[s]; F of the boundary the step starts from
  double mean = 0.0, M2 = 0.0;                             // of x[s .. t - 1], from s up
  double acc = 0.0, done = 0.0;                            // y of sample s so far; of sample s - 64, complete
  const int n0 = ((0 - lane) & 63) + 1;
  double rn = 1.0 / (double)n0, hl = 0.5 * log((double)n0);
  for (int64_t base = 0; base < L; base += 64) {
    const int cnt = (int)(L - base < 64 ? L - base : 64);
    float xv = 0.f;
    double gv = 0.0;                                       // G[base + lane + 1]
    if (lane < cnt) {
      xv = xr[base + lane];
      gv = wr[base + lane + 1];
    }
    float jm = 0.f;                                        // jump[base + lane + 1]
    for (int t = 0; t < cnt; ++t) {                        // the sample base + t; the runs that end behind it
      if (lane == t) {                                     // its candidate was n = 64: it takes boundary base + t
        done = acc;
        acc = 0.0;
        Fl = Ft;
        mean = 0.0;
        M2 = 0.0;
      }
      const double v = pick_sample(xv, t);
      const int len = ((t - lane) & 63) + 1;
      const double d = v - mean;
      mean = mean + d * rn;
      M2 = M2 + d * (v - mean);
      double a = Fl + ((c0 - hl) - M2 * h);
      if (len > K) a = NEG;
      const double M = wave_max(a);
      const double e = exp(a - M);
      const double S = wave_sum(e);
      Ft = M + log(S);
      const double c = exp((M + pick_double(gv, t)) - logZ);
      if (lane == t) jm = (float)(S * c);
      double q = (e * c) * mean;
      const int pos = (lane - t - 1) & 63;                 // 0 for the earliest start
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl(q, (lane - o) & 63);
        if (pos >= o) q = q + u;
      }
      acc = acc + q;
      rn = __shfl(rn, (lane - 1) & 63);
      hl = __shfl(hl, (lane - 1) & 63);
    }
    if (base >= 64) yr[base - 64 + lane] = (float)(lane < cnt ? done : acc);
    if (jr && base + lane + 1 < L) jr[base + lane + 1] = jm;
  }
  if (top + lane < L) yr[top + lane] = (float)acc;
}

}  // namespace bayes

hipError_t launch_bayes_steps(const float* x, float* y, float* jump, double* logz, const double* sigma, int64_t n,
                              int L, int max_len, double level_range, double* work, hipStream_t stream) {
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    const dim3 block(bayes::THREADS), grid((unsigned)((nn + bayes::WAVES - 1) / bayes::WAVES));
    hipLaunchKernelGGL(bayes::bayes_kernel, grid, block, 0, stream, x + n0 * L, y + n0 * L,
                       jump ? jump + n0 * L : nullptr, logz ? logz + n0 : nullptr, sigma + n0, nn, L, max_len,
                       level_range, work + n0 * ((int64_t)L + 1));
  }, (int64_t)0x7fffffff * bayes::WAVES);
}

}  // namespace rdn
