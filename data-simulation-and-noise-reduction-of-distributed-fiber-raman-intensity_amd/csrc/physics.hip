// PhysicsAwareLoss on the device: one 512-thread workgroup per spectrum computes, in fp64, the four terms
// of the loss PIDN and APIDN are trained against, their weighted total and the number of masked
// positions, from the noisy input x, the denoised y and clean (definitions, report layout:
// include/raman_mi355x.h rdn_physics; physics.hpp) -- and, for rdn_physics_grad, the gradient of the
// total with respect to y, written in the same first pass.  The reduction and the exact integer
// accumulators are the metrics kernel's (metrics.hpp block_reduce / acc_add), the bin formula is every
// binned report's (report.hpp bin_row): a report's words are the same bits whatever the batch split, the
// atomics' order or the number of ranks whose reports are summed.
//
// Reference: PIDN/train.py:109-146 (F.mse_loss, F.l1_loss of the first differences, the
// torch.diff(clean, n=2) < 0 mask multiplied into both operands of an F.mse_loss over all L - 2 centre
// positions, torch.var (unbiased) of noisy - clean and the mean of (noise^2 - var)^2).
//
// Passes.  The first reads x, y and clean (and the neighbours clean[p - 1], clean[p + 1], y[p + 1], which
// the adjacent lanes load anyway: cache hits) and leaves mu = mean(x - clean); the variance about mu and
// the noise term about the variance are two further passes over d = x - clean, which re-read x and clean
// (the workgroup has just pulled them into L2).  Keeping d in registers instead (up to 32 doubles per
// thread, a fully unrolled straight-line first pass) was built and measured: slower at every length
// (DESIGN.md section 5), so there is one path for every L.  The neighbour indices are clamped into the row
// and the terms that do not exist are selected away, so that no load sits behind a branch.
//
// One routine, three instantiations (VALUE, GRAD): the values alone (rdn_physics: the code it has always
// had), values and gradient (the training step: one launch), the gradient alone (no x, no reduction, no
// noise passes, no LDS).  The gradient is a three-point stencil over what the first pass loads -- one more
// neighbour, y[p - 1] -- and needs no reduction result: 2 scale / L, scale alpha / (L - 1) and
// 2 scale beta / (L - 2) are launch constants.  Its three terms are joined by explicit fmas, so that its
// bits do not depend on what else the instantiation computes; the values' expressions are the same text in
// both instantiations that have them and contract the same way (an e = m y - m c with m in {0, 1} is exact
// either way).
//
// Rows are addressed as pointer + 64-bit offset (no buffer descriptor), so any L < 2^31 runs.
#include <type_traits>

#include "host_util.hpp"
#include "metrics.hpp"
#include "physics.hpp"

namespace rdn {
namespace phys {

using met::MET_THREADS;

template <typename TC, bool VALUE, bool GRAD>
__global__ __launch_bounds__(MET_THREADS) void physics_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const TC* __restrict__ clean, int L, PhysOut po) {
  const int tid = __builtin_amdgcn_workitem_id_x();
  const int64_t n = __builtin_amdgcn_workgroup_id_x();
  const float* xx = x + (size_t)n * L;
  const float* yy = y + (size_t)n * L;
  const TC* cc = clean + (size_t)n * L;
  float* gg = GRAD ? po.grad + (size_t)n * L : nullptr;
  // the gradient's weights: of r = y - clean, of the difference of the two signs, of the masked residual
  const double w0 = GRAD ? (po.scale * 2.0) / L : 0.0, w1 = GRAD ? (po.scale * po.alpha) / (L - 1) : 0.0,
               w2 = GRAD ? ((po.scale * po.beta) * 2.0) / (L - 2) : 0.0;

  // first pass.  A select, not a product, removes the terms that do not exist: a non-finite y at the
  // row's end must not reach a sum it is not part of.
  double se = 0.0, sm = 0.0, pk = 0.0, cnt = 0.0, sd = 0.0;
#pragma unroll 4
  for (int64_t p = tid; p < L; p += MET_THREADS) {
    const bool has_next = p + 1 < L, inner = has_next && p >= 1;
    const int64_t pn = has_next ? p + 1 : p, pm = p >= 1 ? p - 1 : p;
    const TC c0 = cc[p], c1 = cc[pn], cm = cc[pm];
    const double c = c0, a = yy[p], a1 = yy[pn];
    if constexpr (VALUE) {
      const double d = (double)xx[p] - c;
      se += (a - c) * (a - c);
      sd += d;
    }
    const double df = (a1 - a) - ((double)c1 - c);
    if constexpr (VALUE) {
      const double s = fabs(df);
      sm += has_next ? s : 0.0;
    }
    // torch.diff(clean, n=2) < 0 in clean's own type: both first differences rounded to TC, then compared
    const TC dn = c1 - c0, dp = c0 - cm;
    const double m = dn < dp ? 1.0 : 0.0;
    const double e = m * a - m * c;                  // pred * mask - clean * mask: NaN * 0 stays NaN
    if constexpr (VALUE) {
      pk += inner ? e * e : 0.0;
      cnt += inner ? m : 0.0;
    }
    if constexpr (GRAD) {
      // d |e_i| / d e_i as torch's abs backward has it: the sign, 0 for 0 and for NaN.  The difference to
      // the left is the neighbour lane's df, from the same expression on the same values.
      const double dl = (a - (double)yy[pm]) - (c - (double)cm);
      const double sn = has_next ? (double)((df > 0.0) - (df < 0.0)) : 0.0;
      const double sp = p >= 1 ? (double)((dl > 0.0) - (dl < 0.0)) : 0.0;
      const double t2 = inner ? w2 * (m * e) : 0.0;                   // m is a factor: 0 * NaN is NaN
      gg[p] = (float)__builtin_fma(w0, a - c, __builtin_fma(w1, sp - sn, t2));
    }
  }
  if constexpr (!VALUE) return;
  __shared__ double red[MET_THREADS / 64];
  const auto add = [](double a, double b) { return a + b; };
  se = met::block_reduce(se, red, add);
  sm = met::block_reduce(sm, red, add);
  pk = met::block_reduce(pk, red, add);
  cnt = met::block_reduce(cnt, red, add);
  sd = met::block_reduce(sd, red, add);

  // unbiased variance of d in the centred two-pass form, then the mean of (d^2 - var)^2
  const double mu = sd / L;
  double sv = 0.0;
#pragma unroll 4
  for (int64_t p = tid; p < L; p += MET_THREADS) {
    const double t = ((double)xx[p] - (double)cc[p]) - mu;
    sv += t * t;
  }
  sv = met::block_reduce(sv, red, add);
  const double var = sv / (L - 1);
  double sq = 0.0;
#pragma unroll 4
  for (int64_t p = tid; p < L; p += MET_THREADS) {
    const double d = (double)xx[p] - (double)cc[p];
    const double q = d * d - var;
    sq += q * q;
  }
  sq = met::block_reduce(sq, red, add);

  const double mse = se / L, smooth = sm / (L - 1), peak = pk / (L - 2), noise = sq / L;
  const double total = ((mse + po.alpha * smooth) + po.beta * peak) + po.gamma * noise;
  const double v6[RDN_PHYS_QUANTITIES] = {mse, smooth, peak, noise, total, cnt};
  if (tid == 0 && po.per6) {
#pragma unroll
    for (int k = 0; k < RDN_PHYS_QUANTITIES; ++k) po.per6[n * RDN_PHYS_QUANTITIES + k] = v6[k];
  }
  if (!po.report) return;

  long long* row = po.report + (size_t)(po.key ? bin_row(po.key[n], po.bins) : 1) * RDN_PHYS_ROW_WORDS;
  // lanes 0..5 of wave 0 each own one quantity (integer atomics: order-free)
  if (tid < RDN_PHYS_QUANTITIES) {
    double v = v6[0];
#pragma unroll
    for (int k = 1; k < RDN_PHYS_QUANTITIES; ++k) v = tid == k ? v6[k] : v;
    met::acc_add(row, tid, v);
  }
  if (tid == 0) atomicAdd((unsigned long long*)&row[RDN_PHYS_COUNT], 1ull);
}

}  // namespace phys

// The instantiation a launch asks for: values when it has a per6 or a report, the gradient when it has a
// grad (x is not read without values and may be NULL).
hipError_t launch_physics(const float* x, const float* y, const void* clean, bool clean_f64, int64_t n, int L,
                          const phys::PhysOut& po, hipStream_t stream) {
  const bool value = po.per6 || po.report, grad = po.grad != nullptr;
  if (!value && !grad) return hipErrorInvalidValue;
  return with_clean(clean, clean_f64, [&](auto* cc) {
    using TC = std::remove_cv_t<std::remove_pointer_t<decltype(cc)>>;
    const auto kernel = !value ? &phys::physics_kernel<TC, false, true>
                        : grad ? &phys::physics_kernel<TC, true, true>
                               : &phys::physics_kernel<TC, true, false>;
    return launch_chunks(n, [&](int64_t n0, int64_t nn) {
      phys::PhysOut c = po;
      c.per6 = po.per6 ? po.per6 + n0 * RDN_PHYS_QUANTITIES : nullptr;
      c.key = po.key ? po.key + n0 : nullptr;
      c.grad = po.grad ? po.grad + n0 * L : nullptr;
      hipLaunchKernelGGL(kernel, dim3((unsigned)nn), dim3(met::MET_THREADS), 0, stream, value ? x + n0 * L : nullptr,
                         y + n0 * L, cc + n0 * L, L, c);
    });
  });
}

}  // namespace rdn
