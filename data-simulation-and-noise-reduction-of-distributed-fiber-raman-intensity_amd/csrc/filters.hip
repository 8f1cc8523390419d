// Classical baseline filters on the device: a FIR filter with mirror edges or an edge table (moving
// average, Gaussian, Savitzky-Golay) and a running median, beside the networks they are compared with.
// The arithmetic contract is in include/raman_mi355x.h (rdn_fir, rdn_median); this file is compiled with
// -ffp-contract=off so that each product and each sum of the FIR recurrence is rounded on its own.
//
// One 256-thread workgroup per (spectrum, tile of RDN_FILTER_TILE outputs).  The tile and a halo of
// h = (w - 1) / 2 samples on each side are staged in LDS once, mirror indexing applied while staging; each
// lane then produces 8 consecutive outputs from a register window that slides over its 8 + w - 1 samples:
// one LDS read per tap feeds 8 outputs.  The outputs return through the same LDS image, so the global
// stores are coalesced.  The padded layout (filters.hpp lds_at) keeps the stride-8 reads conflict-free.
//
// The median orders samples by the monotone unsigned key of their bits.  Windows of 3 to 25 run a partial
// sorting network over the window's keys in registers; w = 1 and wider ones a 32-round radix select (one bit
// of the rank-h key per round, each round one pass over the window: 33 w compares per output, NaN round
// included).
//
// Rows are addressed as pointer + 64-bit offset (no buffer descriptor), so any L < 2^31 runs; a spectrum's
// output depends on its own samples only, not on n, its row index or the launches a huge n is split into.
#include "filters.hpp"
#include "host_util.hpp"

namespace rdn {
namespace filt {

__device__ inline int lane_id() { return __builtin_amdgcn_workitem_id_x(); }

// which (row, first output) a workgroup owns
struct Tile {
  int64_t row, t0;
};
__device__ inline Tile my_tile(int tiles) {
  const unsigned b = __builtin_amdgcn_workgroup_id_x(), t = (unsigned)tiles;
  return Tile{(int64_t)(b / t), (int64_t)(b % t) * TILE};
}

// xs[lds_at(s)] = conv(bits of x[idx(t0 - h + s)]) for s < TILE + 2 h, mirror indexing without a repeated
// edge sample; positions past the mirrored end of the row (last tile only, never used) hold conv(0).
template <class Conv>
__device__ inline void stage(uint32_t* xs, const float* __restrict__ xr, int L, int64_t t0, int h, Conv conv) {
  const int count = TILE + 2 * h;
  if (t0 >= h && t0 + TILE + h <= L) {       // an interior tile: every staged sample exists where it stands
    const float* p = xr + (t0 - h);
    for (int s = lane_id(); s < count; s += THREADS) xs[lds_at(s)] = conv(__float_as_uint(p[s]));
    if (lane_id() < PER_LANE) xs[lds_at(count + lane_id())] = conv(0u);
    return;
  }
  for (int s = lane_id(); s < count + PER_LANE; s += THREADS) {
    int64_t j = t0 - h + s;
    if (j < 0) j = -j;
    if (j > L - 1) j = 2 * (int64_t)(L - 1) - j;
    uint32_t u = 0;
    if (s < count && j >= 0 && j < L) u = __float_as_uint(xr[j]);
    xs[lds_at(s)] = conv(u);
  }
}

// The tile's outputs (bits, 8 per lane) through LDS to y: coalesced stores of the positions below L;
// with `skip_edges` the first and last h outputs of the row are left to the edge table.
__device__ inline void store_tile(uint32_t* xs, const uint32_t (&out)[PER_LANE], float* __restrict__ yr, int L,
                                  int64_t t0, int h, bool skip_edges) {
  const int p0 = PER_LANE * lane_id();
  __syncthreads();                       // every lane has read its window
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) xs[lds_at(p0 + o)] = out[o];
  __syncthreads();
  if (t0 + TILE <= L && !(skip_edges && (t0 < h || t0 + TILE > L - h))) {      // a whole tile, no edge output in it
#pragma unroll
    for (int r = 0; r < PER_LANE; ++r) yr[t0 + lane_id() + r * THREADS] = __uint_as_float(xs[lds_at(lane_id() + r * THREADS)]);
    return;
  }
  for (int s = lane_id(); s < TILE; s += THREADS) {
    const int64_t i = t0 + s;
    if (i >= L || (skip_edges && (i < h || i >= L - h))) continue;
    yr[i] = __uint_as_float(xs[lds_at(s)]);
  }
}

__global__ __launch_bounds__(THREADS) void fir_kernel(const float* __restrict__ x, float* __restrict__ y, int L,
                                                      int tiles, const double* __restrict__ taps, int w,
                                                      const double* __restrict__ edge) {
  __shared__ uint32_t xs[STAGE_WORDS];
  __shared__ double tp[MAX_W];
  const Tile t = my_tile(tiles);
  const float* xr = x + t.row * L;
  float* yr = y + t.row * L;
  const int h = (w - 1) / 2, tid = lane_id(), p0 = PER_LANE * tid;
  for (int k = tid; k < w; k += THREADS) tp[k] = taps[k];
  stage(xs, xr, L, t.t0, h, [](uint32_t u) { return u; });
  __syncthreads();

  // output o of this lane is position t0 + p0 + o: its window starts at staged sample p0 + o.  Before tap
  // k, win[m] holds staged sample p0 + q with q = m (mod 8), k <= q < k + 8.
  double acc[PER_LANE];
  float win[PER_LANE];
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) {
    acc[o] = 0.0;
    win[o] = __uint_as_float(xs[lds_at(p0 + o)]);
  }
  for (int k0 = 0; k0 < w; k0 += PER_LANE) {
#pragma unroll
    for (int kk = 0; kk < PER_LANE; ++kk) {
      const int k = k0 + kk;
      if (k < w) {
        const double c = tp[k];
#pragma unroll
        for (int o = 0; o < PER_LANE; ++o) acc[o] = acc[o] + c * (double)win[(o + kk) & (PER_LANE - 1)];
        win[kk] = __uint_as_float(xs[lds_at(p0 + k + PER_LANE)]);
      }
    }
  }
  uint32_t out[PER_LANE];
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) out[o] = __float_as_uint((float)acc[o]);
  store_tile(xs, out, yr, L, t.t0, h, edge != nullptr);

  // edge table: row e < h is output e over the first w samples, row h + e output L - h + e over the last w
  if (edge) {
    for (int e = tid; e < 2 * h; e += THREADS) {
      const int64_t i = e < h ? e : (int64_t)L - 2 * h + e;
      if (i < t.t0 || i >= t.t0 + TILE) continue;
      const float* src = xr + (e < h ? 0 : L - w);
      const double* er = edge + (size_t)e * w;
      double a = 0.0;
      for (int k = 0; k < w; ++k) a = a + er[k] * (double)src[k];
      yr[i] = (float)a;
    }
  }
}

// Monotone unsigned key of a sample's bits (-0 < +0; the infinities ordinary values); every NaN gets the
// largest key, which no other sample has: a window holds a NaN iff its largest key is NAN_KEY.
constexpr uint32_t NAN_KEY = 0xffffffffu, QUIET_NAN = 0x7fc00000u;
__device__ inline uint32_t to_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return NAN_KEY;
  return (u >> 31) ? ~u : u | 0x80000000u;
}
__device__ inline uint32_t from_key(uint32_t k) { return (k >> 31) ? k ^ 0x80000000u : ~k; }

// windows of 3 <= W <= NETWORK_MAX_W: H + 1 passes of a bubble network over the window's keys leave the W - 1 - H largest in
// place, the rank-H key among them (and the largest key, which tells a NaN, after the first pass)
constexpr int NETWORK_MAX_W = 25;
template <int W>
__global__ __launch_bounds__(THREADS) void median_small_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               int L, int tiles) {
  __shared__ uint32_t xs[STAGE_WORDS];
  constexpr int H = (W - 1) / 2;
  const Tile t = my_tile(tiles);
  const int p0 = PER_LANE * lane_id();
  stage(xs, x + t.row * L, L, t.t0, H, to_key);
  __syncthreads();
  uint32_t win[PER_LANE + W - 1], out[PER_LANE];
#pragma unroll
  for (int q = 0; q < PER_LANE + W - 1; ++q) win[q] = xs[lds_at(p0 + q)];
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) {
    uint32_t v[W];
#pragma unroll
    for (int a = 0; a < W; ++a) v[a] = win[o + a];
#pragma unroll
    for (int pass = 0; pass <= H; ++pass) {
#pragma unroll
      for (int a = 0; a + 1 < W - pass; ++a) {
        const uint32_t lo = v[a] < v[a + 1] ? v[a] : v[a + 1], hi = v[a] < v[a + 1] ? v[a + 1] : v[a];
        v[a] = lo;
        v[a + 1] = hi;
      }
    }
    out[o] = v[W - 1] == NAN_KEY ? QUIET_NAN : from_key(v[H]);
  }
  store_tile(xs, out, y + t.row * L, L, t.t0, H, false);
}

// cnt[o] = the number of keys of output o's window that are below cand[o] (the FIR's sliding register window)
__device__ inline void count_below(const uint32_t* xs, int p0, int w, const uint32_t (&cand)[PER_LANE],
                                   int (&cnt)[PER_LANE]) {
  uint32_t win[PER_LANE];
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) {
    cnt[o] = 0;
    win[o] = xs[lds_at(p0 + o)];
  }
  for (int k0 = 0; k0 < w; k0 += PER_LANE) {
#pragma unroll
    for (int kk = 0; kk < PER_LANE; ++kk) {
      const int k = k0 + kk;
      if (k < w) {
#pragma unroll
        for (int o = 0; o < PER_LANE; ++o) cnt[o] += win[(o + kk) & (PER_LANE - 1)] < cand[o];
        win[kk] = xs[lds_at(p0 + k + PER_LANE)];
      }
    }
  }
}

// any odd w: the rank-h key is the largest v with #(keys < v) <= h, found one bit per round from the top
__global__ __launch_bounds__(THREADS) void median_kernel(const float* __restrict__ x, float* __restrict__ y, int L,
                                                         int tiles, int w) {
  __shared__ uint32_t xs[STAGE_WORDS];
  const Tile t = my_tile(tiles);
  const int h = (w - 1) / 2, p0 = PER_LANE * lane_id();
  stage(xs, x + t.row * L, L, t.t0, h, to_key);
  __syncthreads();
  uint32_t key[PER_LANE], cand[PER_LANE], out[PER_LANE];
  int cnt[PER_LANE];
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) key[o] = 0;
  for (int bit = 31; bit >= 0; --bit) {
#pragma unroll
    for (int o = 0; o < PER_LANE; ++o) cand[o] = key[o] | (1u << bit);
    count_below(xs, p0, w, cand, cnt);
#pragma unroll
    for (int o = 0; o < PER_LANE; ++o) key[o] = cnt[o] <= h ? cand[o] : key[o];
  }
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) cand[o] = NAN_KEY;
  count_below(xs, p0, w, cand, cnt);
#pragma unroll
  for (int o = 0; o < PER_LANE; ++o) out[o] = cnt[o] < w ? QUIET_NAN : from_key(key[o]);
  store_tile(xs, out, y + t.row * L, L, t.t0, h, false);
}

// the sorting-network kernel of window w where there is one (3 .. NETWORK_MAX_W), else the radix select
template <int W>
static void launch_median_w(int w, dim3 grid, dim3 block, hipStream_t stream, const float* x, float* y, int L, int tiles) {
  if constexpr (W > NETWORK_MAX_W) hipLaunchKernelGGL(median_kernel, grid, block, 0, stream, x, y, L, tiles, w);
  else if (w == W) hipLaunchKernelGGL(median_small_kernel<W>, grid, block, 0, stream, x, y, L, tiles);
  else launch_median_w<W + 2>(w, grid, block, stream, x, y, L, tiles);
}

}  // namespace filt

hipError_t launch_fir(const float* x, float* y, int64_t n, int L, const double* taps, int w, const double* edge_taps,
                      hipStream_t stream) {
  const int tiles = (int)tiles_of(L, filt::TILE);
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    hipLaunchKernelGGL(filt::fir_kernel, dim3((unsigned)(nn * tiles)), dim3(filt::THREADS), 0, stream, x + n0 * L,
                       y + n0 * L, L, tiles, taps, w, w > 1 ? edge_taps : nullptr);
  }, tiles_chunk(tiles));
}

hipError_t launch_median(const float* x, float* y, int64_t n, int L, int w, hipStream_t stream) {
  const int tiles = (int)tiles_of(L, filt::TILE);
  return launch_chunks(n, [&](int64_t n0, int64_t nn) {
    const dim3 grid((unsigned)(nn * tiles)), block(filt::THREADS);
    const float* xx = x + n0 * L;
    float* yy = y + n0 * L;
    filt::launch_median_w<3>(w, grid, block, stream, xx, yy, L, tiles);
  }, tiles_chunk(tiles));
}

}  // namespace rdn
