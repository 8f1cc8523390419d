// Host sanitizer driver (make asan): exercises the host-only part of the C ABI -- parameter names,
// packed sizes, BatchNorm folding + fragment packing (pack.cpp), argument checking and error
// reporting (abi.cpp) -- under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU call is made.
//
//   host_check <arch> <dtype> <tensors.bin> <blob_out.bin>
//
// tensors.bin: for each name of rdn_param_names(arch), in order: int64 numel, then numel float32
// (written by tests/test_abi.py::test_host_sanitizer_pack).  The packed blob is written to
// blob_out.bin so that the test can compare it byte for byte with the library's own rdn_pack.
// Then the error paths: wrong numel, too-small destination, null pointers, bad arch/dtype, the
// simulator's parameter bounds (rdn_generate with n = 0); and the
// host side of the SNR report (rdn_snr's argument checks, rdn_report_bin, rdn_report_value on an
// exactly-sized report) and of the PhysicsAwareLoss report (rdn_physics's argument checks,
// rdn_physics_value); and the argument checks of the baseline filters (rdn_fir, rdn_median), of
// rdn_haar_shrink, of rdn_physics_grad, of rdn_potts and rdn_noise_mad, and of rdn_bayes_steps (every refusal, each
// overlap pair, n = 0 succeeding).
// And the pure host helpers of the launch path, which no device test can reach: the once-per-(kernel,
// device) bookkeeping of the LDS opt-in with a counting fake setter (host_util.hpp once_per: repeats,
// device bounds, a failing setter, 8 racing threads, a full table), the chunk walk (for_chunks,
// tiles_chunk: 2^33 workgroups in 5 launches; tiles_of and the chunk of every tile size up to rows of
// 2^31 - 1 samples; the refusal of a chunk below 1), overlaps(), and the forward's geometry choice
// (geometry.hpp forward_geometry) against values derived by hand from its formulas.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/raman_mi355x.h"
#include "geometry.hpp"
#include "host_util.hpp"

static int fails = 0;
#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "host_check: FAILED %s (line %d)\n", #c, __LINE__); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

// the last error names the check that refused
static bool refused(int rc, const char* what) { return rc == RDN_EINVAL && std::strstr(rdn_last_error(), what); }

static void check_once_per() {
  using rdn::once_per;
  static char kernels[rdn::OnceTable::CAPACITY + 2];      // distinct addresses stand in for kernels
  int calls = 0;
  const auto ok = [&] { ++calls; return hipSuccess; };
  {
    rdn::OnceTable t;
    EXPECT(once_per(t, &kernels[0], 0, ok) == hipSuccess && once_per(t, &kernels[0], 0, ok) == hipSuccess && calls == 1);
    EXPECT(once_per(t, &kernels[1], 0, ok) == hipSuccess && calls == 2);                 // another kernel, same device
    EXPECT(once_per(t, &kernels[0], 63, ok) == hipSuccess && calls == 3);                // same kernel, devices 0 and 63
    EXPECT(once_per(t, &kernels[0], 63, ok) == hipSuccess && once_per(t, &kernels[1], 0, ok) == hipSuccess && calls == 3);
    EXPECT(once_per(t, &kernels[0], -1, ok) == hipErrorInvalidValue && once_per(t, &kernels[0], 64, ok) == hipErrorInvalidValue);
    EXPECT(once_per(t, nullptr, 0, ok) == hipErrorInvalidValue && calls == 3);
    // a setter that fails once is asked again, then never again
    int tries = 0;
    const auto flaky = [&] { return ++tries == 1 ? hipErrorInvalidValue : hipSuccess; };
    EXPECT(once_per(t, &kernels[2], 5, flaky) == hipErrorInvalidValue && tries == 1);
    EXPECT(once_per(t, &kernels[2], 5, flaky) == hipSuccess && tries == 2);
    EXPECT(once_per(t, &kernels[2], 5, flaky) == hipSuccess && tries == 2);
    EXPECT(t.used.load() == 3);
  }
  {  // 8 threads race on one pair: one set, and every thread sees success
    rdn::OnceTable t;
    std::atomic<int> sets{0}, good{0}, go{0};
    std::vector<std::thread> th;
    for (int i = 0; i < 8; ++i)
      th.emplace_back([&] {
        while (!go.load()) {}
        for (int r = 0; r < 100; ++r)
          good += once_per(t, &kernels[0], 7, [&] { ++sets; return hipSuccess; }) == hipSuccess;
      });
    go = 1;
    for (auto& x : th) x.join();
    EXPECT(sets.load() == 1 && good.load() == 800);
  }
  {  // a full table refuses a new kernel (without calling the setter) and still serves the ones it holds
    rdn::OnceTable t;
    calls = 0;
    for (int i = 0; i < rdn::OnceTable::CAPACITY; ++i) EXPECT(once_per(t, &kernels[i], 1, ok) == hipSuccess);
    EXPECT(calls == rdn::OnceTable::CAPACITY);
    EXPECT(once_per(t, &kernels[rdn::OnceTable::CAPACITY], 1, ok) != hipSuccess && calls == rdn::OnceTable::CAPACITY);
    EXPECT(once_per(t, &kernels[rdn::OnceTable::CAPACITY - 1], 2, ok) == hipSuccess && calls == rdn::OnceTable::CAPACITY + 1);
  }
}

static void check_chunks() {
  // the calls are contiguous from 0, none is empty or exceeds `chunk`, and they end at n
  const auto walk = [](int64_t n, int64_t chunk) {
    int64_t next = 0, calls = 0;
    bool good = true;
    const hipError_t e = rdn::for_chunks(n, chunk, [&](int64_t n0, int64_t nn) {
      good = good && n0 == next && nn >= 1 && nn <= chunk;
      next = n0 + nn;
      ++calls;
    });
    return e == hipSuccess && good && next == (n > 0 ? n : 0) ? calls : (int64_t)-1;
  };
  EXPECT(walk(0, 7) == 0);
  EXPECT(walk(7, 7) == 1);
  EXPECT(walk(8, 7) == 2);
  EXPECT(walk(1, 0x7fffffff) == 1);
  EXPECT(walk((int64_t)1 << 33, 0x7fffffff) == 5);         // 4 (2^31 - 1) = 2^33 - 4: a fifth launch of 4
  EXPECT(rdn::tiles_chunk(18) * 18 <= 0x7fffffff && (rdn::tiles_chunk(18) + 1) * 18 > 0x7fffffff);
  EXPECT(rdn::tiles_chunk(1) == 0x7fffffff);

  // a chunk below 1 is refused without a call (forwards it would never end, backwards it would leave the buffer)
  for (int64_t chunk : {(int64_t)0, (int64_t)-1, (int64_t)-2048}) {
    int64_t calls = 0;
    EXPECT(rdn::for_chunks(1, chunk, [&](int64_t, int64_t) { ++calls; }) == hipErrorInvalidValue && calls == 0);
    EXPECT(rdn::for_chunks(0, chunk, [&](int64_t, int64_t) { ++calls; }) == hipErrorInvalidValue && calls == 0);
    EXPECT(rdn::launch_chunks(1, [&](int64_t, int64_t) { ++calls; }, chunk) == hipErrorInvalidValue && calls == 0);
  }
  EXPECT(rdn::for_chunks(3, 2, [](int64_t, int64_t) {}) == hipSuccess);
  EXPECT(rdn::tiles_chunk(0) == 0 && rdn::tiles_chunk(-1048575) == 0);

  // Every tile size a launcher uses (the filters' 2048, Haar's 512, the positions a forward's tile owns: 198 to
  // 628) at every admitted row length where the count could slip: the tile count is the exact ceiling and a
  // positive int, its chunk is at least one spectrum and fills grid.x at most, and the walk covers the batch.
  const int64_t top = (int64_t)1 << 31;
  for (int64_t T : {(int64_t)2048, (int64_t)512, (int64_t)198, (int64_t)500, (int64_t)582, (int64_t)600, (int64_t)628}) {
    for (int64_t L : {(int64_t)1, T - 1, T, T + 1, top - T, top - T + 1, top - 1}) {
      const int64_t tiles = rdn::tiles_of(L, T);
      // the ceiling by its definition, without the sum that wraps: (tiles - 1) T < L <= tiles T
      EXPECT(tiles >= 1 && tiles <= 0x7fffffff && (tiles - 1) * T < L && L <= tiles * T);
      EXPECT((int)tiles == tiles);
      const int64_t chunk = rdn::tiles_chunk(tiles);
      EXPECT(chunk >= 1 && chunk * tiles <= 0x7fffffff && (chunk + 1) * tiles > 0x7fffffff);
      if (chunk < 1) continue;                 // reported above
      EXPECT(walk(1, chunk) == 1);
      const int64_t n = (int64_t)1 << 33;      // the smallest chunk here is 198 spectra: 4.3e7 calls
      EXPECT(walk(n, chunk) == (n + chunk - 1) / chunk);
    }
  }
}

static void check_overlaps() {
  char b[64];
  EXPECT(rdn::overlaps(b, 16, b, 16));
  EXPECT(!rdn::overlaps(b, 16, b + 16, 16) && !rdn::overlaps(b + 16, 16, b, 16));     // end to start
  EXPECT(rdn::overlaps(b, 17, b + 16, 16) && rdn::overlaps(b + 16, 16, b, 17));       // one byte, from the left
  EXPECT(rdn::overlaps(b, 16, b + 15, 16) && rdn::overlaps(b + 15, 16, b, 16));       // ... from the right
  EXPECT(!rdn::overlaps(b + 8, 0, b, 16) && !rdn::overlaps(b, 16, b + 8, 0) && !rdn::overlaps(b, 0, b, 0));
}

static void check_forward_geometry() {
  using G = rdn::Geometry;
  const auto geo = [](int dtype, int64_t n, int64_t L, int64_t cus = 256, int so = -1, int wo = -1) {
    return rdn::forward_geometry(RDN_RRCDNET, dtype, n, L, cus, so, wo);
  };
  // RRCDNet: halo 29, so a 640-row tile owns T = 582 positions and L = 10,000 is 18 tiles (17 T = 9894);
  // its walk is wt = ceil((10,000 + 28) / 576) = 18 tiles of 576 rows.  256 CUs.
  for (int dtype : {RDN_F16MIX, RDN_F16}) {
    EXPECT(geo(dtype, 1, 10000) == G::Short);              // 2 * 1 * 18 = 36 <= 256
    EXPECT(geo(dtype, 7, 10000) == G::Short);              // 2 * 7 * 18 = 252 <= 256
    // 2 * 8 * 18 = 288 > 256; walk ceil(8 / 256) * 18 * 576 = 10,368 rows against ceil(144 / 256) * 640 = 640
    EXPECT(geo(dtype, 8, 10000) == G::Tiled);
    // walk ceil(8192 / 256) = 32 rounds * 18 * 576 = 331,776 < ceil(147,456 / 256) = 576 rounds * 640 = 368,640
    EXPECT(geo(dtype, 8192, 10000) == G::Walk);
    // L = 7 is one tile: 2 * 128 = 256 <= 256; 2 * 129 = 258 > 256, and then the walk's one round of
    // ceil(35 / 576) = 1 tile, 576 rows, is below the tile's one round of 640
    EXPECT(geo(dtype, 128, 7) == G::Short);
    EXPECT(geo(dtype, 129, 7) == G::Walk);
    // no CU count: Tiled
    for (int64_t n : {1, 7, 8, 8192}) EXPECT(geo(dtype, n, 10000, 0) == G::Tiled);
    // RDN_SHORT_TILES: 1 forces Short where the rule says Walk, 0 refuses it where the rule says Short (n = 1
    // is then Tiled: 10,368 walk rows against 640)
    EXPECT(geo(dtype, 8192, 10000, 256, 1) == G::Short && geo(dtype, 8192, 10000, 0, 1) == G::Short);
    EXPECT(geo(dtype, 1, 10000, 256, 0) == G::Tiled);
    // RDN_WALK: 1 forces Walk where the rule says Tiled (also without a CU count), 0 refuses it where the
    // rule says Walk; Short is tested first
    EXPECT(geo(dtype, 8, 10000, 256, -1, 1) == G::Walk && geo(dtype, 8, 10000, 0, -1, 1) == G::Walk);
    EXPECT(geo(dtype, 8192, 10000, 256, -1, 0) == G::Tiled);
    EXPECT(geo(dtype, 1, 10000, 256, -1, 1) == G::Short && geo(dtype, 1, 10000, 256, 0, 1) == G::Walk);
  }
  // the other dtypes have the one geometry, whatever the overrides say
  for (int dtype : {RDN_BF16, RDN_F32, RDN_BF16X3, RDN_F16F8})
    for (int64_t n : {1, 7, 8, 8192}) EXPECT(geo(dtype, n, 10000) == G::Tiled && geo(dtype, n, 10000, 256, 1, 1) == G::Tiled);
}

// rdn_haar_shrink and rdn_physics_grad: every refusal comes before any HIP call (each call below is
// refused or has n = 0), in the order the checks have always been reported in
static void check_haar_and_grad_args() {
  std::vector<float> buf(256, 0.f);
  float* b = buf.data();
  const double k3[3] = {1.0, 0.5, 0.25};
  const double inf = INFINITY, nan = NAN;
  {
    const auto haar = [&](const float* x, float* y, double* med, int64_t n, int64_t L, int levels, const double* k,
                          int mode = RDN_HAAR_HARD) { return rdn_haar_shrink(x, y, med, n, L, levels, k, mode, nullptr); };
    double* med = (double*)(b + 128);
    EXPECT(refused(haar(b, b + 32, med, 1, 16, 3, nullptr), "null pointer"));
    EXPECT(refused(haar(nullptr, nullptr, nullptr, 0, 16, 3, nullptr), "null pointer"));   // k: for n = 0 too
    EXPECT(refused(haar(nullptr, b + 32, med, 1, 16, 3, k3), "null pointer"));
    EXPECT(refused(haar(b, nullptr, med, 1, 16, 3, k3), "null pointer"));
    EXPECT(refused(haar(b, b + 32, nullptr, 1, 16, 3, k3), "null pointer"));
    EXPECT(refused(haar(b, b + 32, med, -1, 16, 3, k3), "need n >= 0"));
    EXPECT(refused(haar(b, b + 32, med, 1, 16, 0, k3), "levels"));
    EXPECT(refused(haar(b, b + 32, med, 1, 1 << 10, RDN_HAAR_MAX_LEVELS + 1, k3), "levels"));
    EXPECT(refused(haar(b, b + 32, med, 1, 16, 3, k3, 2), "unknown mode 2"));
    EXPECT(refused(haar(b, b + 32, med, 1, 16, 3, k3, -1), "unknown mode -1"));
    EXPECT(refused(haar(b, b + 32, med, 1, 7, 3, k3), "2^levels <= L"));
    EXPECT(refused(haar(nullptr, nullptr, nullptr, 0, (int64_t)1 << 31, 3, k3), "2^levels <= L"));
    for (double bad : {nan, inf, -inf, -1.0}) {
      const double k[3] = {1.0, 0.5, bad};
      EXPECT(refused(haar(b, b + 32, med, 1, 16, 3, k), "every k"));
    }
    const double k2[3] = {1.0, 0.5, nan};                  // entries past `levels` are not read
    EXPECT(haar(nullptr, nullptr, nullptr, 0, 16, 2, k2) == RDN_OK);
    EXPECT(refused(haar(b, b + 15, med, 1, 16, 3, k3), "x and y overlap"));
    EXPECT(refused(haar(b + 15, b, med, 1, 16, 3, k3), "x and y overlap"));
    EXPECT(refused(haar(b, b + 32, (double*)(b + 14), 1, 16, 3, k3), "med overlaps"));     // the last 8 bytes of x
    EXPECT(refused(haar(b, b + 32, (double*)(b + 32), 1, 16, 3, k3), "med overlaps"));     // the first 8 of y
    EXPECT(haar(nullptr, nullptr, nullptr, 0, 16, 3, k3) == RDN_OK);
    EXPECT(haar(nullptr, nullptr, nullptr, 0, ((int64_t)1 << 31) - 1, 3, k3, RDN_HAAR_SOFT) == RDN_OK);
  }
  {
    std::vector<double> per(6, 0.0);
    const auto grad = [&](const float* x, const float* y, const void* clean, int f64, int64_t n, int64_t L, float* g,
                          double alpha = 0.1, double scale = 1.0, double* per6 = nullptr) {
      return rdn_physics_grad(x, y, clean, f64, n, L, alpha, 0.05, 0.01, scale, per6, g, nullptr);
    };
    // n = 1, L = 16: x at 0, y at 16, clean at 32 (fp64: floats 32 .. 63), grad at 64
    EXPECT(refused(grad(b, nullptr, b + 32, 0, 1, 16, b + 64), "null pointer"));
    EXPECT(refused(grad(b, b + 16, nullptr, 0, 1, 16, b + 64), "null pointer"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, nullptr), "null pointer"));
    EXPECT(refused(grad(nullptr, b + 16, b + 32, 0, 1, 16, b + 64, 0.1, 1.0, per.data()), "per_spectrum6 needs x"));
    EXPECT(refused(grad(b, b + 16, b + 32, 2, 1, 16, b + 64), "clean_is_f64"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, -1, 16, b + 64), "3 <= L < 2^31"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 2, b + 64), "3 <= L < 2^31"));
    EXPECT(refused(grad(nullptr, nullptr, nullptr, 0, 0, (int64_t)1 << 31, nullptr), "3 <= L < 2^31"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 64, nan), "weights"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 64, inf), "weights"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 64, 0.1, nan), "scale must be finite"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 64, 0.1, -inf), "scale must be finite"));
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 15), "grad overlaps"));           // x's last sample
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 1), "grad overlaps"));            // x and y
    EXPECT(refused(grad(nullptr, b + 16, b + 32, 0, 1, 16, b + 31), "grad overlaps"));     // y's last sample (no x)
    EXPECT(refused(grad(b, b + 16, b + 32, 0, 1, 16, b + 47), "grad overlaps"));           // fp32 clean's last sample
    EXPECT(refused(grad(b, b + 16, b + 32, 1, 1, 16, b + 48), "grad overlaps"));           // fp64 clean's second half
    EXPECT(refused(grad(b, b + 16, b + 32, 1, 1, 16, b + 63), "grad overlaps"));
    EXPECT(grad(nullptr, nullptr, nullptr, 0, 0, 16, nullptr) == RDN_OK);
    EXPECT(grad(nullptr, nullptr, nullptr, 1, 0, ((int64_t)1 << 31) - 1, nullptr, 0.1, 1.0, per.data()) == RDN_OK);
  }
}

// rdn_potts and rdn_noise_mad: likewise every refusal, each overlap pair, n = 0 succeeding
static void check_potts_and_mad_args() {
  std::vector<float> buf(512, 0.f);
  float* b = buf.data();
  {
    // n = 1, L = 16: x at floats 0 .. 15, y at 16 .. 31, work (16 bytes) at float 32, nseg at 40, gamma at 64
    uint8_t* const w = (uint8_t*)(b + 32);
    int32_t* const s = (int32_t*)(b + 40);
    const double* const g = (const double*)(b + 64);
    const auto potts = [&](const float* x, float* y, int32_t* nseg, const double* gamma, int64_t n, int64_t L, int K,
                           uint8_t* work, size_t wb) { return rdn_potts(x, y, nseg, gamma, n, L, K, work, wb, nullptr); };
    EXPECT(refused(potts(b, b + 16, s, nullptr, 1, 16, 64, w, 16), "null gamma"));
    EXPECT(refused(potts(nullptr, nullptr, nullptr, nullptr, 0, 16, 64, nullptr, 0), "null gamma"));   // for n = 0 too
    EXPECT(refused(potts(b, b + 16, s, g, -1, 16, 64, w, 16), "need n >= 0"));
    for (int K : {0, -1, RDN_POTTS_MAX_LEN + 1}) {
      EXPECT(refused(potts(b, b + 16, s, g, 1, 16, K, w, 16), "max_len"));
      EXPECT(refused(potts(nullptr, nullptr, nullptr, g, 0, 16, K, nullptr, 0), "max_len"));
    }
    for (int64_t L : {(int64_t)0, (int64_t)-3, (int64_t)1 << 31}) {
      EXPECT(refused(potts(b, b + 16, s, g, 1, L, 64, w, (size_t)1 << 40), "1 <= L < 2^31"));
      EXPECT(refused(potts(nullptr, nullptr, nullptr, g, 0, L, 64, nullptr, 0), "1 <= L < 2^31"));
    }
    EXPECT(refused(potts(nullptr, b + 16, s, g, 1, 16, 64, w, 16), "null pointer"));
    EXPECT(refused(potts(b, nullptr, s, g, 1, 16, 64, w, 16), "null pointer"));
    EXPECT(refused(potts(b, b + 16, s, g, 1, 16, 64, nullptr, 16), "null pointer"));
    EXPECT(refused(potts(b, b + 16, s, g, 1, 16, 64, w, 15), "work_bytes"));
    EXPECT(refused(potts(b, b + 32, s, g, 2, 16, 64, (uint8_t*)(b + 100), 31), "work_bytes"));
    EXPECT(refused(potts(b, b + 15, s, g, 1, 16, 64, w, 16), "x and y overlap"));
    EXPECT(refused(potts(b + 15, b, s, g, 1, 16, 64, w, 16), "x and y overlap"));
    EXPECT(refused(potts(b, b + 16, s, g, 1, 16, 64, (uint8_t*)(b + 16) - 1, 16), "work overlaps"));   // x's last byte
    EXPECT(refused(potts(b, b + 16, s, g, 1, 16, 64, (uint8_t*)(b + 32) - 1, 16), "work overlaps"));   // y's last byte
    EXPECT(refused(potts(b + 100, b + 16, s, g, 1, 16, 64, (uint8_t*)(b + 16) - 15, 16), "work overlaps"));  // y's first
    EXPECT(refused(potts(b, b + 16, (int32_t*)(b + 15), g, 1, 16, 64, w, 16), "nseg overlaps"));       // x
    EXPECT(refused(potts(b, b + 16, (int32_t*)(b + 31), g, 1, 16, 64, w, 16), "nseg overlaps"));       // y
    EXPECT(refused(potts(b, b + 16, (int32_t*)(b + 35), g, 1, 16, 64, w, 16), "nseg overlaps"));       // work's last 4 bytes
    EXPECT(refused(potts(b, b + 16, s, g, 1, 16, 64, w, 33), "nseg overlaps"));                        // the stated extent
    EXPECT(potts(nullptr, nullptr, nullptr, g, 0, 16, 64, nullptr, 0) == RDN_OK);
    EXPECT(potts(nullptr, nullptr, nullptr, g, 0, ((int64_t)1 << 31) - 1, 1, nullptr, 0) == RDN_OK);
  }
  {
    double* med = (double*)(b + 128);
    const auto mad = [&](const float* x, double* m, int64_t n, int64_t L) { return rdn_noise_mad(x, m, n, L, nullptr); };
    EXPECT(refused(mad(nullptr, med, 1, 16), "null pointer"));
    EXPECT(refused(mad(b, nullptr, 1, 16), "null pointer"));
    EXPECT(refused(mad(b, med, -1, 16), "1 <= L < 2^31"));
    EXPECT(refused(mad(b, med, 1, 0), "1 <= L < 2^31"));
    EXPECT(refused(mad(nullptr, nullptr, 0, 0), "1 <= L < 2^31"));
    EXPECT(refused(mad(nullptr, nullptr, 0, (int64_t)1 << 31), "1 <= L < 2^31"));
    EXPECT(refused(mad(b, (double*)(b + 14), 1, 16), "med overlaps"));     // the last 8 bytes of x
    EXPECT(refused(mad(b + 1, (double*)b, 1, 16), "med overlaps"));        // 4 bytes below x and its first 4
    EXPECT(mad(nullptr, nullptr, 0, 1) == RDN_OK);
    EXPECT(mad(nullptr, nullptr, 0, ((int64_t)1 << 31) - 1) == RDN_OK);
  }
}

// rdn_bayes_steps: likewise every refusal, each overlap pair, n = 0 succeeding
static void check_bayes_args() {
  std::vector<double> buf(256, 0.0);
  float* b = (float*)buf.data();
  // n = 1, L = 16: x at floats 0 .. 15, y at 16 .. 31, jump at 32 .. 47, work (17 doubles) at float 64 .. 97,
  // logz at float 128, sigma at float 160
  double* const w = (double*)(b + 64);
  double* const z = (double*)(b + 128);
  const double* const s = (const double*)(b + 160);
  const size_t wb = 17 * sizeof(double);
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const auto bayes = [&](const float* x, float* y, float* jump, double* logz, const double* sigma, int64_t n, int64_t L,
                         int K, double W, double* work, size_t bytes) {
    return rdn_bayes_steps(x, y, jump, logz, sigma, n, L, K, W, work, bytes, nullptr);
  };
  EXPECT(refused(bayes(b, b + 16, b + 32, z, nullptr, 1, 16, 40, 1.0, w, wb), "null sigma"));
  EXPECT(refused(bayes(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 16, 40, 1.0, nullptr, 0), "null sigma"));
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, -1, 16, 40, 1.0, w, wb), "need n >= 0"));
  for (int K : {0, -1, RDN_BAYES_MAX_LEN + 1}) {
    EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, K, 1.0, w, wb), "max_len"));
    EXPECT(refused(bayes(nullptr, nullptr, nullptr, nullptr, s, 0, 16, K, 1.0, nullptr, 0), "max_len"));
  }
  for (double W : {0.0, -1.0, nan, inf, -inf}) {
    EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, 40, W, w, wb), "level_range"));
    EXPECT(refused(bayes(nullptr, nullptr, nullptr, nullptr, s, 0, 16, 40, W, nullptr, 0), "level_range"));
  }
  for (int64_t L : {(int64_t)0, (int64_t)-3, (int64_t)1 << 31}) {
    EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, L, 40, 1.0, w, (size_t)1 << 40), "1 <= L < 2^31"));
    EXPECT(refused(bayes(nullptr, nullptr, nullptr, nullptr, s, 0, L, 40, 1.0, nullptr, 0), "1 <= L < 2^31"));
  }
  EXPECT(refused(bayes(nullptr, b + 16, b + 32, z, s, 1, 16, 40, 1.0, w, wb), "null pointer"));
  EXPECT(refused(bayes(b, nullptr, b + 32, z, s, 1, 16, 40, 1.0, w, wb), "null pointer"));
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, 40, 1.0, nullptr, wb), "null pointer"));
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, 40, 1.0, (double*)(b + 65), wb), "8-byte aligned"));
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, 40, 1.0, w, wb - 1), "work_bytes"));
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 2, 7, 40, 1.0, w, 127), "work_bytes"));
  EXPECT(refused(bayes(b, b + 15, b + 32, z, s, 1, 16, 40, 1.0, w, wb), "x and y overlap"));
  EXPECT(refused(bayes(b + 15, b, b + 32, z, s, 1, 16, 40, 1.0, w, wb), "x and y overlap"));
  EXPECT(refused(bayes(b, b + 16, b + 48, z, s, 1, 16, 40, 1.0, (double*)(b + 14), wb), "work overlaps"));     // x's last 8 bytes
  EXPECT(refused(bayes(b + 200, b + 32, nullptr, z, s, 1, 16, 40, 1.0, (double*)b, wb), "work overlaps"));     // y's first 8
  EXPECT(refused(bayes(b, b + 16, b + 15, z, s, 1, 16, 40, 1.0, w, wb), "jump overlaps"));                     // x and y
  EXPECT(refused(bayes(b, b + 16, b + 31, z, s, 1, 16, 40, 1.0, w, wb), "jump overlaps"));                     // y's last sample
  EXPECT(refused(bayes(b, b + 16, b + 97, z, s, 1, 16, 40, 1.0, w, wb), "jump overlaps"));                     // work's last 4 bytes
  EXPECT(refused(bayes(b, b + 16, b + 32, (double*)(b + 14), s, 1, 16, 40, 1.0, w, wb), "logz overlaps"));     // x
  EXPECT(refused(bayes(b, b + 16, b + 32, (double*)(b + 30), s, 1, 16, 40, 1.0, w, wb), "logz overlaps"));     // y
  EXPECT(refused(bayes(b, b + 16, b + 32, (double*)(b + 96), s, 1, 16, 40, 1.0, w, wb), "logz overlaps"));     // work's last double
  EXPECT(refused(bayes(b, b + 16, b + 32, (double*)(b + 46), s, 1, 16, 40, 1.0, w, wb), "logz overlaps"));     // jump
  EXPECT(refused(bayes(b, b + 16, b + 32, z, s, 1, 16, 40, 1.0, w, 33 * sizeof(double)), "logz overlaps"));    // the stated extent
  EXPECT(refused(bayes(b, b + 16, b + 32, z, (const double*)(b + 30), 1, 16, 40, 1.0, w, wb), "sigma overlaps"));   // y
  EXPECT(refused(bayes(b, b + 16, b + 32, z, (const double*)(b + 46), 1, 16, 40, 1.0, w, wb), "sigma overlaps"));   // jump
  EXPECT(refused(bayes(b, b + 16, b + 32, z, w + 16, 1, 16, 40, 1.0, w, wb), "sigma overlaps"));               // work
  EXPECT(refused(bayes(b, b + 16, b + 32, z, z, 1, 16, 40, 1.0, w, wb), "sigma overlaps"));                    // logz
  EXPECT(bayes(nullptr, nullptr, nullptr, nullptr, s, 0, 16, 40, 1.0, nullptr, 0) == RDN_OK);
  EXPECT(bayes(nullptr, nullptr, nullptr, nullptr, s, 0, ((int64_t)1 << 31) - 1, 1, 2.5, nullptr, 0) == RDN_OK);
}

int main(int argc, char** argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: host_check <arch> <dtype> <tensors.bin> <blob_out.bin>\n");
    return 2;
  }
  const int arch = std::atoi(argv[1]), dtype = std::atoi(argv[2]);
  size_t need = 0;
  EXPECT(rdn_param_names(arch, nullptr, 0, &need) == RDN_OK && need > 1);
  std::string names(need, '\0');
  EXPECT(rdn_param_names(arch, &names[0], need, &need) == RDN_OK);
  // a truncating buffer reports ESIZE and still NUL-terminates
  char small[8];
  EXPECT(rdn_param_names(arch, small, sizeof small, &need) == RDN_ESIZE && small[7] == '\0');
  size_t n_names = 0;
  for (char c : names) n_names += c == '\n';

  std::FILE* f = std::fopen(argv[3], "rb");
  if (!f) return 2;
  std::vector<std::vector<float>> data;
  std::vector<int64_t> numels;
  int64_t ne = 0;
  while (std::fread(&ne, sizeof ne, 1, f) == 1) {
    std::vector<float> t((size_t)ne);
    if (ne && std::fread(t.data(), sizeof(float), (size_t)ne, f) != (size_t)ne) return 2;
    numels.push_back(ne);
    data.push_back(std::move(t));
  }
  std::fclose(f);
  EXPECT(data.size() == n_names);
  std::vector<const float*> ptrs;
  for (auto& t : data) ptrs.push_back(t.data());

  size_t bytes = 0;
  EXPECT(rdn_packed_size(arch, dtype, &bytes) == RDN_OK && bytes > 0);
  std::vector<unsigned char> blob(bytes);
  const int n = (int)ptrs.size();
  EXPECT(rdn_pack(arch, dtype, ptrs.data(), numels.data(), n, blob.data(), bytes) == RDN_OK);
  // exactly-sized heap buffer: ASan flags any write past `bytes`
  {
    unsigned char* exact = (unsigned char*)std::malloc(bytes);
    EXPECT(rdn_pack(arch, dtype, ptrs.data(), numels.data(), n, exact, bytes) == RDN_OK);
    EXPECT(std::memcmp(exact, blob.data(), bytes) == 0);
    std::free(exact);
  }
  std::FILE* o = std::fopen(argv[4], "wb");
  if (!o) return 2;
  std::fwrite(blob.data(), 1, bytes, o);
  std::fclose(o);
  // error paths (they may leave `blob` partially written): every one reports, none writes or reads
  // out of bounds
  EXPECT(rdn_pack(arch, dtype, ptrs.data(), numels.data(), n, blob.data(), bytes - 1) == RDN_ESIZE);
  EXPECT(std::strlen(rdn_last_error()) > 0);
  std::vector<int64_t> bad = numels;
  bad[n / 2] -= 1;
  EXPECT(rdn_pack(arch, dtype, ptrs.data(), bad.data(), n, blob.data(), bytes) == RDN_ESHAPE);
  EXPECT(rdn_pack(arch, dtype, ptrs.data(), numels.data(), n - 1, blob.data(), bytes) == RDN_ESHAPE);
  EXPECT(rdn_pack(arch, dtype, nullptr, numels.data(), n, blob.data(), bytes) == RDN_EINVAL);
  EXPECT(rdn_pack(99, dtype, ptrs.data(), numels.data(), n, blob.data(), bytes) == RDN_EINVAL);
  EXPECT(rdn_pack(arch, 17, ptrs.data(), numels.data(), n, blob.data(), bytes) == RDN_EINVAL);
  EXPECT(rdn_packed_size(arch, dtype, nullptr) == RDN_EINVAL);
  // forward argument checks happen before any HIP call
  EXPECT(rdn_forward(arch, dtype, nullptr, nullptr, nullptr, 1, 100, nullptr, 0, nullptr) == RDN_EINVAL);
  EXPECT(rdn_forward(arch, dtype, blob.data(), (const float*)blob.data(), (float*)blob.data(), -1, 100, nullptr, 0,
                     nullptr) == RDN_EINVAL);
  EXPECT(rdn_forward(arch, dtype, blob.data(), (const float*)blob.data(), (float*)blob.data(), 1, 0, nullptr, 0,
                     nullptr) == RDN_EINVAL);
  EXPECT(rdn_metrics(nullptr, nullptr, 1, 100, nullptr, nullptr, nullptr) == RDN_EINVAL);
  EXPECT(rdn_generate(0, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RDN_EINVAL);
  // simulator parameters, n = 0 (nothing touches the device): the 32-bit scan bound at both ends, non-finite floats
  {
    auto gen = [](int64_t L, float lo, float hi, float prob, int32_t max_repeat) {
      const rdn_gen_params p{L, lo, hi, prob, max_repeat};
      return rdn_generate(~0ull, ~0ull, 0, &p, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    const float inf = INFINITY, nan = NAN;
    EXPECT(gen(1000, 20.f, 37.f, 0.05f, 8388604) == RDN_OK);
    EXPECT(gen(1000, 20.f, 37.f, 0.05f, 8388605) == RDN_EINVAL);
    EXPECT(gen(1000, 20.f, 37.f, 0.05f, INT32_MAX) == RDN_EINVAL);
    EXPECT(gen(1000, 20.f, 37.f, 0.05f, INT32_MIN) == RDN_EINVAL);
    EXPECT(gen(INT32_MAX, 20.f, 37.f, 0.05f, 1) == RDN_EINVAL);
    EXPECT(gen(INT64_MAX, 20.f, 37.f, 0.05f, INT32_MAX) == RDN_EINVAL);
    EXPECT(gen(INT32_MAX - 256, 5.f, 5.f, 1.f, 1) == RDN_OK);
    EXPECT(gen(1000, nan, 37.f, 0.05f, 40) == RDN_EINVAL);
    EXPECT(gen(1000, 20.f, inf, 0.05f, 40) == RDN_EINVAL);
    EXPECT(gen(1000, -inf, 37.f, 0.05f, 40) == RDN_EINVAL);
    EXPECT(gen(1000, 20.f, 37.f, nan, 40) == RDN_EINVAL);
  }
  // SNR report: argument checks, the bin formula and the host conversion of an exactly-sized report
  {
    const int nb = 3;
    std::vector<int64_t> rep(RDN_REPORT_WORDS(nb), 0);
    std::vector<double> val((RDN_REPORT_ROWS(nb) + 1) * RDN_REPORT_VALUES, -1.0);
    EXPECT(rdn_snr(nullptr, nullptr, nullptr, 0, 1, 100, nullptr, nullptr, 20.f, 37.f, nb, nullptr, rep.data(), nullptr) ==
           RDN_EINVAL);
    EXPECT(rdn_snr(nullptr, nullptr, nullptr, 0, 0, 100, nullptr, nullptr, 20.f, 37.f, 65, nullptr, rep.data(), nullptr) ==
           RDN_EINVAL);
    EXPECT(rdn_snr(nullptr, nullptr, nullptr, 0, 0, 100, nullptr, nullptr, 20.f, 37.f, nb, nullptr, rep.data(), nullptr) ==
           RDN_OK);
    int row = -1;
    EXPECT(rdn_report_bin(20.f, 20.f, 37.f, nb, &row) == RDN_OK && row == 1);
    EXPECT(rdn_report_bin(37.f, 20.f, 37.f, nb, &row) == RDN_OK && row == nb + 1);
    EXPECT(rdn_report_bin(19.f, 20.f, 37.f, nb, &row) == RDN_OK && row == 0);
    EXPECT(rdn_report_bin(1.f, 2.f, 2.f, nb, &row) == RDN_EINVAL);
    // 1.5 in row 2's SNR_in (limb 4 holds the units: weight 2^(32 * 4 - 128)), -0.5 in the overflow row's
    int64_t* r2 = rep.data() + 2 * RDN_REPORT_ROW_WORDS + 4 * RDN_ACC_STRIDE;
    r2[4] = 1, r2[3] = (int64_t)1 << 31;
    rep[2 * RDN_REPORT_ROW_WORDS + RDN_REPORT_COUNT] = 1;
    int64_t* r4 = rep.data() + (nb + 1) * RDN_REPORT_ROW_WORDS + 4 * RDN_ACC_STRIDE;
    r4[3] = -((int64_t)1 << 31);
    rep[(nb + 1) * RDN_REPORT_ROW_WORDS + RDN_REPORT_COUNT] = 1;
    EXPECT(rdn_report_value(rep.data(), nb, val.data()) == RDN_OK);
    EXPECT(val[2 * RDN_REPORT_VALUES + 5] == 1.5 && val[(nb + 1) * RDN_REPORT_VALUES + 5] == -0.5);
    EXPECT(val[(nb + 2) * RDN_REPORT_VALUES] == 2.0 && val[(nb + 2) * RDN_REPORT_VALUES + 5] == 1.0);
    EXPECT(rdn_report_value(rep.data(), 0, val.data()) == RDN_EINVAL);
    EXPECT(rdn_report_value(nullptr, nb, val.data()) == RDN_EINVAL);
  }
  // PhysicsAwareLoss report: argument checks (before any HIP call) and the host conversion of an
  // exactly-sized report, an out-of-range word included
  {
    const int nb = 2;
    std::vector<int64_t> rep(RDN_PHYS_WORDS(nb), 0);
    std::vector<double> val((RDN_REPORT_ROWS(nb) + 1) * RDN_PHYS_VALUES, -1.0), per(6, 0.0);
    const float* f = (const float*)rep.data();       // never read: every call below fails its checks or has n = 0
    auto phys = [&](int64_t n, int64_t L, double a, double* per6, float lo, float hi, int nbins, int64_t* r) {
      return rdn_physics(f, f, f, 0, n, L, a, 0.05, 0.01, per6, nullptr, lo, hi, nbins, r, nullptr);
    };
    EXPECT(phys(1, 2, 0.1, per.data(), 20.f, 37.f, nb, rep.data()) == RDN_EINVAL);            // L < 3
    EXPECT(phys(1, 100, 0.1, per.data(), 20.f, 37.f, 65, rep.data()) == RDN_EINVAL);          // bad bins
    EXPECT(phys(1, 100, 0.1, per.data(), 37.f, 20.f, nb, rep.data()) == RDN_EINVAL);
    EXPECT(phys(1, 100, 0.1, nullptr, 20.f, 37.f, nb, nullptr) == RDN_EINVAL);                // nothing to write
    EXPECT(phys(1, 100, std::nan(""), per.data(), 20.f, 37.f, nb, rep.data()) == RDN_EINVAL); // non-finite weight
    EXPECT(rdn_physics(nullptr, nullptr, nullptr, 0, 1, 100, 0.1, 0.05, 0.01, per.data(), nullptr, 0.f, 0.f, 0, nullptr,
                       nullptr) == RDN_EINVAL);
    EXPECT(rdn_physics(nullptr, nullptr, nullptr, 0, 0, 100, 0.1, 0.05, 0.01, nullptr, nullptr, 20.f, 37.f, nb,
                       rep.data(), nullptr) == RDN_OK);
    // 2.25 in row 1's Total (quantity 4; limb 4 holds the units), 3 in row 2's PeakCount, and one
    // out-of-range Peak (quantity 2) in row 2
    int64_t* r1 = rep.data() + 1 * RDN_PHYS_ROW_WORDS;
    int64_t* r2 = rep.data() + 2 * RDN_PHYS_ROW_WORDS;
    r1[4 * RDN_ACC_STRIDE + 4] = 2, r1[4 * RDN_ACC_STRIDE + 3] = (int64_t)1 << 30, r1[RDN_PHYS_COUNT] = 1;
    r2[4 * RDN_ACC_STRIDE + 3] = (int64_t)1 << 31, r2[5 * RDN_ACC_STRIDE + 4] = 3, r2[2 * RDN_ACC_STRIDE + RDN_ACC_LIMBS] = 1;
    r2[RDN_PHYS_COUNT] = 2;
    EXPECT(rdn_physics_value(rep.data(), nb, val.data()) == RDN_OK);
    const double* t = val.data() + (nb + 2) * RDN_PHYS_VALUES;
    EXPECT(val[1 * RDN_PHYS_VALUES + 5] == 2.25 && val[2 * RDN_PHYS_VALUES + 5] == 0.5 && val[2 * RDN_PHYS_VALUES + 6] == 3.0);
    EXPECT(std::isnan(val[2 * RDN_PHYS_VALUES + 3]) && val[1 * RDN_PHYS_VALUES + 3] == 0.0);
    EXPECT(t[0] == 3.0 && t[5] == 2.75 && t[6] == 3.0 && std::isnan(t[3]) && t[1] == 0.0);
    EXPECT(rdn_physics_value(rep.data(), 0, val.data()) == RDN_EINVAL);
    EXPECT(rdn_physics_value(nullptr, nb, val.data()) == RDN_EINVAL);
  }

  // baseline filters: every refusal comes before any HIP call, for n = 0 too
  {
    std::vector<float> buf(64, 0.f);
    std::vector<double> tp(5, 0.2);
    const float* x = buf.data();
    float* y = buf.data() + 32;
    EXPECT(rdn_fir(x, y, 1, 16, nullptr, 5, nullptr, nullptr) == RDN_EINVAL);             // null taps
    EXPECT(rdn_fir(nullptr, nullptr, 0, 16, nullptr, 5, nullptr, nullptr) == RDN_EINVAL); // ... for n = 0 too
    EXPECT(rdn_fir(nullptr, y, 1, 16, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, nullptr, 1, 16, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, y, -1, 16, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, y, 1, 16, tp.data(), 4, nullptr, nullptr) == RDN_EINVAL);           // even
    EXPECT(rdn_fir(x, y, 1, 16, tp.data(), 0, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, y, 1, 16, tp.data(), -3, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, y, 0, 1000, tp.data(), RDN_FILTER_MAX_WINDOW + 2, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, y, 1, 4, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);            // L < w
    EXPECT(rdn_fir(x, y, 0, (int64_t)1 << 31, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);
    EXPECT(rdn_fir(x, buf.data() + 8, 1, 16, tp.data(), 5, nullptr, nullptr) == RDN_EINVAL);   // overlap
    EXPECT(rdn_fir(nullptr, nullptr, 0, 16, tp.data(), 5, nullptr, nullptr) == RDN_OK);
    EXPECT(rdn_fir(nullptr, nullptr, 0, ((int64_t)1 << 31) - 1, tp.data(), RDN_FILTER_MAX_WINDOW, nullptr, nullptr) == RDN_OK);
    EXPECT(rdn_median(nullptr, y, 1, 16, 5, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, -1, 16, 5, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, 1, 16, 6, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, 0, 16, 0, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, 0, 1000, 257, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, 1, 4, 5, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, y, 0, (int64_t)1 << 31, 5, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(x, buf.data() + 15, 1, 16, 5, nullptr) == RDN_EINVAL);
    EXPECT(rdn_median(nullptr, nullptr, 0, 16, 5, nullptr) == RDN_OK);
    EXPECT(std::strlen(rdn_last_error()) > 0);
  }

  check_haar_and_grad_args();
  check_potts_and_mad_args();
  check_bayes_args();
  check_once_per();
  check_chunks();
  check_overlaps();
  check_forward_geometry();

  if (fails) return 1;
  std::printf("host_check: arch %d dtype %d: %zu tensors, %zu bytes packed, all checks passed\n", arch, dtype,
              (size_t)n, bytes);
  return 0;
}
