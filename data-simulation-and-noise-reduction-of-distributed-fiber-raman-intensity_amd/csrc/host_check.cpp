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
// rdn_physics_value); and the argument checks of the baseline filters (rdn_fir, rdn_median).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/raman_mi355x.h"

static int fails = 0;
#define EXPECT(c)                                                     \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "host_check: FAILED %s (line %d)\n", #c, __LINE__); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

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

  if (fails) return 1;
  std::printf("host_check: arch %d dtype %d: %zu tensors, %zu bytes packed, all checks passed\n", arch, dtype,
              (size_t)n, bytes);
  return 0;
}
