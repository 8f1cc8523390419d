// Host-side launch helpers shared by the kernel launchers: per-device, thread-safe caches.
//
// The ABI is re-entrant (include/raman_mi355x.h): launches may come from several threads and for
// streams of different devices.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) and the CU count
// are per device, so both caches are keyed by the device that owns the launch stream (the opt-in by the
// kernel too) and guarded by one mutex (taken once per (kernel, device) pair on the slow path; lock-free afterwards).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>

namespace rdn {

constexpr int MAX_DEVICES = 64;

// device that executes work enqueued on `s` (the current device for the null stream)
inline int stream_device(hipStream_t s) {
  int dev = 0;
  if (s) {
    hipDevice_t d;
    if (hipStreamGetDevice(s, &d) == hipSuccess) return (int)d;
  }
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  return dev;
}

// Once per (kernel, device): the bookkeeping of ensure_dynamic_lds, apart from its HIP call.  The key is
// the kernel's host address: an append-only table of {kernel, one bit per device}, scanned without a lock
// (an entry is published by `used`, a device's bit by `devices`) and appended under the mutex.
struct OnceTable {
  static constexpr int CAPACITY = 256;      // kernels that ever asked (about 60 take the LDS opt-in)
  struct Entry {
    const void* fn = nullptr;
    std::atomic<uint64_t> devices{0};
  };
  static_assert(MAX_DEVICES <= 64, "one bit per device");
  Entry entries[CAPACITY];
  std::atomic<int> used{0};
  std::mutex mutex;
};

// set() for the pair (fn, dev), unless an earlier set() for it succeeded: a failed one leaves the pair
// unset, so the next call tries again.  A full table is an error (the opt-in is never skipped).
template <class Set>
inline hipError_t once_per(OnceTable& t, const void* fn, int dev, Set set) {
  if (!fn || dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidValue;
  const uint64_t bit = (uint64_t)1 << dev;
  const auto find = [&](int used) -> OnceTable::Entry* {
    for (int i = 0; i < used; ++i)
      if (t.entries[i].fn == fn) return &t.entries[i];
    return nullptr;
  };
  OnceTable::Entry* e = find(t.used.load(std::memory_order_acquire));
  if (e && (e->devices.load(std::memory_order_acquire) & bit)) return hipSuccess;
  std::lock_guard<std::mutex> lock(t.mutex);
  const int used = t.used.load(std::memory_order_relaxed);
  if (!e && !(e = find(used))) {
    if (used == OnceTable::CAPACITY) return hipErrorOutOfMemory;
    e = &t.entries[used];
    e->fn = fn;
    t.used.store(used + 1, std::memory_order_release);
  }
  if (e->devices.load(std::memory_order_relaxed) & bit) return hipSuccess;
  const hipError_t err = set();
  if (err == hipSuccess) e->devices.fetch_or(bit, std::memory_order_release);
  return err;
}

// Allow `bytes` of dynamic LDS for kernel `fn` on device `dev` (once per pair).
inline hipError_t ensure_dynamic_lds(const void* fn, int bytes, int dev) {
  static OnceTable table;
  return once_per(table, fn, dev, [&] {
    int cur = 0;
    hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return e;
    if (cur != dev && (e = hipSetDevice(dev)) != hipSuccess) return e;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (cur != dev) {
      const hipError_t e2 = hipSetDevice(cur);
      if (e == hipSuccess) e = e2;
    }
    return e;
  });
}

// Copy `bytes` (<= 16) of status words from the device to `out` behind the work on `s` and wait for
// it: through a 16-byte pinned buffer of the calling thread (a copy into pageable memory takes the
// runtime's staging path, ≈ 20 µs more per call of the batch-1 loop).  The buffer is allocated on
// the thread's first read and kept (16 B per thread that ever read a status word); stack memory if
// the allocation fails.
inline hipError_t read_words(void* out, const void* dev_words, size_t bytes, hipStream_t s) {
  thread_local void* pinned = nullptr;
  thread_local bool tried = false;
  if (!tried) {
    tried = true;
    if (hipHostMalloc(&pinned, 16, hipHostMallocPortable) != hipSuccess) {
      pinned = nullptr;
      (void)hipGetLastError();
    }
  }
  if (bytes > 16) return hipErrorInvalidValue;
  void* dst = pinned ? pinned : out;
  hipError_t e = hipMemcpyAsync(dst, dev_words, bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess && pinned) memcpy(out, pinned, bytes);
  return e;
}

// The meters' clean reference is fp32 or fp64: f(clean as a pointer of its own type).
template <class F>
inline hipError_t with_clean(const void* clean, bool clean_f64, F f) {
  return clean_f64 ? f((const double*)clean) : f((const float*)clean);
}

// [0, n) in consecutive pieces of at most `chunk`: f(n0, nn) for the nn that start at n0.  A chunk below 1
// is refused without a call of f (hipErrorInvalidValue): the walk would not advance, or would run backwards.
template <class F>
inline hipError_t for_chunks(int64_t n, int64_t chunk, F f) {
  if (chunk < 1) return hipErrorInvalidValue;
  for (int64_t n0 = 0; n0 < n; n0 += chunk) f(n0, n - n0 < chunk ? n - n0 : chunk);
  return hipSuccess;
}

// Workgroups per spectrum of a kernel whose tiles own T positions each: the exact ceil(L / T), computed in
// 64 bits (in `int`, L + T - 1 wraps for the longest admitted rows, L > 2^31 - T).  For 1 <= L < 2^31 and
// T >= 1 the result is positive and fits `int`.
inline int64_t tiles_of(int64_t L, int64_t T) { return L / T + (L % T != 0); }

// spectra of one launch of a kernel that runs `tiles` workgroups per spectrum: their tiles fill grid.x
// (0, which launch_chunks refuses, for a tile count that is not positive)
inline int64_t tiles_chunk(int64_t tiles) { return tiles < 1 ? 0 : 0x7fffffff / tiles; }

// Walks a batch of n workgroups (one per spectrum) in launches of at most 2^31 - 1, the grid's limit in
// x: launch(n0, nn) enqueues the nn of them that start at n0.  (`chunk`: fewer spectra per launch, for a
// kernel that runs several workgroups per spectrum: tiles_chunk.)
template <class Launch>
inline hipError_t launch_chunks(int64_t n, Launch launch, int64_t chunk = 0x7fffffff) {
  const hipError_t e = for_chunks(n, chunk, launch);
  return e != hipSuccess ? e : hipGetLastError();
}

// the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte (an empty range shares none)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return abytes && bbytes && x < y + bbytes && y < x + abytes;
}

// Compute units of device `dev` (0 if the query fails), cached per device.
inline int device_cus(int dev) {
  static std::atomic<int> cus[MAX_DEVICES];
  if (dev < 0 || dev >= MAX_DEVICES) return 0;
  int v = cus[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  cus[dev].store(v, std::memory_order_relaxed);
  return v;
}

}  // namespace rdn
