// gm_probe_common.h — shared by every gfx950 probe translation unit (PROBE_SRC in native/Makefile:
// gm_probe.hip includes it itself, the others through gm_pattern_stream.h, gm_gemm_shared.h,
// gm_cuscan_frame.h or gm_atomics_dev.h) and the
// block-scaled MFMA experiment: vector types, device selection guard, error macro, owning device /
// pinned buffer, stream and events, and the two clocks (event pair, host monotonic).
// Everything is in an anonymous namespace: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>

namespace {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;

struct DeviceGuard {
  int prev = 0;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
  }
  ~DeviceGuard() {
    if (ok) (void)hipSetDevice(prev);
  }
};

#define GM_CHECK(x)                        \
  do {                                     \
    hipError_t e__ = (x);                  \
    if (e__ != hipSuccess) return (int)e__; \
  } while (0)

// Compute units of the current device.
inline int current_cus(int* cus) {
  int dev = 0;
  GM_CHECK(hipGetDevice(&dev));
  GM_CHECK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
  return 0;
}

// Owning handles for the host entry points (released on every return path).
struct DevBuf {
  void* p = nullptr;
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
struct PinnedBuf {
  void* p = nullptr;
  hipError_t alloc(size_t bytes) {
    return hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
  }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};
struct Stream {
  hipStream_t s = nullptr;
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct Event {
  hipEvent_t e = nullptr;
  hipError_t create() { return hipEventCreate(&e); }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};
struct Events {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t create() {
    hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  ~Events() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// Milliseconds between two recorded events, e1 already waited for; *ms is untouched on error.
inline int elapsed_ms(hipEvent_t e0, hipEvent_t e1, float* ms) {
  return (int)hipEventElapsedTime(ms, e0, e1);
}

// Monotonic host seconds; only differences mean anything.
inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace
