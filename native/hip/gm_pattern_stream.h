// gm_pattern_stream.h — the core of the tests that stream the memtest pattern through memory
// (gm_memtest.hip over HBM, gm_hostlink.hip over pinned host memory): one bandwidth-bound kernel
// template in the form of k_read_chunk / k_copy_chunk (gm_probe.hip), its error path, and the
// host helpers around a launch. Anonymous namespace, as gm_probe_common.h.
//
// A contiguous chunk per 256-thread block (gm_pattern_chunks.h), 16 B per lane per access, U
// nontemporal loads in flight per lane before the first compare, a 16-byte tail loop. The
// expected value of a word is a pure function of its global byte offset (gm_memtest_pattern.h),
// so nothing but the buffers themselves is read. The error path costs one OR per word on clean
// data: each lane ORs expected ^ got of its 2 U words into one flag and only a lane whose flag is
// nonzero looks at the words again, in a cold report().
#pragma once
#include "gm_probe.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include <type_traits>

#include "gm_memtest_pattern.h"
#include "gm_pattern_chunks.h"
#include "gm_probe_common.h"

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// kWrite: buf = P.  kCheck: buf is compared with P.  kCheckInvert: buf is compared with P and
// ~P written over the same words.  kCopy: `from` is compared with P and what was read goes to buf.
enum { kWrite = 0, kCheck = 1, kCheckInvert = 2, kCopy = 3 };

struct DevResult {
  unsigned long long words, bits, stuck;
  unsigned int claims, pad;
  gm_memtest_record_t rec[GM_MEMTEST_MAX_RECORDS];
};

struct Args {
  uint64_t base;  // global byte offset of buf[0] in the region
  uint64_t seed;
  uint64_t inv;   // 0 or ~0: XORed into the pattern value
  uint32_t pass;
  uint64_t flip_offset = 0, flip_mask = 0;  // kFlip writers: word at flip_offset ^= flip_mask
};

template <uint32_t P>
__device__ __forceinline__ uint64_t expect(const Args& a, uint64_t o) {
  return gm_memtest_expected(P, a.seed, a.pass, o) ^ a.inv;
}

// Cold: entered per mismatching word only.
__device__ __noinline__ void report(DevResult* res, uint64_t o, uint64_t e, uint64_t g,
                                    uint32_t pattern, uint32_t pass) {
  const uint64_t x = e ^ g;
  atomicAdd(&res->words, 1ull);
  atomicAdd(&res->bits, (unsigned long long)__popcll(x));
  atomicOr(&res->stuck, (unsigned long long)x);
  const unsigned int slot = atomicAdd(&res->claims, 1u);
  if (slot < GM_MEMTEST_MAX_RECORDS) {
    gm_memtest_record_t* r = &res->rec[slot];
    r->offset = o;
    r->expected = e;
    r->got = g;
    r->pattern = pattern;
    r->pass = pass;
  }
}

template <uint32_t P>
__device__ __forceinline__ void check_pair(DevResult* res, const Args& a, uint64_t o, u64x2 got) {
  const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
  if (got.x != e0) report(res, o, e0, got.x, P, a.pass);
  if (got.y != e1) report(res, o + 8, e1, got.y, P, a.pass);
}

// Stores v, the element at global byte offset o; with kFlip the negative control goes in first.
template <bool kNt, bool kFlip>
__device__ __forceinline__ void put(u64x2* p, const Args& a, uint64_t o, u64x2 v) {
  if constexpr (kFlip) {
    v.x ^= o == a.flip_offset ? a.flip_mask : 0;
    v.y ^= o + 8 == a.flip_offset ? a.flip_mask : 0;
  }
  if constexpr (kNt)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// n and per_block count 16-byte elements. `from` is kCopy's source and unused otherwise: the
// in-place mode kCheckInvert reads and writes through the one pointer buf, so no pair of
// __restrict__ pointers to the same words exists that would let its stores (whose value does
// not depend on what was read) move above its loads.
template <uint32_t P, int kMode, int U, bool kNtStore, bool kFlip>
__global__ __launch_bounds__(256) void k_pattern_stream(u64x2* __restrict__ buf,
                                                        const u64x2* __restrict__ from, size_t n,
                                                        size_t per_block, Args a, DevResult* res) {
  const u64x2* src = kMode == kCopy ? from : buf;
  const size_t begin = (size_t)blockIdx.x * per_block;
  const size_t end = begin + per_block < n ? begin + per_block : n;
  size_t i = begin + threadIdx.x;
  for (; i + (size_t)(U - 1) * 256 < end; i += (size_t)U * 256) {
    if constexpr (kMode == kWrite) {
#pragma unroll
      for (int c = 0; c < U; ++c) {
        const uint64_t o = a.base + (uint64_t)(i + c * 256) * 16;
        const u64x2 v = {expect<P>(a, o), expect<P>(a, o + 8)};
        put<kNtStore, kFlip>(&buf[i + c * 256], a, o, v);
      }
    } else {
      u64x2 r[U];
#pragma unroll
      for (int c = 0; c < U; ++c) r[c] = __builtin_nontemporal_load(&src[i + c * 256]);
      uint64_t flag = 0;
#pragma unroll
      for (int c = 0; c < U; ++c) {
        const uint64_t o = a.base + (uint64_t)(i + c * 256) * 16;
        const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
        flag |= (r[c].x ^ e0) | (r[c].y ^ e1);
        if constexpr (kMode == kCheckInvert) {
          const u64x2 v = {~e0, ~e1};
          put<kNtStore, kFlip>(&buf[i + c * 256], a, o, v);
        } else if constexpr (kMode == kCopy) {
          put<kNtStore, kFlip>(&buf[i + c * 256], a, o, r[c]);
        }
      }
      if (flag != 0) {
#pragma unroll  // constant indices keep r[] in registers
        for (int c = 0; c < U; ++c)
          check_pair<P>(res, a, a.base + (uint64_t)(i + c * 256) * 16, r[c]);
      }
    }
  }
  for (; i < end; i += 256) {  // at most one element per lane, in the main loop's cache policy
    const uint64_t o = a.base + (uint64_t)i * 16;
    const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
    if constexpr (kMode == kWrite) {
      const u64x2 v = {e0, e1};
      put<kNtStore, kFlip>(&buf[i], a, o, v);
    } else {
      const u64x2 g = __builtin_nontemporal_load(&src[i]);
      if constexpr (kMode == kCheckInvert) {
        const u64x2 v = {~e0, ~e1};
        put<kNtStore, kFlip>(&buf[i], a, o, v);
      } else if constexpr (kMode == kCopy) {
        put<kNtStore, kFlip>(&buf[i], a, o, g);
      }
      if (((g.x ^ e0) | (g.y ^ e1)) != 0) check_pair<P>(res, a, o, g);
    }
  }
}

// Everything a launch needs but the template arguments, which the caller's switch supplies:
// each test instantiates only the kernels it ships.
struct StreamLaunch {
  gm_pattern_chunks_t chunks;
  hipStream_t s;
  void* buf;
  const void* from;
  size_t n;
  Args a;
  DevResult* res;
  template <uint32_t P, int kMode, int U, bool kNtStore, bool kFlip>
  void run() const {
    hipLaunchKernelGGL((k_pattern_stream<P, kMode, U, kNtStore, kFlip>), dim3(chunks.grid),
                       dim3(256), 0, s, (u64x2*)buf, (const u64x2*)from, n,
                       (size_t)chunks.per_block, a, res);
  }
};

// Calls f(std::integral_constant<uint32_t, P>) for the one pattern bit P; false for anything else.
template <class F>
bool dispatch_pattern(uint32_t pattern, F f) {
  switch (pattern) {
    case GM_MEMTEST_ADDR: f(std::integral_constant<uint32_t, GM_MEMTEST_ADDR>{}); return true;
    case GM_MEMTEST_SOLID: f(std::integral_constant<uint32_t, GM_MEMTEST_SOLID>{}); return true;
    case GM_MEMTEST_CHECKER: f(std::integral_constant<uint32_t, GM_MEMTEST_CHECKER>{}); return true;
    case GM_MEMTEST_WALK: f(std::integral_constant<uint32_t, GM_MEMTEST_WALK>{}); return true;
    case GM_MEMTEST_RANDOM: f(std::integral_constant<uint32_t, GM_MEMTEST_RANDOM>{}); return true;
    default: return false;
  }
}

inline bool one_pattern(uint32_t p) {
  return dispatch_pattern(p, [](auto) {});
}

inline bool buffer_ok(const void* ptr, uint64_t bytes, uint32_t pattern, uint64_t base_offset) {
  return ptr != nullptr && ((uintptr_t)ptr & 15) == 0 && bytes != 0 && (bytes & 15) == 0 &&
         (base_offset & 7) == 0 && one_pattern(pattern);
}

inline void export_errors(const DevResult& h, gm_memtest_result_t* out) {
  out->words_in_error = h.words;
  out->bit_errors = h.bits;
  out->stuck_mask = h.stuck;
  out->records_filled = h.claims < GM_MEMTEST_MAX_RECORDS ? h.claims : GM_MEMTEST_MAX_RECORDS;
  for (uint32_t i = 0; i < out->records_filled; ++i) out->records[i] = h.rec[i];
}

// One verifying launch over `bytes` of caller-owned memory, waited for: launch(DevResult*)
// enqueues the kernel on s and returns its launch error.
template <class Launch>
int checked_launch(hipStream_t s, uint64_t bytes, gm_memtest_result_t* out, Launch launch) {
  DevBuf dres;
  GM_CHECK(dres.alloc(sizeof(DevResult)));
  GM_CHECK(hipMemsetAsync(dres.p, 0, sizeof(DevResult), s));
  if (int e = launch((DevResult*)dres.p)) return e;
  DevResult h;
  GM_CHECK(hipMemcpyAsync(&h, dres.p, sizeof(h), hipMemcpyDeviceToHost, s));
  GM_CHECK(hipStreamSynchronize(s));
  out->bytes_tested = bytes;
  export_errors(h, out);
  return 0;
}

// The negative control for device memory: the 64-bit word at `at` ^= mask.
inline int xor_device_word(void* at, uint64_t mask) {
  uint64_t word = 0;
  GM_CHECK(hipMemcpy(&word, at, 8, hipMemcpyDeviceToHost));
  word ^= mask;
  GM_CHECK(hipMemcpy(at, &word, 8, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace
