// gm_memtest.hip — HBM pattern test for gfx950: does the VRAM hold what is written to it?
//
// Three bandwidth-bound kernels from one template, in the form of k_read_chunk / k_copy_chunk
// (gm_probe.hip): a contiguous chunk per 256-thread block, 16 B per lane per access, 8 nontemporal
// loads in flight per lane before the compares, a 16-byte tail loop, CUs × 2 blocks.
//   fill           writes P (or ~P)
//   verify_invert  reads and checks P, writes ~P over the same words
//   verify         reads and checks
// The expected value of a word is a pure function of its global byte offset in the test region
// (gm_memtest_pattern.h), so nothing but the buffer itself is read. All three walk the region in
// the same order: what was written first is read first, after everything else has gone through
// the caches. Inside one launch the blocks run in whatever order the dispatcher picks; there is
// no ascending or descending direction as in a CPU march test.
//
// The error path costs one OR per word on clean memory: each lane ORs expected ^ got of its 16
// words into one flag and only a lane whose flag is nonzero looks at the words again.
#include "gm_probe.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <deque>

#include "gm_memtest_pattern.h"
#include "gm_probe_common.h"

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

enum { kFill = 0, kVerify = 1, kVerifyInvert = 2 };
constexpr int kInFlight = 8;          // 16-B accesses per lane per unrolled step
constexpr int kBlocksPerCu = 2;       // gm_probe_hbm_read's default geometry
constexpr size_t kStepElems = (size_t)kInFlight * 256;  // 16-B elements per block per step

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
};

template <uint32_t P>
__device__ __forceinline__ uint64_t expect(const Args& a, uint64_t o) {
  return gm_memtest_expected(P, a.seed, a.pass, o) ^ a.inv;
}

// Cold: entered per mismatching word only.
__device__ __noinline__ void report(DevResult* res, uint64_t o, uint64_t e, uint64_t g,
                                    uint32_t pattern, uint32_t pass) {
  const uint64_t x = e ^ g;
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
__device__ __forceinline__ uint32_t check_pair(DevResult* res, const Args& a, uint64_t o,
                                               u64x2 got) {
  uint32_t bad = 0;
  const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
  if (got.x != e0) {
    report(res, o, e0, got.x, P, a.pass);
    ++bad;
  }
  if (got.y != e1) {
    report(res, o + 8, e1, got.y, P, a.pass);
    ++bad;
  }
  return bad;
}

template <bool kNt>
__device__ __forceinline__ void put(u64x2* p, u64x2 v) {
  if constexpr (kNt)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// n and per_block count 16-byte elements.
template <uint32_t P, int kMode, bool kNtStore>
__global__ __launch_bounds__(256) void k_memtest(u64x2* __restrict__ buf, size_t n,
                                                 size_t per_block, Args a, DevResult* res) {
  const size_t begin = (size_t)blockIdx.x * per_block;
  const size_t end = begin + per_block < n ? begin + per_block : n;
  uint32_t bad = 0;
  size_t i = begin + threadIdx.x;
  for (; i + (kInFlight - 1) * 256 < end; i += kStepElems) {
    if constexpr (kMode == kFill) {
#pragma unroll
      for (int c = 0; c < kInFlight; ++c) {
        const uint64_t o = a.base + (uint64_t)(i + c * 256) * 16;
        const u64x2 v = {expect<P>(a, o), expect<P>(a, o + 8)};
        put<kNtStore>(&buf[i + c * 256], v);
      }
    } else {
      u64x2 r[kInFlight];
#pragma unroll
      for (int c = 0; c < kInFlight; ++c) r[c] = __builtin_nontemporal_load(&buf[i + c * 256]);
      uint64_t flag = 0;
#pragma unroll
      for (int c = 0; c < kInFlight; ++c) {
        const uint64_t o = a.base + (uint64_t)(i + c * 256) * 16;
        const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
        flag |= (r[c].x ^ e0) | (r[c].y ^ e1);
        if constexpr (kMode == kVerifyInvert) {
          const u64x2 v = {~e0, ~e1};
          put<kNtStore>(&buf[i + c * 256], v);
        }
      }
      if (flag != 0) {
#pragma unroll  // constant indices keep r[] in registers
        for (int c = 0; c < kInFlight; ++c)
          bad += check_pair<P>(res, a, a.base + (uint64_t)(i + c * 256) * 16, r[c]);
      }
    }
  }
  for (; i < end; i += 256) {
    const uint64_t o = a.base + (uint64_t)i * 16;
    const uint64_t e0 = expect<P>(a, o), e1 = expect<P>(a, o + 8);
    if constexpr (kMode == kFill) {
      const u64x2 v = {e0, e1};
      buf[i] = v;
    } else {
      const u64x2 g = buf[i];
      if constexpr (kMode == kVerifyInvert) {
        const u64x2 v = {~e0, ~e1};
        buf[i] = v;
      }
      if (((g.x ^ e0) | (g.y ^ e1)) != 0) bad += check_pair<P>(res, a, o, g);
    }
  }
  if constexpr (kMode != kFill) {
    // one atomic per wave, and only from a wave that saw a mismatch (as k_count_diff does)
    unsigned long long local = bad;
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, kWave);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(&res->words, local);
  }
}

std::atomic<int> g_nt_store{1};

struct Geometry {
  unsigned int grid;
  size_t per_block;
};

// CUs × kBlocksPerCu blocks, each a whole number of unrolled steps; blocks whose chunk would
// start past the end are not launched.
Geometry geometry(size_t n, int cus) {
  const size_t blocks = (size_t)(cus > 0 ? cus : 1) * kBlocksPerCu;
  const size_t per_block = ((n + blocks - 1) / blocks + kStepElems - 1) / kStepElems * kStepElems;
  return {(unsigned int)((n + per_block - 1) / per_block), per_block};
}

template <uint32_t P>
void launch_p(int mode, bool nt, const Geometry& g, hipStream_t s, u64x2* buf, size_t n,
              const Args& a, DevResult* res) {
  const dim3 grid(g.grid), block(256);
  if (mode == kFill) {
    if (nt)
      hipLaunchKernelGGL((k_memtest<P, kFill, true>), grid, block, 0, s, buf, n, g.per_block, a,
                         res);
    else
      hipLaunchKernelGGL((k_memtest<P, kFill, false>), grid, block, 0, s, buf, n, g.per_block, a,
                         res);
  } else if (mode == kVerifyInvert) {
    if (nt)
      hipLaunchKernelGGL((k_memtest<P, kVerifyInvert, true>), grid, block, 0, s, buf, n,
                         g.per_block, a, res);
    else
      hipLaunchKernelGGL((k_memtest<P, kVerifyInvert, false>), grid, block, 0, s, buf, n,
                         g.per_block, a, res);
  } else {
    hipLaunchKernelGGL((k_memtest<P, kVerify, false>), grid, block, 0, s, buf, n, g.per_block, a,
                       res);
  }
}

int launch(int mode, uint32_t pattern, int cus, hipStream_t s, void* ptr, uint64_t bytes,
           const Args& a, DevResult* res) {
  const size_t n = bytes / 16;
  const Geometry g = geometry(n, cus);
  const bool nt = g_nt_store.load() != 0;
  u64x2* buf = (u64x2*)ptr;
  switch (pattern) {
    case GM_MEMTEST_ADDR: launch_p<GM_MEMTEST_ADDR>(mode, nt, g, s, buf, n, a, res); break;
    case GM_MEMTEST_SOLID: launch_p<GM_MEMTEST_SOLID>(mode, nt, g, s, buf, n, a, res); break;
    case GM_MEMTEST_CHECKER: launch_p<GM_MEMTEST_CHECKER>(mode, nt, g, s, buf, n, a, res); break;
    case GM_MEMTEST_WALK: launch_p<GM_MEMTEST_WALK>(mode, nt, g, s, buf, n, a, res); break;
    case GM_MEMTEST_RANDOM: launch_p<GM_MEMTEST_RANDOM>(mode, nt, g, s, buf, n, a, res); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

bool one_pattern(uint32_t p) {
  return p == GM_MEMTEST_ADDR || p == GM_MEMTEST_SOLID || p == GM_MEMTEST_CHECKER ||
         p == GM_MEMTEST_WALK || p == GM_MEMTEST_RANDOM;
}

bool buffer_ok(const void* ptr, uint64_t bytes, uint32_t pattern, uint64_t base_offset) {
  return ptr != nullptr && ((uintptr_t)ptr & 15) == 0 && bytes != 0 && (bytes & 15) == 0 &&
         (base_offset & 7) == 0 && one_pattern(pattern);
}

int current_cus(int* cus) {
  int dev = 0;
  GM_CHECK(hipGetDevice(&dev));
  GM_CHECK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
  return 0;
}

void export_errors(const DevResult& h, gm_memtest_result_t* out) {
  out->words_in_error = h.words;
  out->bit_errors = h.bits;
  out->stuck_mask = h.stuck;
  out->records_filled = h.claims < GM_MEMTEST_MAX_RECORDS ? h.claims : GM_MEMTEST_MAX_RECORDS;
  for (uint32_t i = 0; i < out->records_filled; ++i) out->records[i] = h.rec[i];
}

struct Piece {
  DevBuf buf;
  uint64_t bytes = 0, base = 0;
};

}  // namespace

extern "C" {

int gm_probe_mem_info(int dev, uint64_t* free_bytes, uint64_t* total_bytes) {
  *free_bytes = *total_bytes = 0;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  size_t f = 0, t = 0;
  GM_CHECK(hipMemGetInfo(&f, &t));
  *free_bytes = f;
  *total_bytes = t;
  return 0;
}

int gm_probe_memtest_expected(uint32_t pattern, uint64_t seed, uint32_t pass,
                              uint64_t base_offset, uint64_t n_words, uint64_t* out) {
  if (!one_pattern(pattern) || (base_offset & 7) || (n_words && !out))
    return (int)hipErrorInvalidValue;
  for (uint64_t i = 0; i < n_words; ++i)
    out[i] = gm_memtest_expected(pattern, seed, pass, base_offset + 8 * i);
  return 0;
}

int gm_probe_memtest_store_variant(int nontemporal) {
  if (nontemporal == 0 || nontemporal == 1) return g_nt_store.exchange(nontemporal);
  return g_nt_store.load();
}

int gm_probe_memtest_fill(void* ptr, uint64_t bytes, uint32_t pattern, int invert, uint64_t seed,
                          uint32_t pass, uint64_t base_offset, void* stream) {
  if (!buffer_ok(ptr, bytes, pattern, base_offset)) return (int)hipErrorInvalidValue;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass};
  return launch(kFill, pattern, cus, (hipStream_t)stream, ptr, bytes, a, nullptr);
}

int gm_probe_memtest_verify(void* ptr, uint64_t bytes, uint32_t pattern, int invert,
                            int write_inverse, uint64_t seed, uint32_t pass,
                            uint64_t base_offset, void* stream, gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!buffer_ok(ptr, bytes, pattern, base_offset)) return (int)hipErrorInvalidValue;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  hipStream_t s = (hipStream_t)stream;
  DevBuf dres;
  GM_CHECK(dres.alloc(sizeof(DevResult)));
  GM_CHECK(hipMemsetAsync(dres.p, 0, sizeof(DevResult), s));
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass};
  if (int e = launch(write_inverse ? kVerifyInvert : kVerify, pattern, cus, s, ptr, bytes, a,
                     (DevResult*)dres.p))
    return e;
  DevResult h;
  GM_CHECK(hipMemcpyAsync(&h, dres.p, sizeof(h), hipMemcpyDeviceToHost, s));
  GM_CHECK(hipStreamSynchronize(s));
  out->bytes_tested = bytes;
  export_errors(h, out);
  return 0;
}

int gm_probe_memtest(int dev, uint64_t bytes, uint64_t chunk_bytes, uint32_t pattern_mask,
                     int passes, uint64_t seed, uint64_t flip_offset, uint64_t flip_mask,
                     gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (bytes == 0 || (bytes & 15) || (chunk_bytes & 15) || pattern_mask == 0 ||
      (pattern_mask & ~(uint32_t)GM_MEMTEST_ALL) || passes <= 0)
    return (int)hipErrorInvalidValue;
  if (flip_mask && ((flip_offset & 7) || flip_offset + 8 > bytes || flip_offset + 8 < 8))
    return (int)hipErrorInvalidValue;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  const auto t0 = std::chrono::steady_clock::now();
  if (chunk_bytes == 0) chunk_bytes = 8ull << 30;

  // the region: allocations of at most chunk_bytes, each with its global base offset
  std::deque<Piece> pieces;  // a deque never relocates its owning elements
  uint64_t have = 0;
  hipError_t alloc_err = hipSuccess;
  while (have < bytes) {
    uint64_t want = bytes - have < chunk_bytes ? bytes - have : chunk_bytes;
    const uint64_t floor = want < (256ull << 20) ? want : (256ull << 20);
    pieces.emplace_back();
    Piece& p = pieces.back();
    for (;;) {
      alloc_err = p.buf.alloc(want);
      if (alloc_err == hipSuccess) break;
      (void)hipGetLastError();
      p.buf.p = nullptr;
      want = (want / 2) & ~15ull;
      if (want < floor) break;
    }
    if (alloc_err != hipSuccess) {
      pieces.pop_back();
      break;
    }
    p.bytes = want;
    p.base = have;
    have += want;
  }
  if (pieces.empty()) return (int)(alloc_err != hipSuccess ? alloc_err : hipErrorOutOfMemory);

  DevBuf dres;
  GM_CHECK(dres.alloc(sizeof(DevResult)));
  GM_CHECK(hipMemset(dres.p, 0, sizeof(DevResult)));
  Events ev;
  GM_CHECK(ev.create());
  {
    // untimed first launch: the code object is loaded here, not between a timed pair of events
    const uint64_t warm = pieces[0].bytes < 65536 ? pieces[0].bytes : 65536;
    if (int e = launch(kFill, GM_MEMTEST_SOLID, cus, nullptr, pieces[0].buf.p, warm,
                       Args{0, seed, 0, 0}, nullptr))
      return e;
    GM_CHECK(hipStreamSynchronize(nullptr));
  }
  double ms_kind[3] = {0, 0, 0};
  uint64_t launches_kind[3] = {0, 0, 0};  // whole-region sweeps per kind

  // one sweep of the whole region with one kind of kernel, timed by an event pair
  auto sweep = [&](int mode, uint32_t pattern, bool invert, uint32_t pass) -> int {
    int e = (int)hipEventRecord(ev.e0, nullptr);
    for (size_t k = 0; k < pieces.size() && !e; ++k) {
      const Args a{pieces[k].base, seed, invert ? ~0ull : 0ull, pass};
      e = launch(mode, pattern, cus, nullptr, pieces[k].buf.p, pieces[k].bytes, a,
                 (DevResult*)dres.p);
    }
    if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
    if (!e) e = (int)hipEventSynchronize(ev.e1);
    float ms = 0;
    if (!e) e = (int)hipEventElapsedTime(&ms, ev.e0, ev.e1);
    ms_kind[mode] += ms;
    ++launches_kind[mode];
    return e;
  };
  auto flip = [&]() -> int {
    for (Piece& p : pieces) {
      if (flip_offset < p.base || flip_offset + 8 > p.base + p.bytes) continue;
      char* at = (char*)p.buf.p + (flip_offset - p.base);
      uint64_t word = 0;
      GM_CHECK(hipMemcpy(&word, at, 8, hipMemcpyDeviceToHost));
      word ^= flip_mask;
      GM_CHECK(hipMemcpy(at, &word, 8, hipMemcpyHostToDevice));
    }
    return 0;
  };

  int e = 0;
  for (uint32_t pattern = 1; pattern <= GM_MEMTEST_RANDOM && !e; pattern <<= 1) {
    if (!(pattern_mask & pattern)) continue;
    for (int pass = 0; pass < passes && !e; ++pass) {
      e = sweep(kFill, pattern, false, (uint32_t)pass);
      if (!e && flip_mask) e = flip();
      if (!e) e = sweep(kVerifyInvert, pattern, false, (uint32_t)pass);
      if (!e) e = sweep(kVerify, pattern, true, (uint32_t)pass);
    }
  }
  if (e) return e;
  DevResult h;
  GM_CHECK(hipMemcpy(&h, dres.p, sizeof(h), hipMemcpyDeviceToHost));
  export_errors(h, out);
  out->bytes_tested = have;
  out->allocations = (uint32_t)pieces.size();
  const double b = (double)have;
  if (ms_kind[kFill] > 0) out->write_gbps = b * launches_kind[kFill] / (ms_kind[kFill] * 1e-3) / 1e9;
  if (ms_kind[kVerify] > 0)
    out->read_gbps = b * launches_kind[kVerify] / (ms_kind[kVerify] * 1e-3) / 1e9;
  if (ms_kind[kVerifyInvert] > 0)
    out->rw_gbps = 2.0 * b * launches_kind[kVerifyInvert] / (ms_kind[kVerifyInvert] * 1e-3) / 1e9;
  out->seconds =
      std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

}  // extern "C"
