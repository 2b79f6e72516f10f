// gm_cachescan.hip — per-CU cache scan for gfx950: which CU's vector L1, which XCC's L2, which
// scalar data cache or instruction cache hands back a wrong word?
//
// One kernel, k_cachescan, in the CU scan's frame (gm_cuscan_frame.h): a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU. Four
// known-answer tests of 4 signature words per thread; the data formulas are gm_cachescan_ref.h
// (shared with the host, written out in gm_probe.h).
//
// Block b owns segment b of the arena (GM_CACHESCAN_SEG_BYTES) and no other byte of it, so no
// result depends on where a block runs and no block waits for another. A word is stored as
// pattern ^ key(b) and the key is removed before the fold: the signature does not depend on b,
// and a line served from another block's segment decodes wrongly.
//
// The loads: `plain` is a global_load_dword, which allocates in the CU's L1; `bypass32` is the
// agent-scope relaxed atomic load (global_load_dword sc1) and `bypass128` the 16-byte nontemporal
// load (global_load_dwordx4 nt), which the L2 serves. All stores are plain and keep the line in
// the XCC's L2.
//
// Residency is observed, never judged: thread 0 stores the shader-clock counts of each test's
// first and last pass to timing[block][test][2], and nothing reads them but the report.
#include "gm_cachescan_ref.h"

#include "gm_cuscan_frame.h"

#include <algorithm>

namespace {

struct Bufs {
  uint32_t* arena;                  // gridDim.x segments
  const uint32_t* table;            // the scalar test's, GM_CACHESCAN_TABLE_WORDS
  unsigned long long* timing;       // [gridDim.x][4][2] counts, then the icache body's span; or null
};

struct Seg {
  uint32_t* words;
  uint32_t key;
  uint64_t seed;
  gm_cachescan_poke_t poke;
};

struct Passes {
  unsigned long long first, last;
  __device__ __forceinline__ void add(uint32_t pass, unsigned long long c0, unsigned long long c1) {
    if (pass == 0) first = c1 - c0;
    last = c1 - c0;
  }
};

__device__ __forceinline__ uint32_t bypass32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u32x4 bypass128(const u32x4* p) { return __builtin_nontemporal_load(p); }

// Nothing moves across it, and afterwards the compiler knows nothing about the value: two reads
// through the same address stay two loads, and a clock is read where it is written.
template <class V>
__device__ __forceinline__ void opaque(V& v) {
  asm volatile("" : "+v"(v));
}
__device__ __forceinline__ void opaque_uniform(uint32_t& v) { asm volatile("" : "+s"(v)); }

__device__ __forceinline__ u32x4 pattern4(uint64_t seed, uint32_t r, uint32_t v) {
  const u32x4 p = {gm_cachescan_pattern(seed, r, 4 * v), gm_cachescan_pattern(seed, r, 4 * v + 1),
                   gm_cachescan_pattern(seed, r, 4 * v + 2), gm_cachescan_pattern(seed, r, 4 * v + 3)};
  return p;
}

// The fill with round r's pattern, the barrier, and the poke of `test` if it is asked for.
__device__ __forceinline__ void fill(const Seg& g, uint32_t test, uint32_t r, bool poke_now) {
  u32x4* seg4 = (u32x4*)g.words;
  for (uint32_t k = 0; k < GM_CACHESCAN_SEG_VECS / GM_CUSCAN_THREADS; ++k) {
    const uint32_t v = gm_cachescan_fill_vec(threadIdx.x, k);  // < 4096
    seg4[v] = pattern4(g.seed, r, v) ^ g.key;
  }
  __syncthreads();
  if (poke_now && g.poke.mask != 0 && g.poke.test == test) {  // uniform
    if (threadIdx.x == 0) g.words[g.poke.word_offset] ^= g.poke.mask;
    __syncthreads();
  }
}

// ================================================================================ l2
__device__ __forceinline__ void test_l2(const Seg& g, uint32_t iters, uint32_t sig[4], Passes& pt) {
  const uint32_t t = threadIdx.x;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < iters; ++r) {
    const unsigned long long c0 = clock64();
    fill(g, GM_CACHESCAN_L2, r, r == 0);
    for (uint32_t i = 0; i < GM_CACHESCAN_SEG_WORDS / GM_CUSCAN_THREADS; ++i) {
      const uint32_t a = gm_cachescan_l2_perm(i * 256 + t);  // < 16384, each word once
      const uint32_t v = bypass32(g.words + a) ^ g.key;
      gm_cuscan_lds_fold32(sig, v, gm_cachescan_pattern(g.seed, r, a));
      g.words[a] = ~v ^ g.key;
    }
    __syncthreads();
    for (uint32_t k = 0; k < GM_CACHESCAN_SEG_VECS / GM_CUSCAN_THREADS; ++k) {
      const uint32_t v = gm_cachescan_l2_vec(t, k);  // < 4096
      const u32x4 got = bypass128((const u32x4*)g.words + v) ^ g.key;
      const u32x4 want = ~pattern4(g.seed, r, v);
      gm_cuscan_lds_fold128(sig, got.x, want.x);
      gm_cuscan_lds_fold128(sig, got.y, want.y);
      gm_cuscan_lds_fold128(sig, got.z, want.z);
      gm_cuscan_lds_fold128(sig, got.w, want.w);
    }
    __syncthreads();
    pt.add(r, c0, clock64());
  }
}

// ================================================================================ l1
// Word a through the L1 and again past it.
__device__ __forceinline__ void l1_probe(const Seg& g, uint32_t a, uint32_t sig[4]) {
  uint32_t at = a;
  opaque(at);  // the index, not the pointer: the loads stay global_load
  const uint32_t* p = g.words + at;
  const uint32_t l1 = *p ^ g.key;
  const uint32_t l2 = bypass32(p) ^ g.key;
  gm_cachescan_l1_fold(sig, l1, l2, gm_cachescan_pattern(g.seed, GM_CACHESCAN_L1_ROUND, a));
}

__device__ __forceinline__ void test_l1(const Seg& g, uint32_t iters, uint32_t sig[4], Passes& pt) {
  const uint32_t t = threadIdx.x;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  fill(g, GM_CACHESCAN_L1, GM_CACHESCAN_L1_ROUND, true);
  // A hit pass reads its 16 words through the L1 first, and only that half is timed: the bypass
  // loads that follow would hide whether the plain ones hit.
  constexpr uint32_t kHit = GM_CACHESCAN_L1_HIT_WORDS / GM_CUSCAN_THREADS;
  for (uint32_t pass = 0; pass < iters; ++pass) {
    uint32_t l1[kHit], sum = 0;
    opaque(sig[0]);
    const unsigned long long c0 = clock64();
#pragma unroll
    for (uint32_t i = 0; i < kHit; ++i) {
      uint32_t at = gm_cachescan_l1_hit_addr(t, i);  // < 4096
      opaque(at);
      l1[i] = g.words[at] ^ g.key;
      sum += l1[i];
    }
    opaque(sum);  // every value has arrived
    pt.add(pass, c0, clock64());
#pragma unroll
    for (uint32_t i = 0; i < kHit; ++i) {
      const uint32_t a = gm_cachescan_l1_hit_addr(t, i);
      gm_cachescan_l1_fold(sig, l1[i], bypass32(g.words + a) ^ g.key,
                           gm_cachescan_pattern(g.seed, GM_CACHESCAN_L1_ROUND, a));
    }
  }
  for (uint32_t i = 0; i < GM_CACHESCAN_SEG_WORDS / GM_CUSCAN_THREADS; ++i) {
    const uint32_t a = gm_cachescan_l1_sweep_addr(t, i);  // < 16384
    l1_probe(g, a, sig);
    l1_probe(g, a, sig);
  }
  __syncthreads();  // the next test's fill writes what other waves read here
}

// ================================================================================ scalar
// One dependent chain per wave on uniform values: the table reads at uniform indices through a
// const __restrict__ kernel argument are scalar loads, and each index comes from the word before.
__device__ __forceinline__ void test_scalar(uint64_t seed, uint32_t iters,
                                            const uint32_t* __restrict__ table, uint32_t sig[4],
                                            Passes& pt) {
  const uint32_t t = threadIdx.x, l = t & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(t >> 6);
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) sig[i] = gm_cuscan_hash(seed, GM_CACHESCAN_H_SCALAR_LANE, 4 * t + i);
  gm_cachescan_chain c = gm_cachescan_scalar_init(seed, w);
  for (uint32_t it = 0; it < iters; ++it) {
    opaque_uniform(c.i);
    const unsigned long long c0 = clock64();
#pragma unroll 4
    for (uint32_t k = 0; k < GM_CACHESCAN_SCALAR_STEPS; ++k) {
      const uint32_t s = it * GM_CACHESCAN_SCALAR_STEPS + k;
      gm_cachescan_scalar_step(c, s, table[c.i]);  // c.i < GM_CACHESCAN_TABLE_WORDS
      gm_cachescan_scalar_fold(sig, s, l, c);
    }
    opaque_uniform(c.i);
    pt.add(it, c0, clock64());
  }
}

// ================================================================================ icache
// Steps base .. base + count - 1, expanded by halving: the depth is log2 of the count.
template <uint32_t kBase, uint32_t kCount>
__device__ __forceinline__ void ic_steps(uint32_t& x, uint32_t& y) {
  if constexpr (kCount == 1) {
    gm_cachescan_ic_step(kBase, x, y);
  } else {
    ic_steps<kBase, kCount / 2>(x, y);
    ic_steps<kBase + kCount / 2, kCount - kCount / 2>(x, y);
  }
}

// The body, once: a function of its own, so that its code is laid out once and its symbol's size
// is the body's span. The program counter is read at both ends, tied to the chains so that every
// step lies between the two readings. Returns {x, y, span in bytes}; everything is in registers.
__device__ __noinline__ u32x4 ic_body(uint32_t x, uint32_t y) {
  uint64_t pc0, pc1;
  asm volatile("s_getpc_b64 %0" : "=s"(pc0), "+v"(x), "+v"(y));
  ic_steps<0, GM_CACHESCAN_ICACHE_STEPS>(x, y);
  asm volatile("s_getpc_b64 %0" : "=s"(pc1), "+v"(x), "+v"(y));
  const u32x4 r = {x, y, (uint32_t)(pc1 - pc0), 0};
  return r;
}

__device__ __forceinline__ void test_icache(uint64_t seed, uint32_t iters, uint32_t sig[4],
                                            Passes& pt, uint32_t& span) {
  const uint32_t t = threadIdx.x;
  uint32_t x = gm_cuscan_hash(seed, GM_CACHESCAN_H_ICACHE, 2 * t);
  uint32_t y = gm_cuscan_hash(seed, GM_CACHESCAN_H_ICACHE, 2 * t + 1);
  uint32_t sx = 0, sy = 0;
  for (uint32_t it = 0; it < iters; ++it) {
    opaque(x);
    const unsigned long long c0 = clock64();
    const u32x4 r = ic_body(x, y);
    x = r.x;
    y = r.y;
    span = r.z;
    opaque(x);
    pt.add(it, c0, clock64());
    sx = gm_cachescan_fold(sx, x);
    sy = gm_cachescan_fold(sy, y);
  }
  sig[0] = x;
  sig[1] = y;
  sig[2] = sx;
  sig[3] = sy;
}

// kCompare / !kCompare as k_cuscan: the scan, or one block's raw signature of the one test in
// p.tests. The LDS is declared to keep the CU to one block and carries the block's outcome.
template <bool kCompare>
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_cachescan(
    Params p, gm_cachescan_poke_t poke, Bufs bufs, const uint32_t* __restrict__ expected,
    const uint32_t* __restrict__ table, DevTable* tab, uint32_t* sig_out, uint32_t* where_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[GM_CUSCAN_LDS_WORDS];
  const Where at = where_am_i();
  const uint32_t b = blockIdx.x;
  const Seg g = {bufs.arena + (size_t)b * GM_CACHESCAN_SEG_WORDS, gm_cachescan_key(p.seed, b), p.seed,
                 poke};
  unsigned long long* timing = bufs.timing ? bufs.timing + (size_t)b * 2 * GM_CACHESCAN_TESTS : nullptr;
  uint32_t failed = 0, bad = 0;
  uint32_t sig[4];
#define GM_CACHESCAN_DONE(TEST, IX)                                                        \
  if (timing && threadIdx.x == 0) {                                                        \
    timing[2 * IX] = pt.first;                                                             \
    timing[2 * IX + 1] = pt.last;                                                          \
  }                                                                                        \
  finish<kCompare>(p, TEST, IX, at, sig, expected, tab, sig_out, failed, bad)
  if (p.tests & GM_CACHESCAN_L2) {
    Passes pt = {0, 0};
    test_l2(g, p.iters, sig, pt);
    GM_CACHESCAN_DONE(GM_CACHESCAN_L2, GM_CACHESCAN_IX_L2);
  }
  if (p.tests & GM_CACHESCAN_L1) {
    Passes pt = {0, 0};
    test_l1(g, p.iters, sig, pt);
    GM_CACHESCAN_DONE(GM_CACHESCAN_L1, GM_CACHESCAN_IX_L1);
  }
  if (p.tests & GM_CACHESCAN_SCALAR) {
    Passes pt = {0, 0};
    test_scalar(p.seed, p.iters, table, sig, pt);
    GM_CACHESCAN_DONE(GM_CACHESCAN_SCALAR, GM_CACHESCAN_IX_SCALAR);
  }
  if (p.tests & GM_CACHESCAN_ICACHE) {
    Passes pt = {0, 0};
    uint32_t span = 0;
    test_icache(p.seed, p.iters, sig, pt, span);
    // every block stores the same span behind the last block's counts
    if (bufs.timing && threadIdx.x == 0)
      bufs.timing[(size_t)gridDim.x * 2 * GM_CACHESCAN_TESTS] = span;
    GM_CACHESCAN_DONE(GM_CACHESCAN_ICACHE, GM_CACHESCAN_IX_ICACHE);
  }
#undef GM_CACHESCAN_DONE
  book_block<kCompare>(lds, at, failed, bad, tab, where_out);
}

bool iters_ok(uint32_t, uint32_t iters) { return iters >= 1 && iters <= GM_CACHESCAN_MAX_ITERS; }

constexpr ScanArgs kArgs = {GM_CACHESCAN_ALL, iters_ok};

// a poke of one selected test that has data, inside that data
bool poke_ok(const gm_cachescan_poke_t* pk, uint32_t tests) {
  if (!one_bit_ok(kArgs, pk->test) || !(pk->test & tests) || pk->mask == 0) return false;
  if (pk->test == GM_CACHESCAN_ICACHE) return false;
  return pk->word_offset <
         (pk->test == GM_CACHESCAN_SCALAR ? GM_CACHESCAN_TABLE_WORDS : GM_CACHESCAN_SEG_WORDS);
}

// the table of `test` in a run with `pk` (null: none): a poke of another test leaves it alone
void expected_of(uint32_t test, uint64_t seed, uint32_t iters, const gm_cachescan_poke_t* pk,
                 uint32_t* out) {
  const bool mine = pk && pk->test == test;
  gm_cachescan_expected_host(test, seed, iters, mine ? pk->word_offset : 0, mine ? pk->mask : 0, out);
}

// the scalar test's table as uploaded: the host makes that test's poke
void fill_table(uint64_t seed, const gm_cachescan_poke_t* pk, uint32_t* table) {
  for (uint32_t i = 0; i < GM_CACHESCAN_TABLE_WORDS; ++i) table[i] = gm_cachescan_table(seed, i);
  if (pk && pk->test == GM_CACHESCAN_SCALAR) table[pk->word_offset] ^= pk->mask;
}

// What one launch needs besides the frame's buffers: the arena of `blocks` segments, the table and
// the timing buffer (zeroed).
struct Run {
  DevBuf arena, table, timing;
  int blocks = 0;
  int alloc(int n, uint64_t seed, const gm_cachescan_poke_t* pk, hipStream_t stream) {
    blocks = n;
    std::vector<uint32_t> h(GM_CACHESCAN_TABLE_WORDS);
    fill_table(seed, pk, h.data());
    GM_CHECK(arena.alloc((size_t)n * GM_CACHESCAN_SEG_BYTES));
    GM_CHECK(table.alloc(GM_CACHESCAN_TABLE_BYTES));
    GM_CHECK(timing.alloc(timing_bytes()));
    GM_CHECK(hipMemcpyAsync(table.p, h.data(), GM_CACHESCAN_TABLE_BYTES, hipMemcpyHostToDevice, stream));
    GM_CHECK(hipMemsetAsync(timing.p, 0, timing_bytes(), stream));
    GM_CHECK(hipStreamSynchronize(stream));  // h goes out of scope
    return 0;
  }
  size_t timing_words() const { return (size_t)blocks * 2 * GM_CACHESCAN_TESTS + 1; }
  size_t timing_bytes() const { return timing_words() * sizeof(unsigned long long); }
  Bufs bufs() const { return {(uint32_t*)arena.p, (const uint32_t*)table.p, (unsigned long long*)timing.p}; }
};

void min_median_max(std::vector<unsigned long long>& v, uint64_t out[3]) {
  std::sort(v.begin(), v.end());
  out[0] = v.front();
  out[1] = v[v.size() / 2];
  out[2] = v.back();
}

}  // namespace

extern "C" {

int gm_probe_cachescan_expected(uint32_t test, uint64_t seed, uint32_t iters,
                                const gm_cachescan_poke_t* poke, uint32_t* out) {
  if (!one_test_ok(kArgs, test, iters) || !out) return (int)hipErrorInvalidValue;
  // a poke of another test is a legal run in which this test's table is the clean one
  if (poke && !poke_ok(poke, GM_CACHESCAN_ALL)) return (int)hipErrorInvalidValue;
  expected_of(test, seed, iters, poke, out);
  return 0;
}

int gm_probe_cachescan_geometry(uint32_t* seg_bytes, uint32_t* l1_hit_bytes, uint32_t* table_bytes,
                                uint32_t* icache_steps) {
  if (!seg_bytes || !l1_hit_bytes || !table_bytes || !icache_steps) return (int)hipErrorInvalidValue;
  *seg_bytes = GM_CACHESCAN_SEG_BYTES;
  *l1_hit_bytes = GM_CACHESCAN_L1_HIT_BYTES;
  *table_bytes = GM_CACHESCAN_TABLE_BYTES;
  *icache_steps = GM_CACHESCAN_ICACHE_STEPS;
  return 0;
}

int gm_probe_cachescan_signature(uint32_t test, uint64_t seed, uint32_t iters,
                                 const gm_cachescan_poke_t* poke, uint32_t* dev_out,
                                 uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, test, iters) || !signature_out_ok(dev_out, dev_where) ||
      (poke && !poke_ok(poke, test)))
    return (int)hipErrorInvalidValue;
  const Params p = params_of(seed, test, iters);
  Run run;
  if (int e = run.alloc(1, seed, poke, (hipStream_t)stream)) return e;
  hipLaunchKernelGGL(k_cachescan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream, p,
                     poke ? *poke : gm_cachescan_poke_t{}, run.bufs(), (const uint32_t*)nullptr,
                     (const uint32_t*)run.table.p, (DevTable*)nullptr, dev_out, dev_where);
  GM_CHECK(hipGetLastError());
  // the buffers are freed once the block that uses them is done
  GM_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int gm_probe_cachescan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                       int max_rounds, const gm_cuscan_inject_t* inject,
                       const gm_cachescan_poke_t* poke, gm_cuscan_result_t* out, gm_cuscan_cu_t* cus,
                       int cus_cap, int* n_cus, gm_cachescan_timing_t* timing) {
  if (out && timing) memset(timing, 0, sizeof(*timing));
  if (!scan_args_ok(kArgs, tests_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus) ||
      (poke && !poke_ok(poke, tests_mask)))
    return (int)hipErrorInvalidValue;
  const Params p = params_of(seed, tests_mask, iters, inject);
  const gm_cachescan_poke_t pk = poke ? *poke : gm_cachescan_poke_t{};
  DeviceGuard g(dev);  // the buffers below are this device's, from the first launch to the read
  if (!g.ok) return (int)hipErrorInvalidDevice;
  Run run;
  const int e = run_scan_with(
      dev, (const void*)k_cachescan<true>, (size_t)GM_CACHESCAN_TESTS * GM_CUSCAN_SIG_WORDS,
      [&](uint32_t* exp) {
        // the clean table also under a poke: the poked word is what the compare is to find
        for (int t = 0; t < GM_CACHESCAN_TESTS; ++t)
          if (tests_mask & (1u << t))
            expected_of(1u << t, seed, iters, nullptr, exp + (size_t)t * GM_CUSCAN_SIG_WORDS);
      },
      [&](int blocks, const uint32_t* expected, DevTable* tab) {
        if (run.blocks == 0)
          if (int e = run.alloc(blocks, seed, poke, nullptr)) return e;
        hipLaunchKernelGGL(k_cachescan<true>, dim3((unsigned)blocks), dim3(GM_CUSCAN_THREADS), 0,
                           nullptr, p, pk, run.bufs(), expected, (const uint32_t*)run.table.p, tab,
                           (uint32_t*)nullptr, (uint32_t*)nullptr);
        return (int)hipGetLastError();
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
  if (e) return e;
  if (timing) {
    // the last round's counts; the frame's read of the result table waited for that round
    std::vector<unsigned long long> h(run.timing_words());
    GM_CHECK(hipMemcpy(h.data(), run.timing.p, run.timing_bytes(), hipMemcpyDeviceToHost));
    timing->blocks = (uint32_t)run.blocks;
    std::vector<unsigned long long> col((size_t)run.blocks);
    for (int t = 0; t < GM_CACHESCAN_TESTS; ++t) {
      if (!(tests_mask & (1u << t))) continue;
      for (int which = 0; which < 2; ++which) {
        for (int b = 0; b < run.blocks; ++b) col[b] = h[((size_t)b * GM_CACHESCAN_TESTS + t) * 2 + which];
        min_median_max(col, which ? timing->last[t] : timing->first[t]);
      }
    }
  }
  return 0;
}

int gm_probe_cachescan_kernel_info(int* num_regs, int* scratch_bytes, int* icache_body_bytes) {
  if (!num_regs || !scratch_bytes || !icache_body_bytes) return (int)hipErrorInvalidValue;
  hipFuncAttributes attr;
  GM_CHECK(hipFuncGetAttributes(&attr, (const void*)k_cachescan<true>));
  *num_regs = attr.numRegs;
  *scratch_bytes = (int)attr.localSizeBytes;
  // the body's span from the program counter at its two ends: one block runs it once
  Params p{};
  p.tests = GM_CACHESCAN_ICACHE;
  p.iters = 1;
  Run run;
  DevBuf sig;
  if (int e = run.alloc(1, 0, nullptr, nullptr)) return e;
  GM_CHECK(sig.alloc((GM_CUSCAN_SIG_WORDS + 8) * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_cachescan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, nullptr, p,
                     gm_cachescan_poke_t{}, run.bufs(), (const uint32_t*)nullptr,
                     (const uint32_t*)run.table.p, (DevTable*)nullptr, (uint32_t*)sig.p,
                     (uint32_t*)sig.p + GM_CUSCAN_SIG_WORDS);
  GM_CHECK(hipGetLastError());
  unsigned long long span = 0;
  GM_CHECK(hipMemcpy(&span, (unsigned long long*)run.timing.p + 2 * GM_CACHESCAN_TESTS, sizeof(span),
                     hipMemcpyDeviceToHost));
  *icache_body_bytes = (int)span;
  return 0;
}

}  // extern "C"
