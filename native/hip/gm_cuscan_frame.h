// gm_cuscan_frame.h — the frame the per-CU scans share (gm_cuscan.hip, gm_mfmascan.hip,
// gm_lanescan.hip, gm_cachescan.hip, gm_ldsscan.hip): where a
// block runs, the result table, the compare of one test's signature with the host's table, the
// block-outcome reduction, the round loop and the decode into gm_cuscan_cu_t.
//
// A scan kernel is a 256-thread block that statically declares all 160 KiB of LDS, so at most one
// block is resident per CU. Each thread compares its 4 signature words per test with a table the
// host computed, and thread 0 of the block books the outcome under the CU id read from the
// hardware registers. Where a block runs is observed, never assumed: the blocks share nothing but
// atomics into the result table and there is no wait between them.
//
// The error path is cold, as in gm_memtest.hip: one OR per test on a healthy unit.
// Everything is in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "gm_probe.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "gm_cuscan_sig.h"
#include "gm_probe_common.h"
#include "gm_where.h"  // Where, where_am_i(): shared with the attributed burn-in

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Slot {
  uint32_t runs, failed_runs, tests_failed, simds_seen, simds_failed;
};

struct DevTable {
  unsigned long long words, blocks, four_simds;
  uint32_t distinct, claims;
  gm_cuscan_record_t rec[GM_CUSCAN_MAX_RECORDS];
  Slot slot[GM_CUSCAN_IDS];
};

struct Params {
  uint64_t seed;
  uint32_t tests, iters;
  gm_cuscan_inject_t inj;  // mask 0: none
};

// kCompare: the scan (any grid). !kCompare: one block that stores the raw signature of the one
// test in p.tests to sig_out[1024] and {CU id, the 4 waves' SIMDs} to where_out[5].
typedef void (*ScanKernel)(Params, const uint32_t*, DevTable*, uint32_t*, uint32_t*);

// Cold: entered per wrong word only.
__device__ __noinline__ void report(DevTable* tab, uint32_t id, uint32_t simd, uint32_t test,
                                    uint32_t thread, uint32_t word, uint32_t e, uint32_t g) {
  const unsigned int slot = atomicAdd(&tab->claims, 1u);
  if (slot < GM_CUSCAN_MAX_RECORDS) {
    gm_cuscan_record_t* r = &tab->rec[slot];
    r->id = id;
    r->simd = simd;
    r->test = test;
    r->thread = thread;
    r->word = word;
    r->expected = e;
    r->got = g;
    r->pad = 0;
  }
}

// What became of one test's signature: the injected flip, then the compare (or the raw store).
template <bool kCompare>
__device__ __forceinline__ void finish(const Params& p, uint32_t test, int test_index,
                                       const Where& at, uint32_t sig[4],
                                       const uint32_t* __restrict__ expected, DevTable* tab,
                                       uint32_t* sig_out, uint32_t& failed, uint32_t& bad) {
  const uint32_t t = threadIdx.x;
  if (p.inj.mask != 0 && p.inj.test == test && p.inj.thread == t &&
      (p.inj.id == GM_CUSCAN_ANY || p.inj.id == at.id)) {
#pragma unroll  // constant indices keep sig[] in registers
    for (uint32_t i = 0; i < 4; ++i)
      if (i == p.inj.word) sig[i] ^= p.inj.mask;
  }
  if constexpr (kCompare) {
    const u32x4 e = ((const u32x4*)expected)[test_index * GM_CUSCAN_THREADS + t];
    if (((sig[0] ^ e.x) | (sig[1] ^ e.y) | (sig[2] ^ e.z) | (sig[3] ^ e.w)) != 0) {
      const uint32_t ev[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i)
        if (sig[i] != ev[i]) {
          report(tab, at.id, at.simd, test, t, i, ev[i], sig[i]);
          ++bad;
        }
      failed |= test;
    }
  } else {
    const u32x4 v = {sig[0], sig[1], sig[2], sig[3]};
    ((u32x4*)sig_out)[t] = v;
  }
}

// The block's outcome: one leader lane per wave hands its wave's to thread 0 through the LDS,
// which the tests are done with; thread 0 books it (or, !kCompare, stores where the block ran).
template <bool kCompare>
__device__ __forceinline__ void book_block(uint32_t* lds, const Where& at, uint32_t failed,
                                           uint32_t bad, DevTable* tab, uint32_t* where_out) {
  const uint32_t t = threadIdx.x, w = t >> 6;
  __syncthreads();
  uint32_t wave_failed = failed, wave_bad = bad;
  for (int off = 32; off > 0; off >>= 1) {
    wave_failed |= __shfl_down(wave_failed, off, kWave);
    wave_bad += __shfl_down(wave_bad, off, kWave);
  }
  if ((t & 63) == 0) {
    lds[w] = at.simd;
    lds[4 + w] = wave_failed;
    lds[8 + w] = wave_bad;
  }
  __syncthreads();
  if (t != 0) return;
  uint32_t seen = 0, simds_failed = 0, tests_failed = 0, words = 0;
  for (uint32_t i = 0; i < 4; ++i) {
    seen |= 1u << (lds[i] & 3);
    if (lds[4 + i]) simds_failed |= 1u << (lds[i] & 3);
    tests_failed |= lds[4 + i];
    words += lds[8 + i];
  }
  if constexpr (kCompare) {
    Slot* s = &tab->slot[at.id & (GM_CUSCAN_IDS - 1)];
    if (atomicAdd(&s->runs, 1u) == 0) atomicAdd(&tab->distinct, 1u);
    atomicOr(&s->simds_seen, seen);
    atomicAdd(&tab->blocks, 1ull);
    if (__popc(seen) == 4) atomicAdd(&tab->four_simds, 1ull);
    if (tests_failed) {
      atomicAdd(&s->failed_runs, 1u);
      atomicOr(&s->tests_failed, tests_failed);
      atomicOr(&s->simds_failed, simds_failed);
      atomicAdd(&tab->words, (unsigned long long)words);
    }
  } else {
    where_out[0] = at.id;
    for (uint32_t i = 0; i < 4; ++i) where_out[1 + i] = lds[i];
  }
}

// What a scan's entry points check their arguments against: the mask of all its tests (one test
// is one bit of it) and what it accepts as iters for a mask of tests.
struct ScanArgs {
  uint32_t all;
  bool (*iters_ok)(uint32_t tests, uint32_t iters);
};

inline bool one_bit_ok(const ScanArgs& s, uint32_t t) {
  return t != 0 && (t & (t - 1)) == 0 && (t & ~s.all) == 0;
}

// _expected and _signature: one test, its iters.
inline bool one_test_ok(const ScanArgs& s, uint32_t test, uint32_t iters) {
  return one_bit_ok(s, test) && s.iters_ok(test, iters);
}

// _signature: a 16-byte aligned table of signatures, a 4-byte aligned {CU id, 4 SIMDs}.
inline bool signature_out_ok(const uint32_t* dev_out, const uint32_t* dev_where) {
  return dev_out && !((uintptr_t)dev_out & 15) && dev_where && !((uintptr_t)dev_where & 3);
}

inline Params params_of(uint64_t seed, uint32_t tests, uint32_t iters,
                        const gm_cuscan_inject_t* inject = nullptr) {
  Params p{};
  p.seed = seed;
  p.tests = tests;
  p.iters = iters;
  if (inject) p.inj = *inject;
  return p;
}

// The scan entry point's prologue: the outputs zeroed (false without `out`), then every argument
// the scans share checked. A false return is hipErrorInvalidValue, before any HIP call.
inline bool scan_args_ok(const ScanArgs& s, uint32_t tests, uint32_t iters, int min_rounds,
                         int max_rounds, const gm_cuscan_inject_t* in, gm_cuscan_result_t* out,
                         const gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!out) return false;
  memset(out, 0, sizeof(*out));
  if (n_cus) *n_cus = 0;
  if (tests == 0 || (tests & ~s.all) || !s.iters_ok(tests, iters)) return false;
  if (min_rounds < 1 || max_rounds < min_rounds || max_rounds > 1024 || cus_cap < 0 ||
      (cus_cap != 0 && !cus))
    return false;
  return !in || (one_bit_ok(s, in->test) && (in->test & tests) && in->thread < GM_CUSCAN_THREADS &&
                 in->word < 4 && in->mask != 0 &&
                 (in->id == GM_CUSCAN_ANY || in->id < GM_CUSCAN_IDS));
}

// The scan of device `dev` with the compare form of a scan kernel; the arguments were checked.
// `fill` writes the expected table (exp_words words, zeroed) on the host: a unit that computes
// wrongly must not produce its own.
// `launch(blocks, expected, tab)` enqueues one round of `blocks` blocks of the compare form of
// `kernel` on the null stream and returns a HIP error code: a scan whose kernel takes more than
// ScanKernel's arguments brings its own.
template <class Fill, class Launch>
int run_scan_with(int dev, const void* kernel, size_t exp_words, Fill fill, Launch launch,
                  int min_rounds, int max_rounds, gm_cuscan_result_t* out, gm_cuscan_cu_t* cus,
                  int cus_cap, int* n_cus) {
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  const double t0 = now_s();
  int cu_count = 0;
  if (int e = current_cus(&cu_count)) return e;
  if (cu_count <= 0) return (int)hipErrorInvalidDevice;

  std::vector<uint32_t> h_exp(exp_words, 0);
  fill(h_exp.data());
  DevBuf dexp, dtab;
  GM_CHECK(dexp.alloc(h_exp.size() * sizeof(uint32_t)));
  GM_CHECK(dtab.alloc(sizeof(DevTable)));
  GM_CHECK(hipMemcpy(dexp.p, h_exp.data(), h_exp.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  GM_CHECK(hipMemset(dtab.p, 0, sizeof(DevTable)));
  Events ev;
  GM_CHECK(ev.create());
  {
    // loads the code object here, not between a timed pair of events
    hipFuncAttributes attr;
    GM_CHECK(hipFuncGetAttributes(&attr, kernel));
  }
  DevTable* tab = (DevTable*)dtab.p;

  int rounds = 0;
  uint32_t distinct = 0;
  double ms_sum = 0;
  while (rounds < max_rounds) {
    GM_CHECK(hipEventRecord(ev.e0, nullptr));
    if (int e = launch(cu_count, (const uint32_t*)dexp.p, tab)) return e;
    GM_CHECK(hipEventRecord(ev.e1, nullptr));
    GM_CHECK(hipMemcpy(&distinct, &tab->distinct, sizeof(distinct), hipMemcpyDeviceToHost));
    float ms = 0;
    if (int e = elapsed_ms(ev.e0, ev.e1, &ms)) return e;
    ms_sum += ms;
    ++rounds;
    if (rounds >= min_rounds && distinct >= (uint32_t)cu_count) break;
  }

  std::vector<unsigned char> raw(sizeof(DevTable));
  GM_CHECK(hipMemcpy(raw.data(), dtab.p, sizeof(DevTable), hipMemcpyDeviceToHost));
  const DevTable* h = (const DevTable*)raw.data();
  out->cus_expected = (uint32_t)cu_count;
  out->rounds = (uint32_t)rounds;
  out->blocks_run = h->blocks;
  out->words_in_error = h->words;
  out->blocks_four_simds = h->four_simds;
  out->records_filled = h->claims < GM_CUSCAN_MAX_RECORDS ? h->claims : GM_CUSCAN_MAX_RECORDS;
  for (uint32_t i = 0; i < out->records_filled; ++i) out->records[i] = h->rec[i];
  int n = 0;
  for (uint32_t id = 0; id < GM_CUSCAN_IDS; ++id) {
    const Slot& s = h->slot[id];
    if (s.runs == 0) continue;
    ++out->cus_seen;
    ++out->xcc_cus[id >> 8];
    if (s.failed_runs) ++out->failed_cus;
    if (n < cus_cap) {
      gm_cuscan_cu_t* c = &cus[n];
      c->id = id;
      c->xcc = id >> 8;
      c->se = (id >> 5) & 7;
      c->sh = (id >> 4) & 1;
      c->cu = id & 15;
      c->runs = s.runs;
      c->failed_runs = s.failed_runs;
      c->tests_failed = s.tests_failed;
      c->simds_seen = s.simds_seen;
      c->simds_failed = s.simds_failed;
    }
    ++n;
  }
  if (n_cus) *n_cus = n;
  out->complete = out->cus_seen == out->cus_expected;
  out->kernel_ms = ms_sum;
  out->seconds = now_s() - t0;
  return 0;
}

// The scan with a kernel of ScanKernel's signature.
template <class Fill>
int run_scan(int dev, ScanKernel kernel, const Params& p, size_t exp_words, Fill fill,
             int min_rounds, int max_rounds, gm_cuscan_result_t* out, gm_cuscan_cu_t* cus,
             int cus_cap, int* n_cus) {
  return run_scan_with(
      dev, (const void*)kernel, exp_words, fill,
      [&](int blocks, const uint32_t* expected, DevTable* tab) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GM_CUSCAN_THREADS), 0, nullptr, p,
                           expected, tab, (uint32_t*)nullptr, (uint32_t*)nullptr);
        return (int)hipGetLastError();
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

}  // namespace
