// gm_cuscan.hip — per-compute-unit self-test for gfx950: which CU computes a wrong word?
//
// One kernel, k_cuscan, runs the selected known-answer tests (integer VALU, fp32 FMA, bf16 MFMA,
// an LDS march; formulas in gm_probe.h, code in gm_cuscan_sig.h) in a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU. Each thread
// compares its 4 signature words per test with a table the host computed, and thread 0 of the
// block books the outcome under the CU id read from the hardware registers. Where a block runs is
// observed, never assumed: the blocks share nothing but atomics into the result table and there
// is no wait between them.
//
// The frame (where a block runs, the compare, the bookkeeping, the round loop) is
// gm_cuscan_frame.h, shared with the matrix-core format scan.
#include "gm_cuscan_frame.h"

namespace {

__device__ __forceinline__ void test_mfma(uint64_t seed, uint32_t iters, uint32_t sig[4]) {
  const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63;
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t steps = iters * GM_CUSCAN_MFMA_STEPS;
  for (uint32_t s = 0; s < steps; ++s) {
    const uint32_t ha = gm_cuscan_mfma_hash(seed, s, w, 0, l);
    const uint32_t hb = gm_cuscan_mfma_hash(seed, s, w, 1, l);
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = (__bf16)(float)gm_cuscan_mfma_entry(ha, j);  // small integers: exact in bf16
      b[j] = (__bf16)(float)gm_cuscan_mfma_entry(hb, j);
    }
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = gm_cuscan_f32_bits(c[i]);
}

__device__ __forceinline__ void test_lds(uint32_t* lds, uint64_t seed, uint32_t iters,
                                         uint32_t sig[4]) {
  const uint32_t t = threadIdx.x;
  u32x4* lds4 = (u32x4*)lds;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < iters; ++r) {
    for (uint32_t k = 0; k < GM_CUSCAN_LDS_WORDS / 1024; ++k) {
      const uint32_t v = k * 256 + t;  // < 10240
      const u32x4 p = {gm_cuscan_lds_pattern(seed, r, 4 * v),
                       gm_cuscan_lds_pattern(seed, r, 4 * v + 1),
                       gm_cuscan_lds_pattern(seed, r, 4 * v + 2),
                       gm_cuscan_lds_pattern(seed, r, 4 * v + 3)};
      lds4[v] = p;
    }
    __syncthreads();
    for (uint32_t i = 0; i < GM_CUSCAN_LDS_WORDS / 256; ++i) {
      const uint32_t a = gm_cuscan_lds_perm(i * 256 + t);  // < 40960, each address once
      const uint32_t g = lds[a];
      gm_cuscan_lds_fold32(sig, g, gm_cuscan_lds_pattern(seed, r, a));
      lds[a] = ~g;
    }
    __syncthreads();
    for (uint32_t k = 0; k < GM_CUSCAN_LDS_WORDS / 1024; ++k) {
      const uint32_t v = gm_cuscan_lds_vec(t, k);  // < 10240
      const u32x4 g = lds4[v];
      gm_cuscan_lds_fold128(sig, g.x, ~gm_cuscan_lds_pattern(seed, r, 4 * v));
      gm_cuscan_lds_fold128(sig, g.y, ~gm_cuscan_lds_pattern(seed, r, 4 * v + 1));
      gm_cuscan_lds_fold128(sig, g.z, ~gm_cuscan_lds_pattern(seed, r, 4 * v + 2));
      gm_cuscan_lds_fold128(sig, g.w, ~gm_cuscan_lds_pattern(seed, r, 4 * v + 3));
    }
    __syncthreads();
  }
}

// kCompare: the scan (any grid). !kCompare: one block that stores the raw signature of the one
// test in p.tests to sig_out[1024] and {CU id, the 4 waves' SIMDs} to where_out[5].
template <bool kCompare>
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_cuscan(Params p,
                                                              const uint32_t* __restrict__ expected,
                                                              DevTable* tab, uint32_t* sig_out,
                                                              uint32_t* where_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[GM_CUSCAN_LDS_WORDS];
  const uint32_t t = threadIdx.x;
  const Where at = where_am_i();
  uint32_t failed = 0, bad = 0;
  uint32_t sig[4];
  if (p.tests & GM_CUSCAN_VALU_INT) {
    gm_cuscan_int(p.seed, p.iters, t, sig);
    finish<kCompare>(p, GM_CUSCAN_VALU_INT, 0, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_CUSCAN_VALU_F32) {
    gm_cuscan_f32(p.seed, p.iters, t, sig);
    finish<kCompare>(p, GM_CUSCAN_VALU_F32, 1, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_CUSCAN_MFMA) {
    test_mfma(p.seed, p.iters, sig);
    finish<kCompare>(p, GM_CUSCAN_MFMA, 2, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_CUSCAN_LDS) {
    test_lds(lds, p.seed, p.iters, sig);
    finish<kCompare>(p, GM_CUSCAN_LDS, 3, at, sig, expected, tab, sig_out, failed, bad);
  }

  book_block<kCompare>(lds, at, failed, bad, tab, where_out);
}

bool iters_ok(uint32_t tests, uint32_t iters) {
  if (iters == 0 || iters > GM_CUSCAN_MAX_ITERS) return false;
  return !(tests & GM_CUSCAN_MFMA) || iters <= GM_CUSCAN_MFMA_MAX_ITERS;
}

constexpr ScanArgs kArgs = {GM_CUSCAN_ALL, iters_ok};

}  // namespace

extern "C" {

int gm_probe_cuscan_expected(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* out) {
  if (!one_test_ok(kArgs, test, iters) || !out) return (int)hipErrorInvalidValue;
  gm_cuscan_expected_host(test, seed, iters, out);
  return 0;
}

int gm_probe_cuscan_signature(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                              uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, test, iters) || !signature_out_ok(dev_out, dev_where))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cuscan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream,
                     params_of(seed, test, iters), (const uint32_t*)nullptr, (DevTable*)nullptr,
                     dev_out, dev_where);
  return (int)hipGetLastError();
}

int gm_probe_cuscan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                    int max_rounds, const gm_cuscan_inject_t* inject, gm_cuscan_result_t* out,
                    gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!scan_args_ok(kArgs, tests_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus))
    return (int)hipErrorInvalidValue;
  return run_scan(
      dev, k_cuscan<true>, params_of(seed, tests_mask, iters, inject), 4 * GM_CUSCAN_SIG_WORDS,
      [&](uint32_t* exp) {
        for (int i = 0; i < 4; ++i)
          if (tests_mask & (1u << i))
            gm_cuscan_expected_host(1u << i, seed, iters, exp + (size_t)i * GM_CUSCAN_SIG_WORDS);
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

}  // extern "C"
