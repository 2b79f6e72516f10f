// gm_sparsescan.hip — per-CU sparse (2:4) and 32x32 matrix-core scan for gfx950: which CU's
// sparse matrix path (v_smfmac_*: the index register, the 4:2 operand selector, the abid set
// selector) computes a wrong word, and in which form?
//
// One kernel, k_sparsescan, in the CU scan's frame (gm_cuscan_frame.h): a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU. Every wave
// runs `iters` dependent SMFMACs of each selected form (f16, bf16, i8, fp8, bf8 and the two mixed
// fp8/bf8 forms at 16x16; f16, bf16, i8 and fp8 at 32x32) on operand images and index words
// derived from the seed (gm_sparsescan_ref.h, formulas and premises in gm_probe.h). Every product
// and partial sum is exact in the accumulator type, so the accumulator registers of a lane are
// one definite bit pattern, which is compared with the table the host computed.
// k_sparse_apply runs one instruction per wave on images the caller built and stores the raw
// accumulator registers: the premises are checked, and a wrong one is read off, with it.
#include "gm_sparsescan_ref.h"

#include "gm_cuscan_frame.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));

// The accumulator of form F: 4 or 16 registers, int32 for i8.
template <int F>
struct Acc {
  static constexpr bool kBig = F >= GM_SPARSESCAN_IX_F16_32;
  static constexpr bool kInt = F == GM_SPARSESCAN_IX_I8 || F == GM_SPARSESCAN_IX_I8_32;
  static constexpr int kRegs = kBig ? 16 : 4;
  typedef __attribute__((ext_vector_type(kRegs))) int I;
  typedef __attribute__((ext_vector_type(kRegs))) float Fl;
  typedef typename std::conditional<kInt, I, Fl>::type type;
};

// One instruction of form F with set selector kAbid (an immediate, hence a template argument).
template <int F, int kAbid>
__device__ __forceinline__ typename Acc<F>::type mac(const uint32_t a[4], const uint32_t b[8],
                                                     uint32_t idx, typename Acc<F>::type c) {
  const u32x4 ua = {a[0], a[1], a[2], a[3]};
  const u32x8 ub = {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]};
  const i32x4 ia = __builtin_bit_cast(i32x4, ua);
  const i32x8 ib = __builtin_bit_cast(i32x8, ub);
  const int ix = (int)idx;
  if constexpr (F == GM_SPARSESCAN_IX_F16)
    return __builtin_amdgcn_smfmac_f32_16x16x64_f16(__builtin_bit_cast(f16x8, ua),
                                                    __builtin_bit_cast(f16x16, ub), c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_BF16)
    return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(__builtin_bit_cast(bf16x8, ua),
                                                     __builtin_bit_cast(bf16x16, ub), c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_I8)
    return __builtin_amdgcn_smfmac_i32_16x16x128_i8(ia, ib, c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_FP8)
    return __builtin_amdgcn_smfmac_f32_16x16x128_fp8_fp8(ia, ib, c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_BF8)
    return __builtin_amdgcn_smfmac_f32_16x16x128_bf8_bf8(ia, ib, c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_FP8BF8)
    return __builtin_amdgcn_smfmac_f32_16x16x128_fp8_bf8(ia, ib, c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_BF8FP8)
    return __builtin_amdgcn_smfmac_f32_16x16x128_bf8_fp8(ia, ib, c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_F16_32)
    return __builtin_amdgcn_smfmac_f32_32x32x32_f16(__builtin_bit_cast(f16x8, ua),
                                                    __builtin_bit_cast(f16x16, ub), c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_BF16_32)
    return __builtin_amdgcn_smfmac_f32_32x32x32_bf16(__builtin_bit_cast(bf16x8, ua),
                                                     __builtin_bit_cast(bf16x16, ub), c, ix, 0, kAbid);
  else if constexpr (F == GM_SPARSESCAN_IX_I8_32)
    return __builtin_amdgcn_smfmac_i32_32x32x64_i8(ia, ib, c, ix, 0, kAbid);
  else
    return __builtin_amdgcn_smfmac_f32_32x32x64_fp8_fp8(ia, ib, c, ix, 0, kAbid);
}

// The instruction with a set selector known only when it runs: two call sites for the 16-bit
// forms; the 8-bit forms have one set and one site. abid is the same in all lanes of a wave (a
// function of the step, or a kernel argument), so the branch is uniform.
template <int F>
__device__ __forceinline__ typename Acc<F>::type mac_abid(const uint32_t a[4], const uint32_t b[8],
                                                          uint32_t idx, uint32_t abid,
                                                          typename Acc<F>::type c) {
  if constexpr (F == GM_SPARSESCAN_IX_F16 || F == GM_SPARSESCAN_IX_BF16 ||
                F == GM_SPARSESCAN_IX_F16_32 || F == GM_SPARSESCAN_IX_BF16_32) {
    if (abid & 1u) return mac<F, 1>(a, b, idx, c);
  }
  return mac<F, 0>(a, b, idx, c);
}

// Accumulator register r as its bit pattern.
template <int F>
__device__ __forceinline__ uint32_t acc_word(const typename Acc<F>::type& c, int r) {
  if constexpr (Acc<F>::kInt) return (uint32_t)c[r];
  else return gm_cuscan_f32_bits(c[r]);
}

struct Lane {
  uint64_t seed;
  uint32_t iters, w, l;
};

template <int F>
__device__ __forceinline__ void fmt_any(const Lane& q, uint32_t sig[4]) {
  typename Acc<F>::type c = {};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[GM_SPARSESCAN_A_DWORDS], b[GM_SPARSESCAN_B_DWORDS], idx;
    gm_sparsescan_images<F>(q.seed, s, q.w, q.l, a, b, idx);
    c = mac_abid<F>(a, b, idx, gm_sparsescan_abid(F, s), c);
  }
  if constexpr (Acc<F>::kBig) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t bits[4] = {acc_word<F>(c, 4 * i), acc_word<F>(c, 4 * i + 1),
                                acc_word<F>(c, 4 * i + 2), acc_word<F>(c, 4 * i + 3)};
      sig[i] = gm_sparsescan_fold(bits);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) sig[i] = acc_word<F>(c, i);
  }
}

template <bool kCompare, int F>
__device__ __forceinline__ void one_format(const Params& p, const Lane& q, const Where& at,
                                           const uint32_t* __restrict__ expected, DevTable* tab,
                                           uint32_t* sig_out, uint32_t& failed, uint32_t& bad) {
  if (!(p.tests & (1u << F))) return;
  uint32_t sig[4];
  fmt_any<F>(q, sig);
  finish<kCompare>(p, 1u << F, F, at, sig, expected, tab, sig_out, failed, bad);
}

// kCompare / !kCompare as k_cuscan: the scan, or one block's raw signature of the one format in
// p.tests. The LDS is declared to keep the CU to one block and carries the block's outcome.
template <bool kCompare>
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_sparsescan(
    Params p, const uint32_t* __restrict__ expected, DevTable* tab, uint32_t* sig_out,
    uint32_t* where_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[GM_CUSCAN_LDS_WORDS];
  const Where at = where_am_i();
  const Lane q = {p.seed, p.iters, threadIdx.x >> 6, threadIdx.x & 63};
  uint32_t failed = 0, bad = 0;
  one_format<kCompare, 0>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 1>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 2>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 3>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 4>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 5>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 6>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 7>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 8>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 9>(p, q, at, expected, tab, sig_out, failed, bad);
  one_format<kCompare, 10>(p, q, at, expected, tab, sig_out, failed, bad);
  book_block<kCompare>(lds, at, failed, bad, tab, where_out);
}

// One instruction of form F per wave from a zero accumulator; thread t reads a[4 t ..], b[8 t ..]
// and idx[t] and stores its 16 output words (a 16x16 form: 4, then zeroes) at out[16 t ..].
template <int F>
__device__ __forceinline__ void apply_one(const uint32_t a[4], const uint32_t b[8], uint32_t idx,
                                          uint32_t abid, uint32_t* out) {
  typename Acc<F>::type c = {};
  c = mac_abid<F>(a, b, idx, abid, c);
#pragma unroll
  for (int r = 0; r < GM_SPARSESCAN_ACC_WORDS; ++r) {
    if constexpr (Acc<F>::kBig) out[r] = acc_word<F>(c, r);
    else out[r] = r < 4 ? acc_word<F>(c, r & 3) : 0u;
  }
}

__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_sparse_apply(
    uint32_t f, uint32_t abid, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in,
    const uint32_t* __restrict__ idx_in, uint32_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  const u32x4 va = ((const u32x4*)a_in)[t];
  const u32x4 b0 = ((const u32x4*)b_in)[2 * t], b1 = ((const u32x4*)b_in)[2 * t + 1];
  const uint32_t a[4] = {va.x, va.y, va.z, va.w};
  const uint32_t b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  const uint32_t idx = idx_in[t];
  uint32_t* o = out + GM_SPARSESCAN_ACC_WORDS * t;
  switch (f) {
    case 0: apply_one<0>(a, b, idx, abid, o); break;
    case 1: apply_one<1>(a, b, idx, abid, o); break;
    case 2: apply_one<2>(a, b, idx, abid, o); break;
    case 3: apply_one<3>(a, b, idx, abid, o); break;
    case 4: apply_one<4>(a, b, idx, abid, o); break;
    case 5: apply_one<5>(a, b, idx, abid, o); break;
    case 6: apply_one<6>(a, b, idx, abid, o); break;
    case 7: apply_one<7>(a, b, idx, abid, o); break;
    case 8: apply_one<8>(a, b, idx, abid, o); break;
    case 9: apply_one<9>(a, b, idx, abid, o); break;
    default: apply_one<10>(a, b, idx, abid, o); break;
  }
}

bool iters_ok(uint32_t, uint32_t iters) { return iters >= 1 && iters <= GM_SPARSESCAN_MAX_ITERS; }

constexpr ScanArgs kArgs = {GM_SPARSESCAN_ALL, iters_ok};

}  // namespace

extern "C" {

int gm_probe_sparsescan_expected(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* out) {
  if (!one_test_ok(kArgs, format, iters) || !out) return (int)hipErrorInvalidValue;
  gm_sparsescan_expected_host(format, seed, iters, out);
  return 0;
}

int gm_probe_sparsescan_images(uint32_t format, uint64_t seed, uint32_t step, uint32_t* a,
                               uint32_t* b, uint32_t* idx, uint32_t* abid) {
  if (!one_bit_ok(kArgs, format) || step >= GM_SPARSESCAN_MAX_ITERS || !a || !b || !idx || !abid)
    return (int)hipErrorInvalidValue;
  const int f = __builtin_ctz(format);
  for (uint32_t w = 0; w < 4; ++w)
    for (uint32_t l = 0; l < 64; ++l)
      gm_sparsescan_images_host(f, seed, step, w, l, a + (w * 64 + l) * GM_SPARSESCAN_A_DWORDS,
                                b + (w * 64 + l) * GM_SPARSESCAN_B_DWORDS, idx[w * 64 + l]);
  *abid = gm_sparsescan_abid(f, step);
  return 0;
}

int gm_probe_sparsescan_signature(uint32_t format, uint64_t seed, uint32_t iters,
                                  uint32_t* dev_out, uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, format, iters) || !signature_out_ok(dev_out, dev_where))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sparsescan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream,
                     params_of(seed, format, iters), (const uint32_t*)nullptr, (DevTable*)nullptr,
                     dev_out, dev_where);
  return (int)hipGetLastError();
}

int gm_probe_sparsescan_apply(uint32_t format, uint32_t abid, const uint32_t* dev_a,
                              const uint32_t* dev_b, const uint32_t* dev_idx, uint32_t* dev_out,
                              void* stream) {
  if (!one_bit_ok(kArgs, format) || abid > 1 || !dev_a || !dev_b || !dev_idx || !dev_out ||
      (((uintptr_t)dev_a | (uintptr_t)dev_b | (uintptr_t)dev_out) & 15) || ((uintptr_t)dev_idx & 3))
    return (int)hipErrorInvalidValue;
  const int f = __builtin_ctz(format);
  if (abid != 0 && !gm_sparsescan_wide(f)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_sparse_apply, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream,
                     (uint32_t)f, abid, dev_a, dev_b, dev_idx, dev_out);
  return (int)hipGetLastError();
}

int gm_probe_sparsescan(int dev, uint32_t formats_mask, uint32_t iters, uint64_t seed,
                        int min_rounds, int max_rounds, const gm_cuscan_inject_t* inject,
                        gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!scan_args_ok(kArgs, formats_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus))
    return (int)hipErrorInvalidValue;
  return run_scan(
      dev, k_sparsescan<true>, params_of(seed, formats_mask, iters, inject),
      (size_t)GM_SPARSESCAN_FORMATS * GM_CUSCAN_SIG_WORDS,
      [&](uint32_t* exp) {
        for (int f = 0; f < GM_SPARSESCAN_FORMATS; ++f)
          if (formats_mask & (1u << f))
            gm_sparsescan_expected_host(1u << f, seed, iters, exp + (size_t)f * GM_CUSCAN_SIG_WORDS);
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

}  // extern "C"
