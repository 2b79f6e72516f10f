// gm_mfmascan.hip — per-CU matrix-core format scan for gfx950: which CU's matrix cores compute a
// wrong word, and in which number format?
//
// One kernel, k_mfmascan, in the CU scan's frame (gm_cuscan_frame.h): a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU. Every wave
// runs `iters` dependent MFMAs of each selected format (f16, fp8, bf8, i8, f32, f64 and the five
// block-scaled f8f6f4 forms; 16x16 shapes) on operand images derived from the seed
// (gm_mfmascan_ref.h, formulas in gm_probe.h). Every product and partial sum is exact in the
// accumulator type, so the 4 accumulator registers of a lane are one definite bit pattern, which
// is compared with the table the host computed.
#include "gm_mfmascan_ref.h"

#include "gm_cuscan_frame.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Lane {
  uint64_t seed;
  uint32_t iters, w, l;
};

template <int F>
__device__ __forceinline__ void images(const Lane& q, uint32_t s, uint32_t a[8], uint32_t b[8]) {
  gm_mfmascan_image<F>(q.seed, s, q.w, 0, q.l, a);
  gm_mfmascan_image<F>(q.seed, s, q.w, 1, q.l, b);
}

__device__ __forceinline__ void store_f32(const f32x4& c, uint32_t sig[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = gm_cuscan_f32_bits(c[i]);
}

__device__ __forceinline__ void fmt_f16(const Lane& q, uint32_t sig[4]) {
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_F16>(q, s, a, b);
    const u32x4 va = {a[0], a[1], a[2], a[3]}, vb = {b[0], b[1], b[2], b[3]};
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, va),
                                               __builtin_bit_cast(f16x8, vb), c, 0, 0, 0);
  }
  store_f32(c, sig);
}

__device__ __forceinline__ void fmt_fp8(const Lane& q, uint32_t sig[4]) {
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_FP8>(q, s, a, b);
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)(a[0] | (uint64_t)a[1] << 32),
                                                   (long)(b[0] | (uint64_t)b[1] << 32), c, 0, 0, 0);
  }
  store_f32(c, sig);
}

__device__ __forceinline__ void fmt_bf8(const Lane& q, uint32_t sig[4]) {
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_BF8>(q, s, a, b);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)(a[0] | (uint64_t)a[1] << 32),
                                                   (long)(b[0] | (uint64_t)b[1] << 32), c, 0, 0, 0);
  }
  store_f32(c, sig);
}

__device__ __forceinline__ void fmt_i8(const Lane& q, uint32_t sig[4]) {
  i32x4 c = {0, 0, 0, 0};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_I8>(q, s, a, b);
    const i32x4 va = {(int)a[0], (int)a[1], (int)a[2], (int)a[3]},
                vb = {(int)b[0], (int)b[1], (int)b[2], (int)b[3]};
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(va, vb, c, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = (uint32_t)c[i];
}

__device__ __forceinline__ void fmt_f32(const Lane& q, uint32_t sig[4]) {
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_F32>(q, s, a, b);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(float, a[0]),
                                             __builtin_bit_cast(float, b[0]), c, 0, 0, 0);
  }
  store_f32(c, sig);
}

__device__ __forceinline__ void fmt_f64(const Lane& q, uint32_t sig[4]) {
  f64x4 c = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<GM_MFMASCAN_IX_F64>(q, s, a, b);
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(
        __builtin_bit_cast(double, a[0] | (uint64_t)a[1] << 32),
        __builtin_bit_cast(double, b[0] | (uint64_t)b[1] << 32), c, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = gm_mfmascan_f64_word(c[i]);
}

// The five block-scaled forms: F = GM_MFMASCAN_IX_MXFP8 + cbsz, A and B in the same format. The
// lane's scale byte is that of its row (A) / column (B), in byte 0 with opsel 0.
template <int F>
__device__ __forceinline__ void fmt_mx(const Lane& q, uint32_t sig[4]) {
  constexpr int kFmt = F - GM_MFMASCAN_IX_MXFP8;
  const int sa = (int)gm_mfmascan_scale(q.seed, F, q.w, 0, q.l & 15);
  const int sb = (int)gm_mfmascan_scale(q.seed, F, q.w, 1, q.l & 15);
  f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t s = 0; s < q.iters; ++s) {
    uint32_t a[8], b[8];
    images<F>(q, s, a, b);
    i32x8 va, vb;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      va[i] = (int)a[i];
      vb[i] = (int)b[i];
    }
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, vb, c, kFmt, kFmt, 0, sa, 0, sb);
  }
  store_f32(c, sig);
}

template <int F>
__device__ __forceinline__ void fmt_any(const Lane& q, uint32_t sig[4]) {
  if constexpr (F == GM_MFMASCAN_IX_F16) fmt_f16(q, sig);
  else if constexpr (F == GM_MFMASCAN_IX_FP8) fmt_fp8(q, sig);
  else if constexpr (F == GM_MFMASCAN_IX_BF8) fmt_bf8(q, sig);
  else if constexpr (F == GM_MFMASCAN_IX_I8) fmt_i8(q, sig);
  else if constexpr (F == GM_MFMASCAN_IX_F32) fmt_f32(q, sig);
  else if constexpr (F == GM_MFMASCAN_IX_F64) fmt_f64(q, sig);
  else fmt_mx<F>(q, sig);
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
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_mfmascan(
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

bool iters_ok(uint32_t, uint32_t iters) { return iters >= 1 && iters <= GM_MFMASCAN_MAX_ITERS; }

constexpr ScanArgs kArgs = {GM_MFMASCAN_ALL, iters_ok};

}  // namespace

extern "C" {

int gm_probe_mfmascan_expected(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* out) {
  if (!one_test_ok(kArgs, format, iters) || !out) return (int)hipErrorInvalidValue;
  gm_mfmascan_expected_host(format, seed, iters, out);
  return 0;
}

int gm_probe_mfmascan_images(uint32_t format, uint64_t seed, uint32_t step, uint32_t* images,
                             uint32_t* scales) {
  if (!one_bit_ok(kArgs, format) || step >= GM_MFMASCAN_MAX_ITERS || !images || !scales)
    return (int)hipErrorInvalidValue;
  const int f = __builtin_ctz(format);
  for (uint32_t w = 0; w < 4; ++w)
    for (uint32_t m = 0; m < 2; ++m) {
      for (uint32_t l = 0; l < 64; ++l)
        gm_mfmascan_image_host(f, seed, step, w, m, l, images + ((w * 2 + m) * 64 + l) * 8);
      for (uint32_t r = 0; r < 16; ++r)
        scales[(w * 2 + m) * 16 + r] =
            gm_mfmascan_scaled(f) ? gm_mfmascan_scale(seed, f, w, m, r) : 127u;
    }
  return 0;
}

int gm_probe_mfmascan_signature(uint32_t format, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                                uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, format, iters) || !signature_out_ok(dev_out, dev_where))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mfmascan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream,
                     params_of(seed, format, iters), (const uint32_t*)nullptr, (DevTable*)nullptr,
                     dev_out, dev_where);
  return (int)hipGetLastError();
}

int gm_probe_mfmascan(int dev, uint32_t formats_mask, uint32_t iters, uint64_t seed,
                      int min_rounds, int max_rounds, const gm_cuscan_inject_t* inject,
                      gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!scan_args_ok(kArgs, formats_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus))
    return (int)hipErrorInvalidValue;
  return run_scan(
      dev, k_mfmascan<true>, params_of(seed, formats_mask, iters, inject),
      (size_t)GM_MFMASCAN_FORMATS * GM_CUSCAN_SIG_WORDS,
      [&](uint32_t* exp) {
        for (int f = 0; f < GM_MFMASCAN_FORMATS; ++f)
          if (formats_mask & (1u << f))
            gm_mfmascan_expected_host(1u << f, seed, iters, exp + (size_t)f * GM_CUSCAN_SIG_WORDS);
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

}  // extern "C"
