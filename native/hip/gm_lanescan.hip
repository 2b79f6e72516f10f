// gm_lanescan.hip — per-CU register, lane and scalar-unit scan for gfx950: which CU's lane
// crossbar, register file, scalar unit, transcendental pipe, fp64 pipe or packed arithmetic
// computes a wrong word?
//
// One kernel, k_lanescan, in the CU scan's frame (gm_cuscan_frame.h): a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU and one wave per
// SIMD. Six known-answer tests of 4 signature words per thread; the data formulas are
// gm_lanescan_ref.h (shared with the host, written out in gm_probe.h). The operation under test
// is the instruction here, through its builtin, and a plain model on the host.
//
// `expected` starts with the scalar test's read-only table (GM_LANESCAN_TABLE_WORDS), then one
// block of signature words per test: finish() is handed test index + 1.
#include "gm_lanescan_ref.h"

#include "gm_cuscan_frame.h"

namespace {

typedef uint32_t u32x32 __attribute__((ext_vector_type(32)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
typedef int16_t i16x2 __attribute__((ext_vector_type(2)));

struct Lane {
  uint64_t seed;
  uint32_t iters, t, w, l;
};

// ================================================================================ xlane
// One movement of the menu. `entry` and `g` are uniform, so the switch is a scalar branch and
// every lane is active in every case; the DPP controls and swizzle offsets are immediates.
__device__ __forceinline__ uint32_t xlane_move(uint32_t entry, uint32_t g, uint32_t old,
                                               uint32_t src, uint32_t l) {
  switch (entry) {
#define GM_LANESCAN_CASE(i, ctrl, rm, bm, bc) \
  case i: return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, ctrl, rm, bm, bc != 0);
    GM_LANESCAN_DPP_MENU(GM_LANESCAN_CASE)
#undef GM_LANESCAN_CASE
#define GM_LANESCAN_CASE(i, off) \
  case i: return (uint32_t)__builtin_amdgcn_ds_swizzle((int)src, off);
    GM_LANESCAN_SWIZZLE_MENU(GM_LANESCAN_CASE)
#undef GM_LANESCAN_CASE
    case GM_LANESCAN_MV_BPERMUTE:
      return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(gm_lanescan_affine_lane(l, g) * 4), (int)src);
    case GM_LANESCAN_MV_BPERMUTE_MANY:
      return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(gm_lanescan_many_lane(l, g) * 4), (int)src);
    case GM_LANESCAN_MV_PERMUTE:
      return (uint32_t)__builtin_amdgcn_ds_permute((int)(gm_lanescan_affine_lane(l, g) * 4), (int)src);
    case GM_LANESCAN_MV_READLANE:
      return (uint32_t)__builtin_amdgcn_readlane((int)src, (int)(g & 63u));
    case GM_LANESCAN_MV_READFIRSTLANE:
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)src);
    case GM_LANESCAN_MV_WRITELANE: {
      // v_writelane takes one SGPR on gfx9, the value; the lane select is an inline constant. The
      // value comes from a VALU write of an SGPR (readlane): the wait states before v_writelane
      // reads it are inside the statement.
      const uint32_t value = (uint32_t)__builtin_amdgcn_readlane((int)src, (int)((g >> 8) & 63u));
#define GM_LANESCAN_WRITELANE(lane) \
  asm volatile("s_nop 4\n\tv_writelane_b32 %0, %1, " #lane : "+v"(old) : "s"(value))
      switch (g & 3u) {
        case 0: GM_LANESCAN_WRITELANE(0); break;
        case 1: GM_LANESCAN_WRITELANE(21); break;
        case 2: GM_LANESCAN_WRITELANE(42); break;
        default: GM_LANESCAN_WRITELANE(63); break;
      }
#undef GM_LANESCAN_WRITELANE
      return old;
    }
    case GM_LANESCAN_MV_PERMLANE16_SWAP: {
      const auto r = __builtin_amdgcn_permlane16_swap(old, src, false, false);
      return r[0] + gm_cuscan_rotl32(r[1], 13);
    }
    case GM_LANESCAN_MV_PERMLANE32_SWAP: {
      const auto r = __builtin_amdgcn_permlane32_swap(old, src, false, false);
      return r[0] + gm_cuscan_rotl32(r[1], 13);
    }
    default: {  // GM_LANESCAN_MV_BALLOT_MBCNT
      const uint64_t ballot = __builtin_amdgcn_ballot_w64(((src >> (g & 31u)) & 1u) != 0);
      const uint32_t lo = (uint32_t)ballot, hi = (uint32_t)(ballot >> 32);
      return (old ^ lo ^ hi) + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    }
  }
}

__device__ __forceinline__ void test_xlane(const Lane& q, uint32_t sig[4]) {
  uint32_t x[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) x[j] = gm_lanescan_xlane_init(q.seed, q.t, j);
  // four steps at a time, so that x[] is indexed by constants
  for (uint32_t s4 = 0; s4 < q.iters * GM_LANESCAN_XLANE_MENU; s4 += 4) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t s = s4 + j;
      if (s < q.iters * GM_LANESCAN_XLANE_MENU) {
        const uint32_t entry = __builtin_amdgcn_readfirstlane(gm_lanescan_xlane_entry(q.seed, s));
        const uint32_t g = __builtin_amdgcn_readfirstlane(gm_lanescan_xlane_param(q.seed, s));
        x[j] = gm_lanescan_xlane_mix(xlane_move(entry, g, x[(j + 1) & 3], x[j], q.l), x[j], q.l, s);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sig[j] = x[j];
}

// ================================================================================ regfile
// 6 banks of 32 VGPRs indexed at run time (a single array of more than 32 dwords would go to
// scratch) and 192 accumulation registers reached through single-instruction statements that name
// no register. An accumulation register is written 191 such statements or more before it is read
// again, far beyond any wait state between the pair.
__device__ __forceinline__ uint32_t acc_read(const uint32_t& a) {
  uint32_t v;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
  return v;
}
__device__ __forceinline__ void acc_write(uint32_t& a, uint32_t v) {
  asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(a) : "v"(v));
}

// The banks are six local vectors worked on in place (behind references they end up in scratch),
// hence macros: B is the bank's number.
#define GM_LANESCAN_BANKS(X) X(0) X(1) X(2) X(3) X(4) X(5)
#define GM_LANESCAN_FILL(B) \
  _Pragma("unroll") for (uint32_t i = 0; i < 32; ++i) bank##B[i] = gm_lanescan_reg_fill(q.seed, q.t, B * 32 + i);
// register b * 32 + idx (b uniform): fold it into s[k & 3] and store its complement
#define GM_LANESCAN_TOUCH(B)             \
  if (b == B) {                          \
    const uint32_t got = bank##B[idx];   \
    s[k & 3] = gm_lanescan_fold(s[k & 3], got); \
    bank##B[idx] = ~got;                 \
  }
// every register of the bank by constant index: fold it and store its complement
#define GM_LANESCAN_SWEEP(B)                             \
  _Pragma("unroll") for (uint32_t i = 0; i < 32; ++i) {  \
    s[i & 3] = gm_lanescan_fold(s[i & 3], bank##B[i]);   \
    bank##B[i] = ~bank##B[i];                            \
  }
#define GM_LANESCAN_READBACK(B) \
  _Pragma("unroll") for (uint32_t i = 0; i < 32; ++i) s[i & 3] = gm_lanescan_fold(s[i & 3], bank##B[i]);

__device__ __forceinline__ void test_regfile(const Lane& q, uint32_t sig[4]) {
  u32x32 bank0, bank1, bank2, bank3, bank4, bank5;
  uint32_t acc[GM_LANESCAN_REG_ACCS];
  uint32_t s[4] = {0, 0, 0, 0};
  GM_LANESCAN_BANKS(GM_LANESCAN_FILL)
#pragma unroll
  for (uint32_t r = 0; r < GM_LANESCAN_REG_ACCS; ++r)
    acc_write(acc[r], gm_lanescan_reg_fill(q.seed, q.t, GM_LANESCAN_REG_VGPRS + r));
  for (uint32_t round = 0; round < q.iters; ++round) {
#pragma unroll
    for (uint32_t k = 0; k < GM_LANESCAN_REG_UNIFORM_STEPS + GM_LANESCAN_REG_LANE_STEPS; ++k) {
      const uint32_t g = __builtin_amdgcn_readfirstlane(gm_lanescan_reg_step(q.seed, round, k));
      // the first steps index by a uniform register number, the last by one that differs per lane
      const uint32_t r = g % GM_LANESCAN_REG_VGPRS;
      const uint32_t b = k < GM_LANESCAN_REG_UNIFORM_STEPS ? r >> 5 : g % GM_LANESCAN_REG_BANKS;
      const uint32_t idx = k < GM_LANESCAN_REG_UNIFORM_STEPS ? r & 31u : ((g >> 8) + q.l) & 31u;
      GM_LANESCAN_BANKS(GM_LANESCAN_TOUCH)
    }
    GM_LANESCAN_BANKS(GM_LANESCAN_SWEEP)
#pragma unroll
    for (uint32_t r = 0; r < GM_LANESCAN_REG_ACCS; ++r) {
      const uint32_t v = acc_read(acc[r]);
      s[r & 3] = gm_lanescan_fold(s[r & 3], v);
      acc_write(acc[r], ~v);
    }
  }
  GM_LANESCAN_BANKS(GM_LANESCAN_READBACK)
#pragma unroll
  for (uint32_t r = 0; r < GM_LANESCAN_REG_ACCS; ++r)
    s[r & 3] = gm_lanescan_fold(s[r & 3], acc_read(acc[r]));
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = s[i];
}
#undef GM_LANESCAN_FILL
#undef GM_LANESCAN_TOUCH
#undef GM_LANESCAN_SWEEP
#undef GM_LANESCAN_READBACK
#undef GM_LANESCAN_BANKS

// ================================================================================ salu
// One dependent chain per wave on uniform values (kernel arguments and the wave number through
// readfirstlane), in plain C++: the compiler keeps it on the scalar unit, and the table reads at
// uniform addresses through a const __restrict__ kernel argument are scalar loads.
__device__ __forceinline__ void test_salu(const Lane& q, const uint32_t* __restrict__ table,
                                          uint32_t sig[4]) {
  const uint32_t w = __builtin_amdgcn_readfirstlane(q.w);
  uint32_t v[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) v[i] = gm_cuscan_hash(q.seed, GM_LANESCAN_H_SALU_LANE, 4 * q.t + i);
  uint32_t a = gm_cuscan_hash(q.seed, GM_LANESCAN_H_SALU, 4 * w);
  uint32_t b = gm_cuscan_hash(q.seed, GM_LANESCAN_H_SALU, 4 * w + 1);
  uint64_t c = (uint64_t)gm_cuscan_hash(q.seed, GM_LANESCAN_H_SALU, 4 * w + 2) << 32 |
               gm_cuscan_hash(q.seed, GM_LANESCAN_H_SALU, 4 * w + 3);
  for (uint32_t s = 0; s < q.iters * GM_LANESCAN_SALU_STEPS; ++s) {
    const uint32_t k = table[(a ^ s) & (GM_LANESCAN_TABLE_WORDS - 1)];
    const uint32_t hi = __umulhi(a, k), lo = a * k;  // 32 x 32 multiply, low and high
    a ^= hi;
    b += lo;
    c += (uint64_t)b << 32 | a;                      // 64-bit add and subtract
    c -= k;
    a ^= b << (k & 31u);                             // the three kinds of shift
    b ^= a >> ((k >> 5) & 31u);
    a += (uint32_t)((int32_t)b >> ((k >> 10) & 31u));
    const uint32_t r = ((k >> 15) & 31u) + 1u;       // 64-bit rotate by 1..32
    c = c << r | c >> (64u - r);
    const uint32_t off = (k >> 20) & 15u, wd = ((k >> 24) & 15u) + 1u;
    const uint32_t e = (a >> off) & ((1u << wd) - 1u);                               // fields
    const uint32_t se = (uint32_t)((int32_t)(b << (32u - off - wd)) >> (32u - wd));
    b += (uint32_t)__builtin_popcount(a) + 33u * (a ? (uint32_t)__builtin_ctz(a) : 32u) +
         97u * (b ? (uint32_t)__builtin_clz(b) : 32u);
    a ^= __builtin_bitreverse32(b);
    a = a < b ? a + e : a - se;                      // compare and select
    const uint32_t mx = b > k ? b : k;               // unsigned max, signed min
    const int32_t mn = (int32_t)a < (int32_t)k ? (int32_t)a : (int32_t)k;
    b = mx - (uint32_t)mn;
    a += (int32_t)a > (int32_t)b ? a - b : b - a;    // absolute difference of the signed values
    a ^= (uint32_t)c;
    b ^= (uint32_t)(c >> 32);
    gm_lanescan_salu_fold(v, s, q.l, a, b);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = v[i];
}

// ================================================================================ trans
__device__ __forceinline__ float pow2_f32(int e, uint32_t neg = 0) {
  return __builtin_bit_cast(float, neg << 31 | (uint32_t)(127 + e) << 23);
}
__device__ __forceinline__ double pow2_f64(int e, uint32_t neg = 0) {
  return __builtin_bit_cast(double, (uint64_t)neg << 63 | (uint64_t)(1023 + e) << 52);
}
__device__ __forceinline__ _Float16 pow2_f16(int e) {
  return __builtin_bit_cast(_Float16, (uint16_t)((15 + e) << 10));
}
__device__ __forceinline__ uint32_t f64_word(double d) {
  return gm_lanescan_word64(__builtin_bit_cast(uint64_t, d));
}
__device__ __forceinline__ uint32_t f16_bits(_Float16 h) {
  return __builtin_bit_cast(uint16_t, h);
}
// the sign of a zero is not part of the test
__device__ __forceinline__ uint32_t f32_bits_nz(float f) {
  return f == 0.0f ? 0u : gm_cuscan_f32_bits(f);
}

__device__ __forceinline__ void test_trans(const Lane& q, uint32_t sig[4]) {
  constexpr uint32_t kOps = GM_LANESCAN_TRANS_OPS;
  uint32_t g[4];
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) g[i] = gm_lanescan_trans_init(q.seed, q.t, i);
  for (uint32_t s = 0; s < q.iters * GM_LANESCAN_TRANS_STEPS; ++s) {
    const gm_lanescan_trans_pt p = gm_lanescan_trans_point(q.seed, s, q.t, g[0] & 1u);
    if constexpr (kOps & GM_LANESCAN_OP_EXP)
      g[0] = gm_lanescan_fold(g[0], gm_cuscan_f32_bits(__builtin_amdgcn_exp2f((float)p.n)));
    if constexpr (kOps & GM_LANESCAN_OP_LOG)
      g[0] = gm_lanescan_fold(g[0], f32_bits_nz(__builtin_amdgcn_logf(pow2_f32(p.n))));
    if constexpr (kOps & GM_LANESCAN_OP_RCP)
      g[0] = gm_lanescan_fold(g[0], gm_cuscan_f32_bits(__builtin_amdgcn_rcpf(pow2_f32(p.n, p.neg))));
    if constexpr (kOps & GM_LANESCAN_OP_RSQ)
      g[0] = gm_lanescan_fold(g[0], gm_cuscan_f32_bits(__builtin_amdgcn_rsqf(pow2_f32(2 * p.k))));
    if constexpr (kOps & GM_LANESCAN_OP_SQRT)
      g[0] = gm_lanescan_fold(g[0], f32_bits_nz(__builtin_amdgcn_sqrtf((float)(p.m * p.m))));
    const float turns = (float)p.a * 0.25f;
    if constexpr (kOps & GM_LANESCAN_OP_SIN)
      g[1] = gm_lanescan_fold(g[1], f32_bits_nz(__builtin_amdgcn_sinf(turns)));
    if constexpr (kOps & GM_LANESCAN_OP_COS)
      g[1] = gm_lanescan_fold(g[1], f32_bits_nz(__builtin_amdgcn_cosf(turns)));
    if constexpr (kOps & GM_LANESCAN_OP_RCP64)
      g[2] = gm_lanescan_fold(g[2], f64_word(__builtin_amdgcn_rcp(pow2_f64(p.n, p.neg))));
    if constexpr (kOps & GM_LANESCAN_OP_SQRT64)
      g[2] = gm_lanescan_fold(g[2], f64_word(__builtin_amdgcn_sqrt(pow2_f64(2 * p.k))));
    if constexpr (kOps & GM_LANESCAN_OP_RSQ64)
      g[2] = gm_lanescan_fold(g[2], f64_word(__builtin_amdgcn_rsq(pow2_f64(2 * p.k))));
    if constexpr (kOps & GM_LANESCAN_OP_RCP16)
      g[3] = gm_lanescan_fold(g[3], f16_bits(__builtin_amdgcn_rcph(pow2_f16(p.k))));
    if constexpr (kOps & GM_LANESCAN_OP_SQRT16)
      g[3] = gm_lanescan_fold(g[3], f16_bits(__builtin_amdgcn_sqrth(pow2_f16(2 * p.k16))));
    if constexpr (kOps & GM_LANESCAN_OP_RSQ16)
      g[3] = gm_lanescan_fold(g[3], f16_bits(__builtin_amdgcn_rsqh(pow2_f16(2 * p.k16))));
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = g[i];
}

// ================================================================================ f64
// Every intermediate is an integer below 2^53 times a power of two (gm_lanescan_ref.h), so the
// multiply and the add below give the same bits fused or not; contraction is off so that both
// instructions run.
__device__ __forceinline__ void test_f64(const Lane& q, uint32_t sig[4]) {
#pragma clang fp contract(off)
  double x = (double)gm_lanescan_f64_init(q.seed, q.t), sum = 0.0;
  uint32_t g[4] = {0, 0, 0, 0};
  for (uint32_t s = 0; s < q.iters * GM_LANESCAN_F64_STEPS; ++s) {
    const gm_lanescan_f64_pt pt = gm_lanescan_f64_point(q.seed, s, q.t);
    const double p = __builtin_fma(x, (double)pt.a, (double)pt.b);
    sum += p;
    const double m = __builtin_ldexp(p, pt.e - 3) * (double)pt.c;
    const double r = m + __builtin_ldexp((double)pt.d, -3);
    const double fl = __builtin_floor(r);
    const double hi = __builtin_floor(__builtin_ldexp(fl, -GM_LANESCAN_F64_X_BITS));
    x = __builtin_fma(hi, -(double)(1 << GM_LANESCAN_F64_X_BITS), fl);
    const uint32_t eighths = (uint32_t)__builtin_ldexp(r - fl, 3);
    const uint32_t u = (uint32_t)x;
    x = (double)u;
    const int32_t trunc = (int32_t)__builtin_ldexp(p, -12);
    g[0] = gm_lanescan_fold(g[0], f64_word(p));
    g[1] = gm_lanescan_fold(g[1], f64_word(r));
    g[2] = gm_lanescan_fold(g[2], (u ^ eighths << 28) + (uint32_t)trunc);
  }
  g[3] = f64_word(sum);
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = g[i];
}

// ================================================================================ packed
__device__ __forceinline__ void test_packed(const Lane& q, uint32_t sig[4]) {
  f32x2 acc = {0.0f, 0.0f};
  int32_t sdot = 0;
  uint32_t udot = 0;
  float fdot = 0.0f, bdot = 0.0f;
  uint32_t g[4] = {0, 0, 0, 0};
  for (uint32_t s = 0; s < q.iters * GM_LANESCAN_PACKED_STEPS; ++s) {
    uint32_t h[4];
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) h[i] = gm_lanescan_packed_hash(q.seed, s, q.t, i);
    const f32x2 a2 = {(float)(int8_t)h[0], (float)(int8_t)(h[0] >> 8)},
                b2 = {(float)(int8_t)(h[0] >> 16), (float)(int8_t)(h[0] >> 24)};
    acc = __builtin_elementwise_fma(a2, b2, acc);
    float sm[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) sm[i] = (float)gm_lanescan_packed_small(h[1], i);
    const f16x2 pa = {(_Float16)sm[0], (_Float16)sm[1]}, pb = {(_Float16)sm[2], (_Float16)sm[3]},
                pc = {(_Float16)sm[4], (_Float16)sm[5]};
    const f16x2 fm = __builtin_elementwise_fma(pa, pb, pc);
    f16x2 ad, ml;
    {
#pragma clang fp contract(off)
      ad = fm + pb;
      ml = pa * pc;
    }
    g[0] = gm_lanescan_fold(g[0], __builtin_bit_cast(uint32_t, fm));
    g[0] = gm_lanescan_fold(g[0], __builtin_bit_cast(uint32_t, ad));
    g[0] = gm_lanescan_fold(g[0], __builtin_bit_cast(uint32_t, ml));
    const u16x2 ua = __builtin_bit_cast(u16x2, h[2]), ub = __builtin_bit_cast(u16x2, h[3]);
    const i16x2 ia = __builtin_bit_cast(i16x2, h[2]), ib = __builtin_bit_cast(i16x2, h[3]);
    g[1] = gm_lanescan_fold(g[1], __builtin_bit_cast(uint32_t, (u16x2)(ua * ub)));
    g[1] = gm_lanescan_fold(g[1], __builtin_bit_cast(uint32_t, (u16x2)(ua + ub)));
    g[1] = gm_lanescan_fold(g[1], __builtin_bit_cast(uint32_t, (u16x2)(ua - ub)));
    g[1] = gm_lanescan_fold(g[1], __builtin_bit_cast(uint32_t, __builtin_elementwise_max(ia, ib)));
    g[1] = gm_lanescan_fold(g[1], __builtin_bit_cast(uint32_t, __builtin_elementwise_min(ua, ub)));
    sdot = __builtin_amdgcn_sdot4((int)h[2], (int)h[3], sdot, false);
    udot = __builtin_amdgcn_udot4(h[2], h[3], udot, false);
    fdot = __builtin_amdgcn_fdot2(pa, pb, fdot, false);
    const bf16x2 ba = {(__bf16)sm[0], (__bf16)sm[1]}, bc = {(__bf16)sm[4], (__bf16)sm[5]};
    bdot = __builtin_amdgcn_fdot2_f32_bf16(ba, bc, bdot, false);
  }
  g[2] = gm_cuscan_f32_bits(acc.x) + gm_cuscan_rotl32(gm_cuscan_f32_bits(acc.y), 11);
  g[3] = (uint32_t)sdot ^ gm_cuscan_rotl32(udot, 8) ^ gm_cuscan_f32_bits(fdot) ^
         gm_cuscan_rotl32(gm_cuscan_f32_bits(bdot), 24);
#pragma unroll
  for (int i = 0; i < 4; ++i) sig[i] = g[i];
}

template <bool kCompare, int T>
__device__ __forceinline__ void one_test(const Params& p, const Lane& q, const Where& at,
                                         const uint32_t* __restrict__ expected, DevTable* tab,
                                         uint32_t* sig_out, uint32_t& failed, uint32_t& bad) {
  if (!(p.tests & (1u << T))) return;
  uint32_t sig[4];
  if constexpr (T == GM_LANESCAN_IX_XLANE) test_xlane(q, sig);
  else if constexpr (T == GM_LANESCAN_IX_REGFILE) test_regfile(q, sig);
  else if constexpr (T == GM_LANESCAN_IX_SALU) test_salu(q, expected, sig);
  else if constexpr (T == GM_LANESCAN_IX_TRANS) test_trans(q, sig);
  else if constexpr (T == GM_LANESCAN_IX_F64) test_f64(q, sig);
  else test_packed(q, sig);
  // the table of test T follows the scalar test's table: block T + 1 of `expected`
  finish<kCompare>(p, 1u << T, T + 1, at, sig, expected, tab, sig_out, failed, bad);
}

// kCompare / !kCompare as k_cuscan: the scan, or one block's raw signature of the one test in
// p.tests. In both forms `expected` holds the scalar test's table in its first
// GM_LANESCAN_TABLE_WORDS words. The LDS is declared to keep the CU to one block and carries the
// block's outcome.
template <bool kCompare>
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_lanescan(
    Params p, const uint32_t* __restrict__ expected, DevTable* tab, uint32_t* sig_out,
    uint32_t* where_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[GM_CUSCAN_LDS_WORDS];
  const Where at = where_am_i();
  const Lane q = {p.seed, p.iters, threadIdx.x, threadIdx.x >> 6, threadIdx.x & 63};
  uint32_t failed = 0, bad = 0;
  one_test<kCompare, 0>(p, q, at, expected, tab, sig_out, failed, bad);
  one_test<kCompare, 1>(p, q, at, expected, tab, sig_out, failed, bad);
  one_test<kCompare, 2>(p, q, at, expected, tab, sig_out, failed, bad);
  one_test<kCompare, 3>(p, q, at, expected, tab, sig_out, failed, bad);
  one_test<kCompare, 4>(p, q, at, expected, tab, sig_out, failed, bad);
  one_test<kCompare, 5>(p, q, at, expected, tab, sig_out, failed, bad);
  book_block<kCompare>(lds, at, failed, bad, tab, where_out);
}

bool iters_ok(uint32_t, uint32_t iters) { return iters >= 1 && iters <= GM_LANESCAN_MAX_ITERS; }

constexpr ScanArgs kArgs = {GM_LANESCAN_ALL, iters_ok};

void fill_table(uint64_t seed, uint32_t* table) {
  for (uint32_t i = 0; i < GM_LANESCAN_TABLE_WORDS; ++i) table[i] = gm_lanescan_salu_table(seed, i);
}

}  // namespace

extern "C" {

int gm_probe_lanescan_expected(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* out) {
  if (!one_test_ok(kArgs, test, iters) || !out) return (int)hipErrorInvalidValue;
  gm_lanescan_expected_host(test, seed, iters, out);
  return 0;
}

int gm_probe_lanescan_lanes(uint32_t* menu, int menu_cap, int* n_menu, uint32_t* trans_ops) {
  if (!menu || menu_cap < GM_LANESCAN_XLANE_MENU || !n_menu || !trans_ops)
    return (int)hipErrorInvalidValue;
  const gm_lanescan_menu_t* m = gm_lanescan_menu();
  for (int i = 0; i < GM_LANESCAN_XLANE_MENU; ++i) {
    menu[5 * i] = m[i].kind;
    menu[5 * i + 1] = m[i].imm;
    menu[5 * i + 2] = m[i].row_mask;
    menu[5 * i + 3] = m[i].bank_mask;
    menu[5 * i + 4] = m[i].bound_ctrl;
  }
  *n_menu = GM_LANESCAN_XLANE_MENU;
  *trans_ops = GM_LANESCAN_TRANS_OPS;
  return 0;
}

int gm_probe_lanescan_signature(uint32_t test, uint64_t seed, uint32_t iters, uint32_t* dev_out,
                                uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, test, iters) || !signature_out_ok(dev_out, dev_where))
    return (int)hipErrorInvalidValue;
  // the scalar test's table: copied in on the stream, and the buffer is freed once the block
  // that reads it is done
  DevBuf dtable;
  std::vector<uint32_t> table(GM_LANESCAN_TABLE_WORDS);
  fill_table(seed, table.data());
  GM_CHECK(dtable.alloc(table.size() * sizeof(uint32_t)));
  GM_CHECK(hipMemcpyAsync(dtable.p, table.data(), table.size() * sizeof(uint32_t),
                          hipMemcpyHostToDevice, (hipStream_t)stream));
  hipLaunchKernelGGL(k_lanescan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream,
                     params_of(seed, test, iters), (const uint32_t*)dtable.p, (DevTable*)nullptr,
                     dev_out, dev_where);
  GM_CHECK(hipGetLastError());
  GM_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int gm_probe_lanescan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                      int max_rounds, const gm_cuscan_inject_t* inject, gm_cuscan_result_t* out,
                      gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!scan_args_ok(kArgs, tests_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus))
    return (int)hipErrorInvalidValue;
  return run_scan(
      dev, k_lanescan<true>, params_of(seed, tests_mask, iters, inject),
      (size_t)GM_LANESCAN_EXPECTED_WORDS,
      [&](uint32_t* exp) {
        fill_table(seed, exp);
        for (int t = 0; t < GM_LANESCAN_TESTS; ++t)
          if (tests_mask & (1u << t))
            gm_lanescan_expected_host(1u << t, seed, iters,
                                      exp + GM_LANESCAN_TABLE_WORDS + (size_t)t * GM_CUSCAN_SIG_WORDS);
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

int gm_probe_lanescan_kernel_info(int* num_regs, int* scratch_bytes) {
  if (!num_regs || !scratch_bytes) return (int)hipErrorInvalidValue;
  hipFuncAttributes attr;
  GM_CHECK(hipFuncGetAttributes(&attr, (const void*)k_lanescan<true>));
  *num_regs = attr.numRegs;
  *scratch_bytes = (int)attr.localSizeBytes;
  return 0;
}

}  // extern "C"
