// gm_lanescan_ref.h — the lane scan's value model: test bits, caps, the data formulas (one
// definition for the host and for the gfx950 kernel, native/hip/gm_lanescan.hip) and the host
// evaluation of a block's expected table.
// The formulas are written out in gm_probe.h; this is their only implementation.
//
// What is shared is data: hashes, operand values, menus of immediates, the folds. The operation
// under test is not. On the device it is the instruction; here it is a plain model of what the
// ISA document says the instruction does (a lane permutation over a 64-entry array, an array
// index, uint64_t arithmetic, integers standing in for floating point), so a unit that computes
// wrongly cannot produce its own expected value.
#pragma once
#include <stdint.h>

#include "gm_cuscan_sig.h"

enum {
  GM_LANESCAN_XLANE = 1,    // DPP, ds_bpermute / permute / swizzle, read/writelane, permlane swaps
  GM_LANESCAN_REGFILE = 2,  // 192 indexed VGPRs + 192 accumulation registers per lane
  GM_LANESCAN_SALU = 4,     // the scalar ALU and the scalar data cache
  GM_LANESCAN_TRANS = 8,    // v_exp / log / rcp / rsq / sqrt / sin / cos at exact points
  GM_LANESCAN_F64 = 16,     // v_fma / mul / add / ldexp / floor / cvt in fp64
  GM_LANESCAN_PACKED = 32,  // v_pk_* and v_dot*
  GM_LANESCAN_ALL = 63,
};
enum {
  GM_LANESCAN_IX_XLANE, GM_LANESCAN_IX_REGFILE, GM_LANESCAN_IX_SALU, GM_LANESCAN_IX_TRANS,
  GM_LANESCAN_IX_F64, GM_LANESCAN_IX_PACKED,
};

#define GM_LANESCAN_TESTS 6
#define GM_LANESCAN_DEFAULT_ITERS 16
#define GM_LANESCAN_MAX_ITERS 63        /* the smallest of the caps below (packed) */
/* hash test ids: disjoint from the CU scan's (1..8), the atomics' (0x100..) and the format
   scan's (0x200..) */
#define GM_LANESCAN_H_XLANE 0x300u
#define GM_LANESCAN_H_XLANE_STEP 0x301u
#define GM_LANESCAN_H_REG 0x310u
#define GM_LANESCAN_H_REG_STEP 0x311u
#define GM_LANESCAN_H_SALU_TABLE 0x320u
#define GM_LANESCAN_H_SALU 0x321u
#define GM_LANESCAN_H_SALU_LANE 0x322u
#define GM_LANESCAN_H_TRANS 0x330u
#define GM_LANESCAN_H_TRANS_INIT 0x331u
#define GM_LANESCAN_H_F64 0x340u
#define GM_LANESCAN_H_F64_STEP 0x341u
#define GM_LANESCAN_H_PACKED 0x350u

// The expected table handed to the kernel: the scalar test's read-only table first, then one
// block of signature words per test.
#define GM_LANESCAN_TABLE_WORDS 1024    /* 4 KiB */
#define GM_LANESCAN_EXPECTED_WORDS (GM_LANESCAN_TABLE_WORDS + GM_LANESCAN_TESTS * GM_CUSCAN_SIG_WORDS)

// the fold every test but salu uses for what it read
GM_CUSCAN_HD uint32_t gm_lanescan_fold(uint32_t s, uint32_t v) {
  return gm_cuscan_rotl32(s, 5) + v;
}

// ================================================================================ xlane
// The menu: one movement per entry, its immediates shared with the kernel's switch. A step s
// runs entry (s + H(0x301, 0)) % MENU with the uniform parameter word g = H(0x301, 1 + s), so
// every `iters` unit passes through the whole menu once.
//   DPP(index, dpp_ctrl, row_mask, bank_mask, bound_ctrl)
#define GM_LANESCAN_DPP_MENU(X)                                                           \
  X(0, 0x01B, 0xF, 0xF, 0)  /* quad_perm:[3,2,1,0] */                                     \
  X(1, 0x04E, 0xF, 0x5, 1)  /* quad_perm:[2,3,0,1] */                                     \
  X(2, 0x0B1, 0x6, 0xF, 0)  /* quad_perm:[1,0,3,2] */                                     \
  X(3, 0x000, 0xF, 0xA, 0)  /* quad_perm:[0,0,0,0] */                                     \
  X(4, 0x101, 0xF, 0xF, 1)  /* row_shl:1 */                                               \
  X(5, 0x107, 0xF, 0xF, 0)  /* row_shl:7 */                                               \
  X(6, 0x10F, 0x9, 0xF, 1)  /* row_shl:15 */                                              \
  X(7, 0x111, 0xF, 0xF, 0)  /* row_shr:1 */                                               \
  X(8, 0x112, 0xF, 0xF, 1)  /* row_shr:2 */                                               \
  X(9, 0x113, 0xF, 0xC, 0)  /* row_shr:3 */                                               \
  X(10, 0x114, 0xF, 0xE, 1) /* row_shr:4 */                                               \
  X(11, 0x118, 0x5, 0xF, 0) /* row_shr:8 */                                               \
  X(12, 0x11F, 0xF, 0xF, 1) /* row_shr:15 */                                              \
  X(13, 0x121, 0xF, 0xF, 0) /* row_ror:1 */                                               \
  X(14, 0x125, 0xB, 0x7, 0) /* row_ror:5 */                                               \
  X(15, 0x128, 0xF, 0xF, 1) /* row_ror:8 */                                               \
  X(16, 0x12C, 0xF, 0x3, 0) /* row_ror:12 */                                              \
  X(17, 0x12F, 0xD, 0xF, 0) /* row_ror:15 */                                              \
  X(18, 0x140, 0xF, 0xF, 0) /* row_mirror */                                              \
  X(19, 0x140, 0xA, 0x9, 1) /* row_mirror */                                              \
  X(20, 0x141, 0xF, 0xF, 0) /* row_half_mirror */                                         \
  X(21, 0x141, 0x3, 0x6, 0) /* row_half_mirror */                                         \
  X(22, 0x142, 0xA, 0xF, 0) /* row_bcast:15 into rows 1 and 3 */                          \
  X(23, 0x143, 0xC, 0xF, 0) /* row_bcast:31 into rows 2 and 3 */                          \
  X(24, 0x138, 0xF, 0xF, 0) /* wave_shr:1 */                                              \
  X(25, 0x138, 0xF, 0xF, 1) /* wave_shr:1 */                                              \
  X(26, 0x130, 0xF, 0xF, 1) /* wave_shl:1 */                                              \
  X(27, 0x13C, 0xF, 0xF, 0) /* wave_ror:1 */                                              \
  X(28, 0x134, 0x7, 0xD, 0) /* wave_rol:1 */
//   SWIZZLE(index, offset): bit 15 set: quad-perm mode, else and | or << 5 | xor << 10
#define GM_LANESCAN_SWIZZLE_MENU(X)                                                       \
  X(29, 0x8039) /* quad perm [1,2,3,0] */                                                 \
  X(30, 0x8093) /* quad perm [3,0,1,2] */                                                 \
  X(31, 0x401F) /* swap 16 */                                                             \
  X(32, 0x7C1F) /* reverse 32 */                                                          \
  X(33, 0x0078) /* and 0x18, or 3: lane 3 of each group of 8 */
enum {
  GM_LANESCAN_MV_DPP = 0,
  GM_LANESCAN_MV_SWIZZLE = 1,
  GM_LANESCAN_MV_BPERMUTE = 34,      // from lane (l * (g | 1) + (g >> 8)) & 63
  GM_LANESCAN_MV_BPERMUTE_MANY = 35, // from lane ((l & (g >> 14)) + (g >> 20)) & 63: many to one
  GM_LANESCAN_MV_PERMUTE = 36,       // to lane (l * (g | 1) + (g >> 8)) & 63: a bijection
  GM_LANESCAN_MV_READLANE = 37,      // every lane: src of lane g & 63
  GM_LANESCAN_MV_READFIRSTLANE = 38, // every lane: src of lane 0 (all lanes are active)
  GM_LANESCAN_MV_WRITELANE = 39,     // old, but lane 21 (g & 3) gets src of lane (g >> 8) & 63
  GM_LANESCAN_MV_PERMLANE16_SWAP = 40,  // (old, src) swapped: new old + rotl(new src, 13)
  GM_LANESCAN_MV_PERMLANE32_SWAP = 41,
  GM_LANESCAN_MV_BALLOT_MBCNT = 42,  // (old ^ lo(B) ^ hi(B)) + set bits of B below the lane,
                                     // B = ballot of bit g & 31 of src
  GM_LANESCAN_XLANE_MENU = 43,
};

struct gm_lanescan_menu_t {
  uint32_t kind;   // GM_LANESCAN_MV_DPP, _SWIZZLE, or the entry's own GM_LANESCAN_MV_* (>= 34)
  uint32_t imm;    // dpp_ctrl / swizzle offset
  uint32_t row_mask, bank_mask, bound_ctrl;
};

GM_CUSCAN_HD uint32_t gm_lanescan_xlane_init(uint64_t seed, uint32_t t, uint32_t j) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_XLANE, 4 * t + j);
}
GM_CUSCAN_HD uint32_t gm_lanescan_xlane_entry(uint64_t seed, uint32_t s) {
  return (s + gm_cuscan_hash(seed, GM_LANESCAN_H_XLANE_STEP, 0) % GM_LANESCAN_XLANE_MENU) %
         GM_LANESCAN_XLANE_MENU;
}
GM_CUSCAN_HD uint32_t gm_lanescan_xlane_param(uint64_t seed, uint32_t s) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_XLANE_STEP, 1 + s);
}
// The per-lane mix after a movement: a value's position matters, and the lane's own word from
// before the movement stays in (`own`), so that broadcasts and zero fills do not drain the state
// of what distinguishes lanes and waves.
GM_CUSCAN_HD uint32_t gm_lanescan_xlane_mix(uint32_t moved, uint32_t own, uint32_t l, uint32_t s) {
  return (gm_cuscan_rotl32(moved + gm_cuscan_rotl32(own, 16), 9) ^ (l * 0x85EBCA6Bu + s)) * 0x9E3779B1u;
}
GM_CUSCAN_HD uint32_t gm_lanescan_affine_lane(uint32_t l, uint32_t g) {
  return (l * (g | 1u) + (g >> 8)) & 63u;
}
GM_CUSCAN_HD uint32_t gm_lanescan_writelane_lane(uint32_t g) { return 21u * (g & 3u); }
GM_CUSCAN_HD uint32_t gm_lanescan_many_lane(uint32_t l, uint32_t g) {
  return ((l & (g >> 14)) + (g >> 20)) & 63u;
}

// ================================================================================ regfile
#define GM_LANESCAN_REG_BANKS 6
#define GM_LANESCAN_REG_VGPRS 192       /* 6 banks of 32 */
#define GM_LANESCAN_REG_ACCS 192
#define GM_LANESCAN_REGS 384
#define GM_LANESCAN_REG_UNIFORM_STEPS 12
#define GM_LANESCAN_REG_LANE_STEPS 4
GM_CUSCAN_HD uint32_t gm_lanescan_reg_fill(uint64_t seed, uint32_t t, uint32_t r) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_REG, t * GM_LANESCAN_REGS + r);
}
GM_CUSCAN_HD uint32_t gm_lanescan_reg_step(uint64_t seed, uint32_t round, uint32_t k) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_REG_STEP, round * 16 + k);
}

// ================================================================================ salu
#define GM_LANESCAN_SALU_STEPS 16
GM_CUSCAN_HD uint32_t gm_lanescan_salu_table(uint64_t seed, uint32_t i) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_SALU_TABLE, i);
}
// what leaves the scalar unit in step s, into the lane's vector words
GM_CUSCAN_HD void gm_lanescan_salu_fold(uint32_t v[4], uint32_t s, uint32_t l, uint32_t a,
                                        uint32_t b) {
  const uint32_t i = s & 3u, j = (s + 2u) & 3u;
  v[i] = gm_cuscan_rotl32(v[i], 7) + (a ^ (l * 0x01000193u));
  v[j] ^= b + l;
}

// ================================================================================ trans
#define GM_LANESCAN_TRANS_STEPS 8
enum {
  GM_LANESCAN_OP_EXP = 1 << 0,     // v_exp_f32 at integers
  GM_LANESCAN_OP_LOG = 1 << 1,     // v_log_f32 at powers of two
  GM_LANESCAN_OP_RCP = 1 << 2,     // v_rcp_f32 at +-2^n
  GM_LANESCAN_OP_RSQ = 1 << 3,     // v_rsq_f32 at 4^n
  GM_LANESCAN_OP_SQRT = 1 << 4,    // v_sqrt_f32 at m^2, m < 2^12
  GM_LANESCAN_OP_SIN = 1 << 5,     // v_sin_f32 at quarter turns
  GM_LANESCAN_OP_COS = 1 << 6,
  GM_LANESCAN_OP_RCP64 = 1 << 7,   // v_rcp_f64 at +-2^n
  GM_LANESCAN_OP_SQRT64 = 1 << 8,  // v_sqrt_f64 at 4^n
  GM_LANESCAN_OP_RSQ64 = 1 << 9,
  GM_LANESCAN_OP_RCP16 = 1 << 10,  // v_rcp_f16 at 2^n
  GM_LANESCAN_OP_SQRT16 = 1 << 11, // v_sqrt_f16 at 4^n
  GM_LANESCAN_OP_RSQ16 = 1 << 12,
  GM_LANESCAN_OP_ALL = (1 << 13) - 1,
};
// The operations in the chain: one whose hardware result is not exact at these points is taken
// out here. v_sqrt_f64 is: on an MI355X it returns 2^k (1 + 2^-26) at every 4^k tried, within
// its documented accuracy but not the exact value (profiles/lanescan/README.md).
#define GM_LANESCAN_TRANS_OPS (GM_LANESCAN_OP_ALL & ~GM_LANESCAN_OP_SQRT64)

// The operand points of lane t in step s; `carry` is bit 0 of the lane's word 0 so far, which
// makes the chain dependent.
struct gm_lanescan_trans_pt {
  int32_t n;       // [-16, 16]: exp, log, rcp
  uint32_t neg;    // rcp of -2^n
  int32_t k;       // [-8, 7]: rsq and sqrt of 4^k (f64 too), rcp_f16 of 2^k
  int32_t k16;     // [-3, 4]: sqrt_f16 and rsq_f16 of 4^k16
  uint32_t m;      // < 2^12: sqrt of m^2
  int32_t a;       // [-64, 64]: sin and cos of a quarter turns
};
GM_CUSCAN_HD gm_lanescan_trans_pt gm_lanescan_trans_point(uint64_t seed, uint32_t s, uint32_t t,
                                                          uint32_t carry) {
  const uint32_t h = gm_cuscan_hash(seed, GM_LANESCAN_H_TRANS, s * 256 + t);
  gm_lanescan_trans_pt p;
  p.n = (int32_t)(h & 31u) - 16 + (int32_t)carry;
  p.neg = (h >> 5) & 1u;
  p.k = (int32_t)((h >> 6) & 15u) - 8;
  p.k16 = (int32_t)((h >> 6) & 7u) - 3;
  p.m = (h >> 10) & 4095u;
  p.a = (int32_t)((h >> 22) & 127u) - 64 + (int32_t)carry;
  return p;
}
GM_CUSCAN_HD uint32_t gm_lanescan_trans_init(uint64_t seed, uint32_t t, uint32_t i) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_TRANS_INIT, 4 * t + i);
}
// the signature word of a 64-bit pattern (the format scan's, on bits)
GM_CUSCAN_HD uint32_t gm_lanescan_word64(uint64_t u) {
  return (uint32_t)u ^ gm_cuscan_rotl32((uint32_t)(u >> 32), 16);
}

// ================================================================================ f64
#define GM_LANESCAN_F64_STEPS 8
#define GM_LANESCAN_F64_X_BITS 26
// |p| = |x a + b| < 2^26 * 2^15 + 2^23 < 2^42, and S sums one p per step
static_assert((1ull << 26) * (1ull << 15) + (1ull << 23) < (1ull << 42), "f64: |p| < 2^42");
static_assert((uint64_t)GM_LANESCAN_F64_STEPS * GM_LANESCAN_MAX_ITERS * (1ull << 42) < (1ull << 53),
              "f64: the running sum stays an exact fp64 integer");
static_assert((uint64_t)GM_LANESCAN_F64_STEPS * 255 * (1ull << 42) < (1ull << 53) &&
                  (uint64_t)GM_LANESCAN_F64_STEPS * 256 * (1ull << 42) >= (1ull << 53),
              "f64: its own cap is 255");
// p c 2^e with c <= 64, e <= 3 is below 2^51 eighths, plus d < 2^8 eighths
static_assert((1ull << 42) * 64 * 8 + 256 < (1ull << 52), "f64: r is an exact fp64");
struct gm_lanescan_f64_pt {
  int32_t a;     // [-2^15, 2^15)
  int32_t b;     // [-2^23, 2^23)
  int32_t e;     // 0..3: ldexp by e - 3
  int32_t c;     // 1..64
  int32_t d;     // 0..255 eighths
};
GM_CUSCAN_HD gm_lanescan_f64_pt gm_lanescan_f64_point(uint64_t seed, uint32_t s, uint32_t t) {
  const uint32_t h1 = gm_cuscan_hash(seed, GM_LANESCAN_H_F64_STEP, (s * 256 + t) * 2);
  const uint32_t h2 = gm_cuscan_hash(seed, GM_LANESCAN_H_F64_STEP, (s * 256 + t) * 2 + 1);
  gm_lanescan_f64_pt p;
  p.a = (int32_t)(h1 & 0xFFFFu) - 0x8000;
  p.b = (int32_t)(h2 & 0xFFFFFFu) - 0x800000;
  p.e = (int32_t)((h1 >> 16) & 3u);
  p.c = (int32_t)((h1 >> 18) & 63u) + 1;
  p.d = (int32_t)(h2 >> 24);
  return p;
}
GM_CUSCAN_HD uint32_t gm_lanescan_f64_init(uint64_t seed, uint32_t t) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_F64, t) >> (32 - GM_LANESCAN_F64_X_BITS);
}

// ================================================================================ packed
#define GM_LANESCAN_PACKED_STEPS 16
// v_pk_fma_f32 accumulates one product of two signed bytes per step and half
static_assert((uint64_t)GM_LANESCAN_PACKED_STEPS * GM_LANESCAN_MAX_ITERS * 128 * 128 < (1ull << 24),
              "packed: every partial sum is an exact fp32 integer");
static_assert((uint64_t)GM_LANESCAN_PACKED_STEPS * (GM_LANESCAN_MAX_ITERS + 1) * 128 * 128 >=
                  (1ull << 24),
              "packed is the test that sets GM_LANESCAN_MAX_ITERS");
// the dots: 4 byte products, or 2 products of integers of magnitude <= 32, per step
static_assert((uint64_t)GM_LANESCAN_PACKED_STEPS * GM_LANESCAN_MAX_ITERS * 4 * 128 * 128 < (1ull << 31),
              "packed: sdot4 stays inside an int32");
static_assert((uint64_t)GM_LANESCAN_PACKED_STEPS * GM_LANESCAN_MAX_ITERS * 4 * 255 * 255 < (1ull << 32),
              "packed: udot4 stays inside a uint32");
static_assert((uint64_t)GM_LANESCAN_PACKED_STEPS * GM_LANESCAN_MAX_ITERS * 2 * 32 * 32 < (1ull << 24),
              "packed: the f16 and bf16 dots stay exact fp32 integers");
static_assert(32 * 32 + 8 <= 2048 && 32 * 32 + 8 + 32 <= 2048, "packed: f16 integers <= 2048");
GM_CUSCAN_HD uint32_t gm_lanescan_packed_hash(uint64_t seed, uint32_t s, uint32_t t, uint32_t q) {
  return gm_cuscan_hash(seed, GM_LANESCAN_H_PACKED, (s * 256 + t) * 4 + q);
}
// The small integers of a step, from h1: two halves each of A and B in [-32, 31], C in [-8, 7].
GM_CUSCAN_HD int32_t gm_lanescan_packed_small(uint32_t h1, int which) {
  return which < 4 ? (int32_t)((h1 >> (6 * which)) & 63u) - 32
                   : (int32_t)((h1 >> (24 + 4 * (which - 4))) & 15u) - 8;
}

// ------------------------------------------------------------------------------ host only

// ---- number formats from integers, by exponent arithmetic (no libm, no conversion instruction)
inline uint32_t gm_lanescan_f32_pow2(int e, uint32_t neg = 0) {  // +-2^e, normal
  return neg << 31 | (uint32_t)(127 + e) << 23;
}
inline uint64_t gm_lanescan_f64_pow2(int e, uint32_t neg = 0) {
  return (uint64_t)neg << 63 | (uint64_t)(1023 + e) << 52;
}
inline uint32_t gm_lanescan_f16_pow2(int e) { return (uint32_t)(15 + e) << 10; }
// the bits of integer v in a format with `mant` mantissa bits and exponent bias `bias`;
// |v| <= 2^(mant + 1), so nothing rounds
inline uint64_t gm_lanescan_float_of_int(int64_t v, int mant, int bias, int sign_bit) {
  if (v == 0) return 0;
  const uint64_t s = v < 0, m = s ? (uint64_t)-v : (uint64_t)v;
  int top = 63;
  while (!(m >> top)) --top;
  const uint64_t frac = top <= mant ? m << (mant - top) : m >> (top - mant);
  return s << sign_bit | (uint64_t)(bias + top) << mant | (frac & ((1ull << mant) - 1));
}
inline uint32_t gm_lanescan_f32_of_int(int64_t v) {
  return (uint32_t)gm_lanescan_float_of_int(v, 23, 127, 31);
}
inline uint32_t gm_lanescan_f16_of_int(int64_t v) {
  return (uint32_t)gm_lanescan_float_of_int(v, 10, 15, 15);
}
// v * 2^-3 as fp64 bits, |v| < 2^53
inline uint64_t gm_lanescan_f64_of_eighths(int64_t v) {
  if (v == 0) return 0;
  const uint64_t s = v < 0, m = s ? (uint64_t)-v : (uint64_t)v;
  int top = 63;
  while (!(m >> top)) --top;
  return s << 63 | (uint64_t)(1023 + top - 3) << 52 | ((m << (52 - top)) & ((1ull << 52) - 1));
}

// ---- xlane: the menu as a table, and each movement over a wave's 64 lanes
inline const gm_lanescan_menu_t* gm_lanescan_menu() {
  static const gm_lanescan_menu_t menu[GM_LANESCAN_XLANE_MENU] = {
#define GM_LANESCAN_ROW(i, ctrl, rm, bm, bc) {GM_LANESCAN_MV_DPP, ctrl, rm, bm, bc},
      GM_LANESCAN_DPP_MENU(GM_LANESCAN_ROW)
#undef GM_LANESCAN_ROW
#define GM_LANESCAN_ROW(i, off) {GM_LANESCAN_MV_SWIZZLE, off, 0, 0, 0},
      GM_LANESCAN_SWIZZLE_MENU(GM_LANESCAN_ROW)
#undef GM_LANESCAN_ROW
      {34, 0, 0, 0, 0}, {35, 0, 0, 0, 0}, {36, 0, 0, 0, 0}, {37, 0, 0, 0, 0}, {38, 0, 0, 0, 0},
      {39, 0, 0, 0, 0}, {40, 0, 0, 0, 0}, {41, 0, 0, 0, 0}, {42, 0, 0, 0, 0},
  };
  return menu;
}

// DPP: lane l's source lane under `ctrl`, or -1 where the control points outside the wave or row
inline int gm_lanescan_dpp_source(uint32_t ctrl, int l) {
  const int n = (int)(ctrl & 15u), row = l & ~15, pos = l & 15;
  if (ctrl < 0x100u) return (l & ~3) | (int)((ctrl >> (2 * (l & 3))) & 3u);
  if (ctrl >= 0x101u && ctrl <= 0x10Fu) return pos + n < 16 ? l + n : -1;       // row_shl
  if (ctrl >= 0x111u && ctrl <= 0x11Fu) return pos >= n ? l - n : -1;           // row_shr
  if (ctrl >= 0x121u && ctrl <= 0x12Fu) return row | ((pos - n) & 15);          // row_ror
  switch (ctrl) {
    case 0x130u: return l < 63 ? l + 1 : -1;      // wave_shl:1
    case 0x134u: return (l + 1) & 63;             // wave_rol:1
    case 0x138u: return l > 0 ? l - 1 : -1;       // wave_shr:1
    case 0x13Cu: return (l - 1) & 63;             // wave_ror:1
    case 0x140u: return row | (15 - pos);         // row_mirror
    case 0x141u: return (l & ~7) | (7 - (l & 7)); // row_half_mirror
    case 0x142u: return l >= 16 ? row - 1 : -1;   // row_bcast:15: lane 15 of the row before
    case 0x143u: return l >= 32 ? 31 : -1;        // row_bcast:31: lane 31 into the upper half
    default: return -1;
  }
}
// A lane that row_mask or bank_mask disables keeps `old`; an enabled lane whose source is out
// of range reads 0 with bound_ctrl and keeps `old` without.
inline void gm_lanescan_dpp_host(const gm_lanescan_menu_t& e, const uint32_t old[64],
                                 const uint32_t src[64], uint32_t out[64]) {
  for (int l = 0; l < 64; ++l) {
    const bool enabled = (e.row_mask >> (l >> 4) & 1u) && (e.bank_mask >> ((l >> 2) & 3) & 1u);
    const int from = gm_lanescan_dpp_source(e.imm, l);
    out[l] = !enabled ? old[l] : from >= 0 ? src[from] : e.bound_ctrl ? 0u : old[l];
  }
}
inline void gm_lanescan_swizzle_host(uint32_t off, const uint32_t src[64], uint32_t out[64]) {
  for (int l = 0; l < 64; ++l) {
    if (off & 0x8000u) {
      out[l] = src[(l & ~3) | (int)((off >> (2 * (l & 3))) & 3u)];
    } else {
      const uint32_t j = (((uint32_t)l & 31u & (off & 31u)) | ((off >> 5) & 31u)) ^ ((off >> 10) & 31u);
      out[l] = src[(l & 32) | (int)j];
    }
  }
}
inline void gm_lanescan_move_host(uint32_t entry, uint32_t g, const uint32_t old[64],
                                  const uint32_t src[64], uint32_t out[64]) {
  const gm_lanescan_menu_t& e = gm_lanescan_menu()[entry];
  switch (e.kind) {
    case GM_LANESCAN_MV_DPP: gm_lanescan_dpp_host(e, old, src, out); break;
    case GM_LANESCAN_MV_SWIZZLE: gm_lanescan_swizzle_host(e.imm, src, out); break;
    case GM_LANESCAN_MV_BPERMUTE:
      for (uint32_t l = 0; l < 64; ++l) out[l] = src[gm_lanescan_affine_lane(l, g)];
      break;
    case GM_LANESCAN_MV_BPERMUTE_MANY:
      for (uint32_t l = 0; l < 64; ++l) out[l] = src[gm_lanescan_many_lane(l, g)];
      break;
    case GM_LANESCAN_MV_PERMUTE:
      for (uint32_t l = 0; l < 64; ++l) out[l] = 0;  // a lane nobody writes to reads 0
      for (uint32_t l = 0; l < 64; ++l) out[gm_lanescan_affine_lane(l, g)] = src[l];
      break;
    case GM_LANESCAN_MV_READLANE:
      for (int l = 0; l < 64; ++l) out[l] = src[g & 63u];
      break;
    case GM_LANESCAN_MV_READFIRSTLANE:
      for (int l = 0; l < 64; ++l) out[l] = src[0];
      break;
    case GM_LANESCAN_MV_WRITELANE:
      for (int l = 0; l < 64; ++l) out[l] = old[l];
      out[gm_lanescan_writelane_lane(g)] = src[(g >> 8) & 63u];
      break;
    case GM_LANESCAN_MV_PERMLANE16_SWAP:
    case GM_LANESCAN_MV_PERMLANE32_SWAP: {
      // (vdst, vsrc) = (old, src): the odd rows (upper half) of vdst change places with the even
      // rows (lower half) of vsrc
      const int span = e.kind == GM_LANESCAN_MV_PERMLANE16_SWAP ? 16 : 32;
      uint32_t d[64], s[64];
      for (int l = 0; l < 64; ++l) {
        const bool upper = (l / span) & 1;
        d[l] = upper ? src[l - span] : old[l];
        s[l] = upper ? src[l] : old[l + span];
      }
      for (int l = 0; l < 64; ++l) out[l] = d[l] + gm_cuscan_rotl32(s[l], 13);
      break;
    }
    default: {  // GM_LANESCAN_MV_BALLOT_MBCNT
      uint64_t ballot = 0;
      for (int l = 0; l < 64; ++l) ballot |= (uint64_t)((src[l] >> (g & 31u)) & 1u) << l;
      uint32_t below = 0;
      for (int l = 0; l < 64; ++l) {
        out[l] = (old[l] ^ (uint32_t)ballot ^ (uint32_t)(ballot >> 32)) + below;
        below += (uint32_t)(ballot >> l) & 1u;
      }
    }
  }
}
inline void gm_lanescan_xlane_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  for (uint32_t w = 0; w < 4; ++w) {
    uint32_t x[4][64];
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t j = 0; j < 4; ++j) x[j][l] = gm_lanescan_xlane_init(seed, w * 64 + l, j);
    for (uint32_t s = 0; s < iters * GM_LANESCAN_XLANE_MENU; ++s) {
      const uint32_t j = s & 3u, o = (s + 1u) & 3u;
      uint32_t moved[64];
      gm_lanescan_move_host(gm_lanescan_xlane_entry(seed, s), gm_lanescan_xlane_param(seed, s),
                            x[o], x[j], moved);
      for (uint32_t l = 0; l < 64; ++l) x[j][l] = gm_lanescan_xlane_mix(moved[l], x[j][l], l, s);
    }
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t j = 0; j < 4; ++j) out[(w * 64 + l) * 4 + j] = x[j][l];
  }
}

// ---- regfile: the register file of a lane is an array
inline void gm_lanescan_regfile_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
    const uint32_t l = t & 63u;
    uint32_t reg[GM_LANESCAN_REGS], s[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < GM_LANESCAN_REGS; ++r) reg[r] = gm_lanescan_reg_fill(seed, t, r);
    for (uint32_t round = 0; round < iters; ++round) {
      for (uint32_t k = 0; k < GM_LANESCAN_REG_UNIFORM_STEPS + GM_LANESCAN_REG_LANE_STEPS; ++k) {
        const uint32_t g = gm_lanescan_reg_step(seed, round, k);
        const uint32_t r = k < GM_LANESCAN_REG_UNIFORM_STEPS
                               ? g % GM_LANESCAN_REG_VGPRS
                               : (g % GM_LANESCAN_REG_BANKS) * 32 + (((g >> 8) + l) & 31u);
        s[k & 3] = gm_lanescan_fold(s[k & 3], reg[r]);
        reg[r] = ~reg[r];
      }
      for (uint32_t r = 0; r < GM_LANESCAN_REGS; ++r) {
        s[r & 3] = gm_lanescan_fold(s[r & 3], reg[r]);
        reg[r] = ~reg[r];
      }
    }
    for (uint32_t r = 0; r < GM_LANESCAN_REGS; ++r) s[r & 3] = gm_lanescan_fold(s[r & 3], reg[r]);
    for (int i = 0; i < 4; ++i) out[4 * t + i] = s[i];
  }
}

// ---- salu: the chain in 64-bit arithmetic and bit loops
inline uint32_t gm_lanescan_bit_count(uint32_t v) {
  uint32_t n = 0;
  for (int i = 0; i < 32; ++i) n += (v >> i) & 1u;
  return n;
}
inline uint32_t gm_lanescan_lowest_bit(uint32_t v) {  // 32 for 0
  for (uint32_t i = 0; i < 32; ++i)
    if ((v >> i) & 1u) return i;
  return 32;
}
inline uint32_t gm_lanescan_leading_zeros(uint32_t v) {  // 32 for 0
  for (uint32_t i = 0; i < 32; ++i)
    if ((v >> (31 - i)) & 1u) return i;
  return 32;
}
inline uint32_t gm_lanescan_bit_reverse(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
  return r;
}
inline int64_t gm_lanescan_signed(uint32_t v) { return (int64_t)v - ((v >> 31) ? (1ll << 32) : 0); }
struct gm_lanescan_salu_state {
  uint32_t a, b;
  uint64_t c;
};
inline gm_lanescan_salu_state gm_lanescan_salu_init(uint64_t seed, uint32_t w) {
  gm_lanescan_salu_state q;
  q.a = gm_cuscan_hash(seed, GM_LANESCAN_H_SALU, 4 * w);
  q.b = gm_cuscan_hash(seed, GM_LANESCAN_H_SALU, 4 * w + 1);
  q.c = (uint64_t)gm_cuscan_hash(seed, GM_LANESCAN_H_SALU, 4 * w + 2) << 32 |
        gm_cuscan_hash(seed, GM_LANESCAN_H_SALU, 4 * w + 3);
  return q;
}
inline void gm_lanescan_salu_step_host(gm_lanescan_salu_state& q, uint32_t s,
                                       const uint32_t table[GM_LANESCAN_TABLE_WORDS]) {
  const uint64_t M = 0xFFFFFFFFull;
  uint64_t a = q.a, b = q.b, c = q.c;
  const uint64_t k = table[(a ^ s) & (GM_LANESCAN_TABLE_WORDS - 1)];
  const uint64_t m = a * k;                       // 32 x 32 multiply, low and high
  a ^= m >> 32;
  b = (b + (m & M)) & M;
  c += b << 32 | a;                               // 64-bit add and subtract
  c -= k;
  a ^= (b << (k & 31)) & M;                       // the three kinds of shift
  b ^= a >> ((k >> 5) & 31);
  {
    const int64_t sb = gm_lanescan_signed((uint32_t)b);
    int64_t sh = sb;
    for (uint32_t i = 0; i < ((k >> 10) & 31); ++i) sh = (sh - (sh & 1)) / 2;  // floor
    a = (a + ((uint64_t)sh & M)) & M;
  }
  {
    const uint32_t r = (uint32_t)((k >> 15) & 31) + 1;  // 1..32: 64-bit rotate
    c = c << r | c >> (64 - r);
  }
  const uint32_t off = (uint32_t)(k >> 20) & 15u, wd = ((uint32_t)(k >> 24) & 15u) + 1;
  const uint64_t e = (a >> off) & ((1ull << wd) - 1);              // unsigned field
  uint64_t se = (b >> off) & ((1ull << wd) - 1);                   // signed field
  if (se >> (wd - 1)) se = (se - (1ull << wd)) & M;
  b = (b + gm_lanescan_bit_count((uint32_t)a) + 33 * gm_lanescan_lowest_bit((uint32_t)a) +
       97 * gm_lanescan_leading_zeros((uint32_t)b)) & M;
  a ^= gm_lanescan_bit_reverse((uint32_t)b);
  a = a < b ? (a + e) & M : (a - se) & M;                          // compare and select
  {
    const uint64_t mx = b > k ? b : k;                             // unsigned max
    const int64_t sa = gm_lanescan_signed((uint32_t)a), sk = gm_lanescan_signed((uint32_t)k);
    const int64_t mn = sa < sk ? sa : sk;                          // signed min
    b = (mx - ((uint64_t)mn & M)) & M;
    const int64_t diff = gm_lanescan_signed((uint32_t)a) - gm_lanescan_signed((uint32_t)b);
    a = (a + (uint64_t)(diff < 0 ? -diff : diff)) & M;             // absolute difference
  }
  a ^= c & M;
  b ^= c >> 32;
  q.a = (uint32_t)a;
  q.b = (uint32_t)b;
  q.c = c;
}
inline void gm_lanescan_salu_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  uint32_t table[GM_LANESCAN_TABLE_WORDS];
  for (uint32_t i = 0; i < GM_LANESCAN_TABLE_WORDS; ++i) table[i] = gm_lanescan_salu_table(seed, i);
  for (uint32_t w = 0; w < 4; ++w) {
    uint32_t v[64][4];
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t i = 0; i < 4; ++i)
        v[l][i] = gm_cuscan_hash(seed, GM_LANESCAN_H_SALU_LANE, 4 * (w * 64 + l) + i);
    gm_lanescan_salu_state q = gm_lanescan_salu_init(seed, w);
    for (uint32_t s = 0; s < iters * GM_LANESCAN_SALU_STEPS; ++s) {
      gm_lanescan_salu_step_host(q, s, table);
      for (uint32_t l = 0; l < 64; ++l) gm_lanescan_salu_fold(v[l], s, l, q.a, q.b);
    }
    for (uint32_t l = 0; l < 64; ++l)
      for (uint32_t i = 0; i < 4; ++i) out[(w * 64 + l) * 4 + i] = v[l][i];
  }
}

// ---- trans: every result by exponent arithmetic. A zero result is folded as 0: its sign is
// not part of the test.
inline void gm_lanescan_trans_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS],
                                   uint32_t ops = GM_LANESCAN_TRANS_OPS) {
  static const int kSin[4] = {0, 1, 0, -1};
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
    uint32_t g[4];
    for (uint32_t i = 0; i < 4; ++i) g[i] = gm_lanescan_trans_init(seed, t, i);
    for (uint32_t s = 0; s < iters * GM_LANESCAN_TRANS_STEPS; ++s) {
      const gm_lanescan_trans_pt p = gm_lanescan_trans_point(seed, s, t, g[0] & 1u);
      if (ops & GM_LANESCAN_OP_EXP) g[0] = gm_lanescan_fold(g[0], gm_lanescan_f32_pow2(p.n));
      if (ops & GM_LANESCAN_OP_LOG) g[0] = gm_lanescan_fold(g[0], gm_lanescan_f32_of_int(p.n));
      if (ops & GM_LANESCAN_OP_RCP) g[0] = gm_lanescan_fold(g[0], gm_lanescan_f32_pow2(-p.n, p.neg));
      if (ops & GM_LANESCAN_OP_RSQ) g[0] = gm_lanescan_fold(g[0], gm_lanescan_f32_pow2(-p.k));
      if (ops & GM_LANESCAN_OP_SQRT) g[0] = gm_lanescan_fold(g[0], gm_lanescan_f32_of_int(p.m));
      if (ops & GM_LANESCAN_OP_SIN) g[1] = gm_lanescan_fold(g[1], gm_lanescan_f32_of_int(kSin[p.a & 3]));
      if (ops & GM_LANESCAN_OP_COS)
        g[1] = gm_lanescan_fold(g[1], gm_lanescan_f32_of_int(kSin[(p.a + 1) & 3]));
      if (ops & GM_LANESCAN_OP_RCP64)
        g[2] = gm_lanescan_fold(g[2], gm_lanescan_word64(gm_lanescan_f64_pow2(-p.n, p.neg)));
      if (ops & GM_LANESCAN_OP_SQRT64)
        g[2] = gm_lanescan_fold(g[2], gm_lanescan_word64(gm_lanescan_f64_pow2(p.k)));
      if (ops & GM_LANESCAN_OP_RSQ64)
        g[2] = gm_lanescan_fold(g[2], gm_lanescan_word64(gm_lanescan_f64_pow2(-p.k)));
      if (ops & GM_LANESCAN_OP_RCP16) g[3] = gm_lanescan_fold(g[3], gm_lanescan_f16_pow2(-p.k));
      if (ops & GM_LANESCAN_OP_SQRT16) g[3] = gm_lanescan_fold(g[3], gm_lanescan_f16_pow2(p.k16));
      if (ops & GM_LANESCAN_OP_RSQ16) g[3] = gm_lanescan_fold(g[3], gm_lanescan_f16_pow2(-p.k16));
    }
    for (int i = 0; i < 4; ++i) out[4 * t + i] = g[i];
  }
}

// ---- f64: everything in eighths, in int64_t
inline void gm_lanescan_f64_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
    int64_t x = gm_lanescan_f64_init(seed, t), sum = 0;
    uint32_t g[4] = {0, 0, 0, 0};
    for (uint32_t s = 0; s < iters * GM_LANESCAN_F64_STEPS; ++s) {
      const gm_lanescan_f64_pt q = gm_lanescan_f64_point(seed, s, t);
      const int64_t p = x * q.a + q.b;                            // v_fma_f64
      sum += p;                                                   // v_add_f64
      const int64_t r8 = p * q.c * (1ll << q.e) + q.d;            // ldexp, v_mul_f64, v_add_f64
      const int64_t fl = (r8 - (r8 & 7)) / 8;                     // v_floor_f64
      x = fl & ((1ll << GM_LANESCAN_F64_X_BITS) - 1);             // floor, ldexp, v_fma_f64
      const int64_t trunc = p / 4096;                             // v_cvt_i32_f64 rounds to zero
      g[0] = gm_lanescan_fold(g[0], gm_lanescan_word64(gm_lanescan_f64_of_eighths(p * 8)));
      g[1] = gm_lanescan_fold(g[1], gm_lanescan_word64(gm_lanescan_f64_of_eighths(r8)));
      g[2] = gm_lanescan_fold(g[2], ((uint32_t)x ^ (uint32_t)(r8 & 7) << 28) + (uint32_t)(int32_t)trunc);
    }
    g[3] = gm_lanescan_word64(gm_lanescan_f64_of_eighths(sum * 8));
    for (int i = 0; i < 4; ++i) out[4 * t + i] = g[i];
  }
}

// ---- packed: integers
inline void gm_lanescan_packed_host(uint64_t seed, uint32_t iters, uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
    int64_t acc[2] = {0, 0}, sdot = 0, fdot = 0, bdot = 0;
    uint64_t udot = 0;
    uint32_t g[4] = {0, 0, 0, 0};
    for (uint32_t s = 0; s < iters * GM_LANESCAN_PACKED_STEPS; ++s) {
      uint32_t h[4];
      for (uint32_t q = 0; q < 4; ++q) h[q] = gm_lanescan_packed_hash(seed, s, t, q);
      for (int i = 0; i < 2; ++i)                                  // v_pk_fma_f32
        acc[i] += (int64_t)(int8_t)(h[0] >> (8 * i)) * (int8_t)(h[0] >> (16 + 8 * i));
      uint32_t fma16 = 0, add16 = 0, mul16 = 0;                    // v_pk_fma/add/mul_f16
      for (int i = 0; i < 2; ++i) {
        const int64_t a = gm_lanescan_packed_small(h[1], i), b = gm_lanescan_packed_small(h[1], 2 + i),
                      c = gm_lanescan_packed_small(h[1], 4 + i);
        fma16 |= gm_lanescan_f16_of_int(a * b + c) << (16 * i);
        add16 |= gm_lanescan_f16_of_int(a * b + c + b) << (16 * i);
        // IEEE: a zero product of a negative factor is -0
        mul16 |= (a * c == 0 && (a < 0 || c < 0) ? 0x8000u : gm_lanescan_f16_of_int(a * c)) << (16 * i);
        fdot += a * b;                                             // v_dot2_f32_f16
        bdot += a * c;                                             // v_dot2_f32_bf16
      }
      g[0] = gm_lanescan_fold(gm_lanescan_fold(gm_lanescan_fold(g[0], fma16), add16), mul16);
      uint32_t mul = 0, add = 0, sub = 0, maxi = 0, minu = 0;      // the packed 16-bit integers
      for (int i = 0; i < 2; ++i) {
        const uint32_t a = (h[2] >> (16 * i)) & 0xFFFFu, b = (h[3] >> (16 * i)) & 0xFFFFu;
        const int32_t sa = (int16_t)a, sb = (int16_t)b;
        mul |= ((a * b) & 0xFFFFu) << (16 * i);
        add |= ((a + b) & 0xFFFFu) << (16 * i);
        sub |= ((a - b) & 0xFFFFu) << (16 * i);
        maxi |= ((uint32_t)(sa > sb ? sa : sb) & 0xFFFFu) << (16 * i);
        minu |= (a < b ? a : b) << (16 * i);
      }
      g[1] = gm_lanescan_fold(g[1], mul);
      g[1] = gm_lanescan_fold(g[1], add);
      g[1] = gm_lanescan_fold(g[1], sub);
      g[1] = gm_lanescan_fold(g[1], maxi);
      g[1] = gm_lanescan_fold(g[1], minu);
      for (int i = 0; i < 4; ++i) {                                // v_dot4_i32_i8, v_dot4_u32_u8
        sdot += (int64_t)(int8_t)(h[2] >> (8 * i)) * (int8_t)(h[3] >> (8 * i));
        udot += (uint64_t)((h[2] >> (8 * i)) & 255u) * ((h[3] >> (8 * i)) & 255u);
      }
    }
    g[2] = gm_lanescan_f32_of_int(acc[0]) + gm_cuscan_rotl32(gm_lanescan_f32_of_int(acc[1]), 11);
    g[3] = (uint32_t)(int32_t)sdot ^ gm_cuscan_rotl32((uint32_t)udot, 8) ^
           gm_lanescan_f32_of_int(fdot) ^ gm_cuscan_rotl32(gm_lanescan_f32_of_int(bdot), 24);
    for (int i = 0; i < 4; ++i) out[4 * t + i] = g[i];
  }
}

// The expected table of a whole block, out[4 t + i], for one test bit and 1 <= iters <=
// GM_LANESCAN_MAX_ITERS (the entry points check both).
inline void gm_lanescan_expected_host(uint32_t test, uint64_t seed, uint32_t iters,
                                      uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  switch (test) {
    case GM_LANESCAN_XLANE: gm_lanescan_xlane_host(seed, iters, out); break;
    case GM_LANESCAN_REGFILE: gm_lanescan_regfile_host(seed, iters, out); break;
    case GM_LANESCAN_SALU: gm_lanescan_salu_host(seed, iters, out); break;
    case GM_LANESCAN_TRANS: gm_lanescan_trans_host(seed, iters, out); break;
    case GM_LANESCAN_F64: gm_lanescan_f64_host(seed, iters, out); break;
    case GM_LANESCAN_PACKED: gm_lanescan_packed_host(seed, iters, out); break;
    default: break;
  }
}
