// gm_ldsscan_ref.h — the LDS scan's value model: test bits, geometry, the address schedules and
// data formulas (one definition for the host and for the gfx950 kernel,
// native/hip/gm_ldsscan.hip) and the host evaluation of a block's expected table, with or without
// a poked word. The formulas are written out in gm_probe.h; this is their only implementation.
//
// What is shared is data: hashes, address schedules, operands, folds. What is under test is not
// here at all: on the device a value passes through the byte enables, the paired and wide
// accesses, the LDS atomic units, the bank crossbar, the transposing read or the global -> LDS
// path; the host keeps the LDS image and the arena in plain arrays and never reads what the
// device wrote.
//
// The rule of the atomic test: no signature word depends on the order in which lanes or waves
// reach a word. A returned old value is folded only where one thread alone touches the word
// (phase a); a contended word is folded after a barrier, as its final value, and every contended
// operation commutes (phases b, c). A compare-and-swap loop runs at most GM_LDSSCAN_CAS_TRIES
// tries: each failed try of a thread is caused by another thread's success, of which there are at
// most 255, so the number of give-ups is folded and is 0.
#pragma once
#include <stdint.h>
#include <string.h>

#include "gm_cuscan_sig.h"

enum {
  GM_LDSSCAN_WIDTH = 1,   // 8/16/64/96-bit and paired accesses, partial overwrites
  GM_LDSSCAN_ATOMIC = 2,  // the LDS atomic units: private, contended, tickets
  GM_LDSSCAN_BANK = 4,    // the bank crossbar at every conflict degree, broadcasts
  GM_LDSSCAN_TR16 = 8,    // ds_read_b64_tr_b16
  GM_LDSSCAN_DMA = 16,    // global_load_lds_dword / _dwordx4
  GM_LDSSCAN_ALL = 31,
};
enum { GM_LDSSCAN_IX_WIDTH, GM_LDSSCAN_IX_ATOMIC, GM_LDSSCAN_IX_BANK, GM_LDSSCAN_IX_TR16,
       GM_LDSSCAN_IX_DMA };

#define GM_LDSSCAN_TESTS 5
/* measured on an MI355X (profiles/ldsscan/README.md): a round of all five tests takes 0.52 ms at
   2, 0.29 ms at 1 and 14.5 ms at 63; at 4 (0.98 ms) it would exceed the slowest other scan's
   default round (the CU scan's, 0.62 ms) */
#define GM_LDSSCAN_DEFAULT_ITERS 2
#define GM_LDSSCAN_MAX_ITERS 63
/* hash test ids: disjoint from the earlier scans' (1..0x4ff) */
#define GM_LDSSCAN_H_WIDTH 0x500u
#define GM_LDSSCAN_H_ATOMIC_INIT 0x510u
#define GM_LDSSCAN_H_ATOMIC_OP 0x511u
#define GM_LDSSCAN_H_BANK 0x520u
#define GM_LDSSCAN_H_TR16 0x530u
#define GM_LDSSCAN_H_DMA 0x540u

#define GM_LDSSCAN_WORDS GM_CUSCAN_LDS_WORDS /* 40960 */
#define GM_LDSSCAN_BYTES (4 * GM_LDSSCAN_WORDS)
#define GM_LDSSCAN_ARENA_BYTES GM_LDSSCAN_BYTES
#define GM_LDSSCAN_ARENA_WORDS GM_LDSSCAN_WORDS

GM_CUSCAN_HD uint32_t gm_ldsscan_fold(uint32_t s, uint32_t v) {
  return gm_cuscan_rotl32(s, 5) + v;
}
// word a of the image of pass `pass` (0..7) of round r (0..62) of test `id`
GM_CUSCAN_HD uint32_t gm_ldsscan_pattern(uint64_t seed, uint32_t id, uint32_t r, uint32_t pass,
                                         uint32_t a) {
  return gm_cuscan_hash(seed, id, (r * 8u + pass) * 65536u + a);
}
// An odd stride that 5 does not divide is coprime to every range here (2^k * 5): j -> each cell
// of [0, n) once. j * stride stays below 2^32.
GM_CUSCAN_HD uint32_t gm_ldsscan_perm(uint32_t j, uint32_t n, uint32_t stride, uint32_t off) {
  return (j * stride + off) % n;
}
// index j of thread t in step i of a pass: `turn` quarter turns on, so that a pass reads what
// another wave wrote
GM_CUSCAN_HD uint32_t gm_ldsscan_j(uint32_t t, uint32_t i, uint32_t turn) {
  return i * 256u + ((t + 64u * turn) & 255u);
}

// ================================================================================ width
// The cell (byte, halfword, word, 8-byte cell, 16-byte slot or pair) thread t touches in step i.
GM_CUSCAN_HD uint32_t gm_ldsscan_w_fill8(uint32_t t, uint32_t i) {  // word, 160 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 0), GM_LDSSCAN_WORDS, 12347u, 7u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read16(uint32_t t, uint32_t i) {  // halfword, 320 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 1), GM_LDSSCAN_WORDS * 2u, 20483u, 5u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read32(uint32_t t, uint32_t i) {  // word, 160 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 2), GM_LDSSCAN_WORDS, 6151u, 3u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_fill16(uint32_t t, uint32_t i) {  // word, 160 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 0), GM_LDSSCAN_WORDS, 4099u, 11u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read8(uint32_t t, uint32_t i) {  // byte, 640 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 1), GM_LDSSCAN_BYTES, 16411u, 1u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read64(uint32_t t, uint32_t i) {  // 8-byte cell, 80 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 3), GM_LDSSCAN_WORDS / 2u, 8209u, 9u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_fill64(uint32_t t, uint32_t i) {  // 8-byte cell, 80 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 0), GM_LDSSCAN_WORDS / 2u, 6163u, 13u);
}
// pair q of 20480 -> its first word x; the pair is (x, x + 32): ds_read2_b32 offset1:32
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read2(uint32_t t, uint32_t i) {  // 80 steps
  const uint32_t q = gm_ldsscan_perm(gm_ldsscan_j(t, i, 1), GM_LDSSCAN_WORDS / 2u, 3079u, 17u);
  return 64u * (q >> 5) + (q & 31u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_fill96(uint32_t t, uint32_t i) {  // 16-byte slot, 40 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 0), GM_LDSSCAN_WORDS / 4u, 3083u, 19u);
}
// pair q of 5120 -> word 3 of its first slot; the pair is (x, x + 32), slots s and s + 8:
// ds_write2_b32 offset1:32
GM_CUSCAN_HD uint32_t gm_ldsscan_w_write2(uint32_t t, uint32_t i) {  // 20 steps
  const uint32_t q = gm_ldsscan_perm(gm_ldsscan_j(t, i, 2), GM_LDSSCAN_WORDS / 8u, 1543u, 23u);
  return 4u * (16u * (q >> 3) + (q & 7u)) + 3u;
}
// pair q of 20480 -> its first word x; the pair is (x, x + 64): ds_read2st64_b32 offset1:1
GM_CUSCAN_HD uint32_t gm_ldsscan_w_read2st64(uint32_t t, uint32_t i) {  // 80 steps
  const uint32_t q = gm_ldsscan_perm(gm_ldsscan_j(t, i, 3), GM_LDSSCAN_WORDS / 2u, 12301u, 29u);
  return 128u * (q >> 6) + (q & 63u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_partial(uint32_t t, uint32_t i) {  // word, 160 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 0), GM_LDSSCAN_WORDS, 10243u, 31u);
}
GM_CUSCAN_HD uint32_t gm_ldsscan_w_reread(uint32_t t, uint32_t i) {  // word, 160 steps
  return gm_ldsscan_perm(gm_ldsscan_j(t, i, 1), GM_LDSSCAN_WORDS, 14341u, 37u);
}
// The partial overwrite of a word with v = pattern(pass 4): byte v[7:0] to byte (v >> 8) & 3,
// then halfword v[31:16] to halfword (v >> 10) & 1.
GM_CUSCAN_HD uint32_t gm_ldsscan_w_partial_byte(uint32_t v) { return (v >> 8) & 3u; }
GM_CUSCAN_HD uint32_t gm_ldsscan_w_partial_half(uint32_t v) { return (v >> 10) & 1u; }

// ================================================================================ atomic
// The table, in words. Private: kind k of thread t at P32 + 256 k + t (13 kinds), P64 + 2 (256 k
// + t) (4 kinds), PF + t. Contended: group 0 for the block, group 1 + w for wave w.
enum {
  GM_LDSSCAN_A_ADD, GM_LDSSCAN_A_SUB, GM_LDSSCAN_A_INC, GM_LDSSCAN_A_DEC, GM_LDSSCAN_A_SMIN,
  GM_LDSSCAN_A_SMAX, GM_LDSSCAN_A_UMIN, GM_LDSSCAN_A_UMAX, GM_LDSSCAN_A_AND, GM_LDSSCAN_A_OR,
  GM_LDSSCAN_A_XOR, GM_LDSSCAN_A_XCHG, GM_LDSSCAN_A_CAS, GM_LDSSCAN_A_KINDS32,  // 13
};
enum { GM_LDSSCAN_A_ADD64, GM_LDSSCAN_A_MIN64, GM_LDSSCAN_A_MAX64, GM_LDSSCAN_A_CAS64,
       GM_LDSSCAN_A_KINDS64 };  // min signed, max unsigned
#define GM_LDSSCAN_A_STEPS 2      /* private operations per kind and unit of iters */
#define GM_LDSSCAN_A_P32 0u
#define GM_LDSSCAN_A_P64 (GM_LDSSCAN_A_P32 + 256u * GM_LDSSCAN_A_KINDS32)        /* 3328 */
#define GM_LDSSCAN_A_PF (GM_LDSSCAN_A_P64 + 512u * GM_LDSSCAN_A_KINDS64)         /* 5376 */
#define GM_LDSSCAN_A_GROUPS (GM_LDSSCAN_A_PF + 256u)                             /* 5632 */
// one contended group, in words from its (8-byte aligned) base
enum {
  GM_LDSSCAN_G_ADD64 = 0, GM_LDSSCAN_G_MIN64 = 2, GM_LDSSCAN_G_MAX64 = 4, GM_LDSSCAN_G_CAS64 = 6,
  GM_LDSSCAN_G_ADD = 8, GM_LDSSCAN_G_SUB, GM_LDSSCAN_G_SMIN, GM_LDSSCAN_G_SMAX, GM_LDSSCAN_G_UMIN,
  GM_LDSSCAN_G_UMAX, GM_LDSSCAN_G_AND, GM_LDSSCAN_G_OR, GM_LDSSCAN_G_XOR, GM_LDSSCAN_G_CAS,
  GM_LDSSCAN_G_FADD, GM_LDSSCAN_G_USED,  // 19
  GM_LDSSCAN_G_WORDS = 24,
};
#define GM_LDSSCAN_A_TICKET (GM_LDSSCAN_A_GROUPS + 5u * GM_LDSSCAN_G_WORDS)      /* 5752 */
#define GM_LDSSCAN_A_BITMAP (GM_LDSSCAN_A_TICKET + 8u)                           /* 5760 */
#define GM_LDSSCAN_A_TICKETS 4    /* per thread and unit of iters */
#define GM_LDSSCAN_A_BITMAP_WORDS (256u * GM_LDSSCAN_A_TICKETS / 32u)            /* 32 */
#define GM_LDSSCAN_A_TABLE_WORDS (GM_LDSSCAN_A_BITMAP + GM_LDSSCAN_A_BITMAP_WORDS) /* 5792 */
#define GM_LDSSCAN_CAS_TRIES 256
// operand slots: a private 32-bit kind k has slot k; the others start at
#define GM_LDSSCAN_A_SLOT_P64 16u  /* + 2 kind, + 1 for the high half */
#define GM_LDSSCAN_A_SLOT_PF 24u
#define GM_LDSSCAN_A_SLOT_BLOCK 32u /* + word of the group */
#define GM_LDSSCAN_A_SLOT_WAVE 64u
static_assert(GM_LDSSCAN_A_TABLE_WORDS <= GM_LDSSCAN_WORDS && GM_LDSSCAN_A_P64 % 2 == 0 &&
                  GM_LDSSCAN_A_GROUPS % 2 == 0 && GM_LDSSCAN_G_WORDS % 2 == 0,
              "the table fits and its 64-bit words are aligned");

GM_CUSCAN_HD uint32_t gm_ldsscan_a_init(uint64_t seed, uint32_t r, uint32_t word) {
  return gm_cuscan_hash(seed, GM_LDSSCAN_H_ATOMIC_INIT, r * 8192u + word);
}
// the operand of thread t in step s (0..3) of operand slot `slot` (0..127) of round r
GM_CUSCAN_HD uint32_t gm_ldsscan_a_op(uint64_t seed, uint32_t r, uint32_t slot, uint32_t s,
                                      uint32_t t) {
  return gm_cuscan_hash(seed, GM_LDSSCAN_H_ATOMIC_OP, ((r * 128u + slot) * 4u + s) * 256u + t);
}
GM_CUSCAN_HD uint64_t gm_ldsscan_a_op64(uint64_t seed, uint32_t r, uint32_t slot, uint32_t s,
                                        uint32_t t) {
  return (uint64_t)gm_ldsscan_a_op(seed, r, slot + 1u, s, t) << 32 |
         gm_ldsscan_a_op(seed, r, slot, s, t);
}
// f32 values are small integers: a word starts below 1024 and takes addends below 16, so every
// sum stays below 2^24 and is exact in any order
GM_CUSCAN_HD float gm_ldsscan_a_finit(uint32_t h) { return (float)(h & 1023u); }
GM_CUSCAN_HD float gm_ldsscan_a_fop(uint32_t h) { return (float)(h & 15u); }
// the initial value of table word `word` in round r: a float where f32 is added, 0 for tickets
GM_CUSCAN_HD uint32_t gm_ldsscan_a_init_word(uint64_t seed, uint32_t r, uint32_t word) {
  const uint32_t h = gm_ldsscan_a_init(seed, r, word);
  if (word >= GM_LDSSCAN_A_TICKET) return 0;
  if (word >= GM_LDSSCAN_A_GROUPS) {
    const uint32_t g = (word - GM_LDSSCAN_A_GROUPS) % GM_LDSSCAN_G_WORDS;
    return g == GM_LDSSCAN_G_FADD ? gm_cuscan_f32_bits(gm_ldsscan_a_finit(h)) : h;
  }
  if (word >= GM_LDSSCAN_A_PF) return gm_cuscan_f32_bits(gm_ldsscan_a_finit(h));
  return h;
}
// what the wrapping increment and decrement leave (ds_inc_u32, ds_dec_u32)
GM_CUSCAN_HD uint32_t gm_ldsscan_a_inc(uint32_t old, uint32_t src) {
  return old >= src ? 0u : old + 1u;
}
GM_CUSCAN_HD uint32_t gm_ldsscan_a_dec(uint32_t old, uint32_t src) {
  return (old == 0u || old > src) ? src : old - 1u;
}
// the bound of inc and dec from an operand: small, so that the wrap happens
GM_CUSCAN_HD uint32_t gm_ldsscan_a_bound(uint32_t h) { return (h & 7u) + 1u; }
// The new value of a private 32-bit word after kind k with operand h; `cmp` is compare-and-swap's
// comparand: the word's initial value in step 0 (it swaps), ~h of step 0 in step 1 (it does not).
GM_CUSCAN_HD uint32_t gm_ldsscan_a_apply32(uint32_t k, uint32_t old, uint32_t h, uint32_t cmp) {
  switch (k) {
    case GM_LDSSCAN_A_ADD: return old + h;
    case GM_LDSSCAN_A_SUB: return old - h;
    case GM_LDSSCAN_A_INC: return gm_ldsscan_a_inc(old, gm_ldsscan_a_bound(h));
    case GM_LDSSCAN_A_DEC: return gm_ldsscan_a_dec(old, gm_ldsscan_a_bound(h));
    case GM_LDSSCAN_A_SMIN: return (int32_t)h < (int32_t)old ? h : old;
    case GM_LDSSCAN_A_SMAX: return (int32_t)h > (int32_t)old ? h : old;
    case GM_LDSSCAN_A_UMIN: return h < old ? h : old;
    case GM_LDSSCAN_A_UMAX: return h > old ? h : old;
    case GM_LDSSCAN_A_AND: return old & (h | gm_cuscan_rotl32(h, 11));
    case GM_LDSSCAN_A_OR: return old | (h & gm_cuscan_rotl32(h, 11));
    case GM_LDSSCAN_A_XOR: return old ^ h;
    case GM_LDSSCAN_A_XCHG: return h;
    default: return old == cmp ? h : old;  // GM_LDSSCAN_A_CAS
  }
}
GM_CUSCAN_HD uint64_t gm_ldsscan_a_apply64(uint32_t k, uint64_t old, uint64_t h, uint64_t cmp) {
  switch (k) {
    case GM_LDSSCAN_A_ADD64: return old + h;
    case GM_LDSSCAN_A_MIN64: return (int64_t)h < (int64_t)old ? h : old;
    case GM_LDSSCAN_A_MAX64: return h > old ? h : old;
    default: return old == cmp ? h : old;  // GM_LDSSCAN_A_CAS64
  }
}
// what `and` and `or` take of an operand: about three quarters and one quarter of the bits set
GM_CUSCAN_HD uint32_t gm_ldsscan_a_and_op(uint32_t h) { return h | gm_cuscan_rotl32(h, 11); }
GM_CUSCAN_HD uint32_t gm_ldsscan_a_or_op(uint32_t h) { return h & gm_cuscan_rotl32(h, 11); }

// ================================================================================ bank
// A pass is 640 wave-instructions g of 32-bit accesses, or 320 of 64-bit ones. The LDS is ten
// chunks of 4096 words (2048 8-byte elements); chunk u of round r is walked at stride 2^k, and
// lane l of instruction m of the chunk takes index n = 64 m + ((l + m) & 63) of it:
// position (n mod C/2^k) 2^k + n / (C/2^k), each cell of the chunk once. The 64 lanes of an
// instruction are 2^k apart, the rotation by m moves every lane over every bank.
#define GM_LDSSCAN_B_CHUNK 4096u
#define GM_LDSSCAN_B_STRIDES32 7u /* 1 .. 64 words */
#define GM_LDSSCAN_B_STRIDES64 6u /* 1 .. 32 elements = 2 .. 64 words */
#define GM_LDSSCAN_B_BCAST_STEPS 8u
GM_CUSCAN_HD uint32_t gm_ldsscan_b_word32(uint32_t g, uint32_t l, uint32_t r, uint32_t shift) {
  const uint32_t u = g >> 6, m = g & 63u, k = (u + r + shift) % GM_LDSSCAN_B_STRIDES32;
  const uint32_t n = 64u * m + ((l + m) & 63u), per = GM_LDSSCAN_B_CHUNK >> k;
  return u * GM_LDSSCAN_B_CHUNK + ((n & (per - 1u)) << k) + (n >> (12u - k));  // < 40960
}
GM_CUSCAN_HD uint32_t gm_ldsscan_b_elem64(uint32_t g, uint32_t l, uint32_t r) {
  const uint32_t u = g >> 5, m = g & 31u, k = (u + r) % GM_LDSSCAN_B_STRIDES64;
  const uint32_t n = 64u * m + ((l + m) & 63u), per = (GM_LDSSCAN_B_CHUNK / 2u) >> k;
  return u * (GM_LDSSCAN_B_CHUNK / 2u) + ((n & (per - 1u)) << k) + (n >> (11u - k));  // < 20480
}
// the wave-instruction of wave w in step i: `turn` waves on
GM_CUSCAN_HD uint32_t gm_ldsscan_b_g(uint32_t w, uint32_t i, uint32_t turn) {
  return 4u * i + ((w + turn) & 3u);
}
// broadcasts, instruction g (0..31) of round r: all 64 lanes at one word, each half at one,
// lanes l and l + 16 at one
GM_CUSCAN_HD uint32_t gm_ldsscan_b_all(uint32_t g, uint32_t r) {
  return ((g + 32u * r) * 1237u + 5u) % GM_LDSSCAN_WORDS;
}
GM_CUSCAN_HD uint32_t gm_ldsscan_b_half(uint32_t g, uint32_t l, uint32_t r) {
  return (((g + 32u * r) * 2u + (l >> 5)) * 3571u + 9u) % GM_LDSSCAN_WORDS;
}
GM_CUSCAN_HD uint32_t gm_ldsscan_b_pair(uint32_t g, uint32_t l, uint32_t r) {
  return (((g + 32u * r) * 32u + (l & 15u) + 16u * (l >> 5)) * 12347u + 13u) % GM_LDSSCAN_WORDS;
}

// ================================================================================ tr16
// Stride index k: a 4 x 16 block of 16-bit elements has its row q at origin + q * stride bytes.
// Group G = t >> 4 reads block n = 16 i + G in step i; its origin is unit(k) ((n 4099 + ...) mod
// origins(k)) bytes, origins(k) the number of such origins at which the block fits. At stride 32 a
// block is 128 contiguous bytes and the unit is 128: the 1280 blocks tile the LDS, every cell
// once. At the other strides the unit is 8, the alignment the read needs.
#define GM_LDSSCAN_T_STEPS 80u
GM_CUSCAN_HD uint32_t gm_ldsscan_t_stride(uint32_t k) { return k == 0 ? 32u : k == 1 ? 72u : 264u; }
GM_CUSCAN_HD uint32_t gm_ldsscan_t_unit(uint32_t k) { return k == 0 ? 128u : 8u; }
GM_CUSCAN_HD uint32_t gm_ldsscan_t_origins(uint32_t k) {
  return (GM_LDSSCAN_BYTES - 3u * gm_ldsscan_t_stride(k) - 32u) / gm_ldsscan_t_unit(k) + 1u;
}
GM_CUSCAN_HD uint32_t gm_ldsscan_t_origin(uint32_t k, uint32_t n, uint32_t r) {
  return gm_ldsscan_t_unit(k) * ((n * 4099u + 17u * k + 131u * r) % gm_ldsscan_t_origins(k));
}
// the byte address lane j (0..15) of the group supplies: row j >> 2, columns 4 (j & 3) ...
GM_CUSCAN_HD uint32_t gm_ldsscan_t_addr(uint32_t k, uint32_t n, uint32_t r, uint32_t j) {
  return gm_ldsscan_t_origin(k, n, r) + (j >> 2) * gm_ldsscan_t_stride(k) + 8u * (j & 3u);
}

// ================================================================================ dma
// 160 chunks of 1 KiB; wave w moves chunk c = 4 i + w in step i to chunk d(c, r) of the LDS, as
// one 16-byte instruction where c + r is even and as four 4-byte ones (sub-chunk j to sub-chunk
// (j + 1) & 3) where it is odd. Lane l's source is the slot (l + rho) & 63 of the (sub-)chunk.
#define GM_LDSSCAN_D_CHUNKS 160u
GM_CUSCAN_HD uint32_t gm_ldsscan_d_dest(uint32_t c, uint32_t r) {
  return (c * 37u + r * 11u + 3u) % GM_LDSSCAN_D_CHUNKS;
}
GM_CUSCAN_HD uint32_t gm_ldsscan_d_wide(uint32_t c, uint32_t r) { return ((c + r) & 1u) == 0; }
GM_CUSCAN_HD uint32_t gm_ldsscan_d_rho(uint32_t c, uint32_t r) { return (c * 7u + r) & 63u; }
// the instruction's view. Source byte offset in the arena of lane l: c < 160, slot < 64, so
// wide: at most 159 * 1024 + 63 * 16 + 16 = 163840 = the arena; narrow (j < 4): at most
// 159 * 1024 + 3 * 256 + 63 * 4 + 4 = 163840.
GM_CUSCAN_HD uint32_t gm_ldsscan_d_src_byte(uint32_t c, uint32_t r, uint32_t l, uint32_t j) {
  const uint32_t slot = (l + gm_ldsscan_d_rho(c, r)) & 63u;
  return gm_ldsscan_d_wide(c, r) ? c * 1024u + slot * 16u : c * 1024u + j * 256u + slot * 4u;
}
// LDS byte offset of the wave's base (lane l lands at base + l * size)
GM_CUSCAN_HD uint32_t gm_ldsscan_d_dst_byte(uint32_t c, uint32_t r, uint32_t j) {
  const uint32_t d = gm_ldsscan_d_dest(c, r);
  return gm_ldsscan_d_wide(c, r) ? d * 1024u : d * 1024u + ((j + 1u) & 3u) * 256u;
}
// the reader's view: item y = 64 j + l (0..255) of chunk c -> the LDS word it reads and the
// arena word that must be there
GM_CUSCAN_HD void gm_ldsscan_d_item(uint32_t c, uint32_t r, uint32_t y, uint32_t& lds_word,
                                    uint32_t& arena_word) {
  const uint32_t d = gm_ldsscan_d_dest(c, r), rho = gm_ldsscan_d_rho(c, r);
  if (gm_ldsscan_d_wide(c, r)) {
    lds_word = d * 256u + y;
    arena_word = c * 256u + 4u * (((y >> 2) + rho) & 63u) + (y & 3u);
  } else {
    const uint32_t j = y >> 6, l = y & 63u;
    lds_word = d * 256u + ((j + 1u) & 3u) * 64u + l;
    arena_word = c * 256u + j * 64u + ((l + rho) & 63u);
  }
}
GM_CUSCAN_HD uint32_t gm_ldsscan_d_arena(uint64_t seed, uint32_t a) {
  return gm_ldsscan_pattern(seed, GM_LDSSCAN_H_DMA, 0, 0, a);
}
GM_CUSCAN_HD void gm_ldsscan_d_fold(uint32_t s[4], uint32_t got, uint32_t want) {
  s[0] = gm_ldsscan_fold(s[0], got);
  s[1] = gm_cuscan_rotl32(s[1], 7) ^ got;
  s[2] += got;
  s[3] += got != want;
}

// ================================================================================ the host's LDS
// A plain byte array, little endian as the device's.
struct gm_ldsscan_image {
  uint8_t b[GM_LDSSCAN_BYTES];
  uint32_t r8(uint32_t a) const { return b[a]; }
  uint32_t r16(uint32_t h) const { return b[2 * h] | (uint32_t)b[2 * h + 1] << 8; }
  uint32_t r32(uint32_t w) const { return r16(2 * w) | r16(2 * w + 1) << 16; }
  void w8(uint32_t a, uint32_t v) { b[a] = (uint8_t)v; }
  void w16(uint32_t h, uint32_t v) { w8(2 * h, v), w8(2 * h + 1, v >> 8); }
  void w32(uint32_t w, uint32_t v) { w16(2 * w, v), w16(2 * w + 1, v >> 16); }
};

inline void gm_ldsscan_expected_width(uint64_t seed, uint32_t iters, uint32_t poke_offset,
                                      uint32_t poke_mask, gm_ldsscan_image& m, uint32_t* out) {
  const uint32_t T = GM_CUSCAN_THREADS, W = GM_LDSSCAN_WORDS, H = GM_LDSSCAN_H_WIDTH;
  for (uint32_t r = 0; r < iters; ++r) {
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / T; ++i) {
        const uint32_t a = gm_ldsscan_w_fill8(t, i), v = gm_ldsscan_pattern(seed, H, r, 0, a);
        for (uint32_t k = 0; k < 4; ++k) m.w8(4 * a + k, v >> (8 * k));
      }
    if (r == 0) m.w32(poke_offset, m.r32(poke_offset) ^ poke_mask);
    for (uint32_t t = 0; t < T; ++t) {
      uint32_t* s = out + 4 * t;
      for (uint32_t i = 0; i < 2 * W / T; ++i) {
        const uint32_t v = m.r16(gm_ldsscan_w_read16(t, i));
        s[0] = gm_ldsscan_fold(s[0], (i & 1) ? (uint32_t)(int32_t)(int16_t)v : v);
      }
      for (uint32_t i = 0; i < W / T; ++i) s[0] = gm_ldsscan_fold(s[0], m.r32(gm_ldsscan_w_read32(t, i)));
    }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / T; ++i) {
        const uint32_t a = gm_ldsscan_w_fill16(t, i), v = gm_ldsscan_pattern(seed, H, r, 1, a);
        m.w16(2 * a, v), m.w16(2 * a + 1, v >> 16);
      }
    for (uint32_t t = 0; t < T; ++t) {
      uint32_t* s = out + 4 * t;
      for (uint32_t i = 0; i < 4 * W / T; ++i) {
        const uint32_t v = m.r8(gm_ldsscan_w_read8(t, i));
        s[1] = gm_ldsscan_fold(s[1], (i & 1) ? (uint32_t)(int32_t)(int8_t)v : v);
      }
      for (uint32_t i = 0; i < W / 2 / T; ++i) {
        const uint32_t c = gm_ldsscan_w_read64(t, i);
        s[1] = gm_ldsscan_fold(gm_ldsscan_fold(s[1], m.r32(2 * c)), m.r32(2 * c + 1));
      }
    }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / 2 / T; ++i) {
        const uint32_t c = gm_ldsscan_w_fill64(t, i);
        m.w32(2 * c, gm_ldsscan_pattern(seed, H, r, 2, 2 * c));
        m.w32(2 * c + 1, gm_ldsscan_pattern(seed, H, r, 2, 2 * c + 1));
      }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / 2 / T; ++i) {
        const uint32_t x = gm_ldsscan_w_read2(t, i);
        out[4 * t + 2] = gm_ldsscan_fold(gm_ldsscan_fold(out[4 * t + 2], m.r32(x)), m.r32(x + 32));
      }
    for (uint32_t t = 0; t < T; ++t) {
      for (uint32_t i = 0; i < W / 4 / T; ++i) {
        const uint32_t q = gm_ldsscan_w_fill96(t, i);
        for (uint32_t k = 0; k < 3; ++k) m.w32(4 * q + k, gm_ldsscan_pattern(seed, H, r, 3, 4 * q + k));
      }
      for (uint32_t i = 0; i < W / 8 / T; ++i) {
        const uint32_t x = gm_ldsscan_w_write2(t, i);
        m.w32(x, gm_ldsscan_pattern(seed, H, r, 3, x));
        m.w32(x + 32, gm_ldsscan_pattern(seed, H, r, 3, x + 32));
      }
    }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / 2 / T; ++i) {
        const uint32_t x = gm_ldsscan_w_read2st64(t, i);
        out[4 * t + 2] = gm_ldsscan_fold(gm_ldsscan_fold(out[4 * t + 2], m.r32(x)), m.r32(x + 64));
      }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / T; ++i) {
        const uint32_t a = gm_ldsscan_w_partial(t, i), v = gm_ldsscan_pattern(seed, H, r, 4, a);
        m.w8(4 * a + gm_ldsscan_w_partial_byte(v), v);
        m.w16(2 * a + gm_ldsscan_w_partial_half(v), v >> 16);
      }
    for (uint32_t t = 0; t < T; ++t)
      for (uint32_t i = 0; i < W / T; ++i)
        out[4 * t + 3] = gm_ldsscan_fold(out[4 * t + 3], m.r32(gm_ldsscan_w_reread(t, i)));
  }
}

// One contended group in sequence: every operation commutes, so the order is the host's choice.
inline void gm_ldsscan_host_group(uint64_t seed, uint32_t r, uint32_t slot0, uint32_t t0,
                                  uint32_t n, uint32_t* g) {
  uint64_t q[4];
  for (int k = 0; k < 4; ++k) q[k] = (uint64_t)g[2 * k + 1] << 32 | g[2 * k];
  float f;
  memcpy(&f, &g[GM_LDSSCAN_G_FADD], 4);
  for (uint32_t t = t0; t < t0 + n; ++t) {
    for (uint32_t k = 0; k < 4; ++k) {
      const uint64_t h = gm_ldsscan_a_op64(seed, r, slot0 + 2 * k, 0, t);
      // the bounded compare-and-swap loop adds
      q[k] = gm_ldsscan_a_apply64(k == GM_LDSSCAN_A_CAS64 ? GM_LDSSCAN_A_ADD64 : k, q[k], h, 0);
    }
    for (uint32_t x = GM_LDSSCAN_G_ADD; x < GM_LDSSCAN_G_USED; ++x) {
      const uint32_t h = gm_ldsscan_a_op(seed, r, slot0 + x, 0, t);
      switch (x) {
        case GM_LDSSCAN_G_ADD: case GM_LDSSCAN_G_CAS: g[x] += h; break;
        case GM_LDSSCAN_G_SUB: g[x] -= h; break;
        case GM_LDSSCAN_G_SMIN: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_SMIN, g[x], h, 0); break;
        case GM_LDSSCAN_G_SMAX: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_SMAX, g[x], h, 0); break;
        case GM_LDSSCAN_G_UMIN: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_UMIN, g[x], h, 0); break;
        case GM_LDSSCAN_G_UMAX: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_UMAX, g[x], h, 0); break;
        case GM_LDSSCAN_G_AND: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_AND, g[x], h, 0); break;
        case GM_LDSSCAN_G_OR: g[x] = gm_ldsscan_a_apply32(GM_LDSSCAN_A_OR, g[x], h, 0); break;
        case GM_LDSSCAN_G_XOR: g[x] ^= h; break;
        default: f += gm_ldsscan_a_fop(h); break;  // GM_LDSSCAN_G_FADD
      }
    }
  }
  for (int k = 0; k < 4; ++k) g[2 * k] = (uint32_t)q[k], g[2 * k + 1] = (uint32_t)(q[k] >> 32);
  memcpy(&g[GM_LDSSCAN_G_FADD], &f, 4);
}

// The table after round r's operations (tab[GM_LDSSCAN_A_TABLE_WORDS]); `olds`, if given, takes
// the fold of the old values the private operations returned, per thread.
inline void gm_ldsscan_host_atomic_round(uint64_t seed, uint32_t r, uint32_t* tab, uint32_t* olds) {
  for (uint32_t a = 0; a < GM_LDSSCAN_A_TABLE_WORDS; ++a) tab[a] = gm_ldsscan_a_init_word(seed, r, a);
  for (uint32_t t = 0; t < GM_CUSCAN_THREADS; ++t) {
    uint32_t o = olds ? olds[t] : 0;
    for (uint32_t k = 0; k < GM_LDSSCAN_A_KINDS32; ++k) {
      uint32_t& w = tab[GM_LDSSCAN_A_P32 + 256 * k + t];
      uint32_t cmp = w;
      for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
        const uint32_t h = gm_ldsscan_a_op(seed, r, k, s, t);
        o = gm_ldsscan_fold(o, w);
        w = gm_ldsscan_a_apply32(k, w, h, cmp);
        cmp = ~h;  // the second try fails
      }
    }
    for (uint32_t k = 0; k < GM_LDSSCAN_A_KINDS64; ++k) {
      uint32_t* p = &tab[GM_LDSSCAN_A_P64 + 2 * (256 * k + t)];
      uint64_t w = (uint64_t)p[1] << 32 | p[0], cmp = w;
      for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
        const uint64_t h = gm_ldsscan_a_op64(seed, r, GM_LDSSCAN_A_SLOT_P64 + 2 * k, s, t);
        o = gm_ldsscan_fold(gm_ldsscan_fold(o, (uint32_t)w), (uint32_t)(w >> 32));
        w = gm_ldsscan_a_apply64(k, w, h, cmp);
        cmp = ~h;
      }
      p[0] = (uint32_t)w, p[1] = (uint32_t)(w >> 32);
    }
    {
      float f;
      memcpy(&f, &tab[GM_LDSSCAN_A_PF + t], 4);
      for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
        o = gm_ldsscan_fold(o, gm_cuscan_f32_bits(f));
        f += gm_ldsscan_a_fop(gm_ldsscan_a_op(seed, r, GM_LDSSCAN_A_SLOT_PF, s, t));
      }
      memcpy(&tab[GM_LDSSCAN_A_PF + t], &f, 4);
    }
    if (olds) olds[t] = o;
  }
  gm_ldsscan_host_group(seed, r, GM_LDSSCAN_A_SLOT_BLOCK, 0, 256, tab + GM_LDSSCAN_A_GROUPS);
  for (uint32_t w = 0; w < 4; ++w)
    gm_ldsscan_host_group(seed, r, GM_LDSSCAN_A_SLOT_WAVE, 64 * w, 64,
                          tab + GM_LDSSCAN_A_GROUPS + (1 + w) * GM_LDSSCAN_G_WORDS);
  // every thread takes GM_LDSSCAN_A_TICKETS tickets and marks each: whatever the order, the
  // counter ends at their number and every bit is set once
  for (uint32_t n = 0; n < 256u * GM_LDSSCAN_A_TICKETS; ++n) {
    const uint32_t ticket = tab[GM_LDSSCAN_A_TICKET]++;
    tab[GM_LDSSCAN_A_BITMAP + (ticket >> 5) % GM_LDSSCAN_A_BITMAP_WORDS] |= 1u << (ticket & 31);
  }
}

// what a thread folds of the table after the barrier: sig[1] its private words, sig[2] the
// block's group, its wave's and its give-ups (0), sig[3] the counter and the bitmap
inline void gm_ldsscan_host_atomic_fold(const uint32_t* tab, uint32_t t, uint32_t* s) {
  for (uint32_t k = 0; k < GM_LDSSCAN_A_KINDS32; ++k)
    s[1] = gm_ldsscan_fold(s[1], tab[GM_LDSSCAN_A_P32 + 256 * k + t]);
  for (uint32_t k = 0; k < 2 * GM_LDSSCAN_A_KINDS64; ++k)
    s[1] = gm_ldsscan_fold(s[1], tab[GM_LDSSCAN_A_P64 + 2 * (256 * (k >> 1) + t) + (k & 1)]);
  s[1] = gm_ldsscan_fold(s[1], tab[GM_LDSSCAN_A_PF + t]);
  for (uint32_t x = 0; x < GM_LDSSCAN_G_USED; ++x)
    s[2] = gm_ldsscan_fold(s[2], tab[GM_LDSSCAN_A_GROUPS + x]);
  for (uint32_t x = 0; x < GM_LDSSCAN_G_USED; ++x)
    s[2] = gm_ldsscan_fold(s[2], tab[GM_LDSSCAN_A_GROUPS + (1 + (t >> 6)) * GM_LDSSCAN_G_WORDS + x]);
  s[2] = gm_ldsscan_fold(s[2], 0);
  s[3] = gm_ldsscan_fold(s[3], tab[GM_LDSSCAN_A_TICKET]);
  for (uint32_t x = 0; x < GM_LDSSCAN_A_BITMAP_WORDS; ++x)
    s[3] = gm_ldsscan_fold(s[3], tab[GM_LDSSCAN_A_BITMAP + x]);
}

// ---- host evaluation of a whole block's table, out[4 t + i]; `test` one GM_LDSSCAN_* bit and
// iters within its bound (the entry points check both). poke_mask != 0: the run in which
// poke_mask was XORed into word poke_offset (< 40960) of the LDS image after the test's first
// fill, or of the arena (dma); the atomic test has no such run.
inline void gm_ldsscan_expected_host(uint32_t test, uint64_t seed, uint32_t iters,
                                     uint32_t poke_offset, uint32_t poke_mask,
                                     uint32_t out[GM_CUSCAN_SIG_WORDS]) {
  const uint32_t T = GM_CUSCAN_THREADS, W = GM_LDSSCAN_WORDS;
  static thread_local gm_ldsscan_image m;
  for (uint32_t i = 0; i < GM_CUSCAN_SIG_WORDS; ++i) out[i] = 0;
  if (test == GM_LDSSCAN_WIDTH) {
    gm_ldsscan_expected_width(seed, iters, poke_offset, poke_mask, m, out);
  } else if (test == GM_LDSSCAN_ATOMIC) {
    static thread_local uint32_t tab[GM_LDSSCAN_A_TABLE_WORDS], olds[GM_CUSCAN_THREADS];
    for (uint32_t t = 0; t < T; ++t) olds[t] = 0;
    for (uint32_t r = 0; r < iters; ++r) {
      gm_ldsscan_host_atomic_round(seed, r, tab, olds);
      for (uint32_t t = 0; t < T; ++t) gm_ldsscan_host_atomic_fold(tab, t, out + 4 * t);
    }
    for (uint32_t t = 0; t < T; ++t) out[4 * t] = olds[t];
  } else if (test == GM_LDSSCAN_BANK) {
    for (uint32_t r = 0; r < iters; ++r) {
      for (uint32_t g = 0; g < W / 64; ++g)
        for (uint32_t l = 0; l < 64; ++l) {
          const uint32_t a = gm_ldsscan_b_word32(g, l, r, 0);
          m.w32(a, gm_ldsscan_pattern(seed, GM_LDSSCAN_H_BANK, r, 0, a));
        }
      if (r == 0) m.w32(poke_offset, m.r32(poke_offset) ^ poke_mask);
      for (uint32_t t = 0; t < T; ++t) {
        uint32_t* s = out + 4 * t;
        const uint32_t w = t >> 6, l = t & 63;
        for (uint32_t i = 0; i < W / T; ++i)
          s[0] = gm_ldsscan_fold(s[0], m.r32(gm_ldsscan_b_word32(gm_ldsscan_b_g(w, i, 1), l, r, 3)));
        for (uint32_t i = 0; i < W / 2 / T; ++i) {
          const uint32_t e = gm_ldsscan_b_elem64(gm_ldsscan_b_g(w, i, 2), l, r);
          s[1] = gm_ldsscan_fold(s[1], m.r32(2 * e));
          s[2] = gm_ldsscan_fold(s[2], m.r32(2 * e + 1));
        }
        for (uint32_t i = 0; i < GM_LDSSCAN_B_BCAST_STEPS; ++i) {
          const uint32_t g = gm_ldsscan_b_g(w, i, 0);
          s[3] = gm_ldsscan_fold(s[3], m.r32(gm_ldsscan_b_all(g, r)));
          s[3] = gm_ldsscan_fold(s[3], m.r32(gm_ldsscan_b_half(g, l, r)));
          s[3] = gm_ldsscan_fold(s[3], m.r32(gm_ldsscan_b_pair(g, l, r)));
        }
      }
    }
  } else if (test == GM_LDSSCAN_TR16) {
    for (uint32_t r = 0; r < iters; ++r) {
      for (uint32_t a = 0; a < W; ++a) m.w32(a, gm_ldsscan_pattern(seed, GM_LDSSCAN_H_TR16, r, 0, a));
      if (r == 0) m.w32(poke_offset, m.r32(poke_offset) ^ poke_mask);
      for (uint32_t t = 0; t < T; ++t) {
        uint32_t* s = out + 4 * t;
        for (uint32_t k = 0; k < 3; ++k)
          for (uint32_t i = 0; i < GM_LDSSCAN_T_STEPS; ++i) {
            // lane i of the group receives column i: row q is what lane 4 q supplied, plus i
            uint32_t e[4];
            for (uint32_t q = 0; q < 4; ++q)
              e[q] = m.r16(gm_ldsscan_t_addr(k, 16 * i + (t >> 4), r, 4 * q) / 2 + (t & 15));
            const uint32_t lo = e[0] | e[1] << 16, hi = e[2] | e[3] << 16;
            s[k] = gm_ldsscan_fold(gm_ldsscan_fold(s[k], lo), hi);
            s[3] = gm_ldsscan_fold(s[3], lo ^ gm_cuscan_rotl32(hi, 13));
          }
      }
    }
  } else if (test == GM_LDSSCAN_DMA) {
    static thread_local uint32_t arena[GM_LDSSCAN_ARENA_WORDS];
    for (uint32_t a = 0; a < GM_LDSSCAN_ARENA_WORDS; ++a) arena[a] = gm_ldsscan_d_arena(seed, a);
    arena[poke_offset] ^= poke_mask;
    for (uint32_t r = 0; r < iters; ++r) {
      // the instructions, by their own view
      for (uint32_t c = 0; c < GM_LDSSCAN_D_CHUNKS; ++c)
        for (uint32_t l = 0; l < 64; ++l) {
          if (gm_ldsscan_d_wide(c, r)) {
            for (uint32_t e = 0; e < 4; ++e)
              m.w32(gm_ldsscan_d_dst_byte(c, r, 0) / 4 + 4 * l + e,
                    arena[gm_ldsscan_d_src_byte(c, r, l, 0) / 4 + e]);
          } else {
            for (uint32_t j = 0; j < 4; ++j)
              m.w32(gm_ldsscan_d_dst_byte(c, r, j) / 4 + l, arena[gm_ldsscan_d_src_byte(c, r, l, j) / 4]);
          }
        }
      for (uint32_t t = 0; t < T; ++t)
        for (uint32_t i = 0; i < GM_LDSSCAN_D_CHUNKS / 4; ++i)
          for (uint32_t j = 0; j < 4; ++j) {
            uint32_t x, a;
            gm_ldsscan_d_item(4 * i + (((t >> 6) + 1) & 3), r, 64 * j + (t & 63), x, a);
            gm_ldsscan_d_fold(out + 4 * t, m.r32(x), gm_ldsscan_d_arena(seed, a));
          }
    }
  }
}
