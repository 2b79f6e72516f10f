// gm_ldsscan.hip — per-CU LDS scan for gfx950: what sits between a lane and the cells of a CU's
// LDS. The CU scan's `lds` march proves that each of the 40960 words holds a value; this scan
// checks the byte enables of sub-dword stores, the 64/96-bit and paired accesses, the LDS atomic
// units, the bank crossbar under conflicts and broadcasts, the transposing read
// (ds_read_b64_tr_b16) and the direct global -> LDS path (global_load_lds_dword / _dwordx4).
//
// One kernel, k_ldsscan, in the CU scan's frame (gm_cuscan_frame.h): a 256-thread block that
// statically declares all 160 KiB of LDS, so at most one block is resident per CU. Five
// known-answer tests of 4 signature words per thread; the schedules and data formulas are
// gm_ldsscan_ref.h (shared with the host, written out in gm_probe.h).
//
// The rule of the atomic test: no signature word depends on the order in which lanes or waves
// reach a word. Returned old values are folded only for words one thread alone touches; contended
// words are folded as final values, read after a barrier.
//
// Every block reads the same 160 KiB arena in device memory (dma) and writes none of it.
//
// Measured on an MI355X (profiles/ldsscan/README.md): a round of all five tests takes 0.52 ms at
// iters 2 (the default), 0.29 ms at 1 and 14.5 ms at 63; 108 registers, no scratch.
#include "gm_ldsscan_ref.h"

#include "gm_cuscan_frame.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void gbl_void;
// volatile, and in the LDS address space by type: each access stays one ds_ access of its width
typedef volatile __attribute__((address_space(3))) uint8_t lds_u8;
typedef volatile __attribute__((address_space(3))) int8_t lds_i8;
typedef volatile __attribute__((address_space(3))) uint16_t lds_u16;
typedef volatile __attribute__((address_space(3))) int16_t lds_i16;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

struct Ctx {
  uint32_t* lds;
  uint64_t seed;
  uint32_t iters;
  gm_ldsscan_poke_t poke;
};

// The barrier after a test's first fill, and the poke of `test` if it is asked for: thread 0
// flips the word before the barrier that precedes the reads.
__device__ __forceinline__ void filled(const Ctx& c, uint32_t test, bool poke_now) {
  __syncthreads();
  if (poke_now && c.poke.mask != 0 && c.poke.test == test) {  // uniform
    if (threadIdx.x == 0) c.lds[c.poke.word_offset] ^= c.poke.mask;  // < 40960: poke_ok
    __syncthreads();
  }
}

// ================================================================================ width
// The sub-dword accesses are volatile: each stays one access of its own width.
__device__ __forceinline__ void test_width(const Ctx& c, uint32_t sig[4]) {
  const uint32_t t = threadIdx.x;
  constexpr uint32_t W = GM_LDSSCAN_WORDS, T = GM_CUSCAN_THREADS, H = GM_LDSSCAN_H_WIDTH;
  uint32_t* lds = c.lds;
  lds_u8* b8 = (lds_u8*)lds;
  lds_u16* b16 = (lds_u16*)lds;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < c.iters; ++r) {
    // 8-bit stores; 16-bit unsigned and signed and 32-bit loads
    for (uint32_t i = 0; i < W / T; ++i) {
      const uint32_t a = gm_ldsscan_w_fill8(t, i), v = gm_ldsscan_pattern(c.seed, H, r, 0, a);
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) b8[4 * a + k] = (uint8_t)(v >> (8 * k));  // a < 40960
    }
    filled(c, GM_LDSSCAN_WIDTH, r == 0);
    for (uint32_t i = 0; i < 2 * W / T; i += 2) {
      const uint32_t u = b16[gm_ldsscan_w_read16(t, i)];  // < 81920
      const int32_t s = ((lds_i16*)b16)[gm_ldsscan_w_read16(t, i + 1)];
      sig[0] = gm_ldsscan_fold(gm_ldsscan_fold(sig[0], u), (uint32_t)s);
    }
    for (uint32_t i = 0; i < W / T; ++i) sig[0] = gm_ldsscan_fold(sig[0], lds[gm_ldsscan_w_read32(t, i)]);
    __syncthreads();
    // 16-bit stores; 8-bit unsigned and signed and 64-bit loads
    for (uint32_t i = 0; i < W / T; ++i) {
      const uint32_t a = gm_ldsscan_w_fill16(t, i), v = gm_ldsscan_pattern(c.seed, H, r, 1, a);
      b16[2 * a] = (uint16_t)v;
      b16[2 * a + 1] = (uint16_t)(v >> 16);
    }
    __syncthreads();
    for (uint32_t i = 0; i < 4 * W / T; i += 2) {
      const uint32_t u = b8[gm_ldsscan_w_read8(t, i)];  // < 163840
      const int32_t s = ((lds_i8*)b8)[gm_ldsscan_w_read8(t, i + 1)];
      sig[1] = gm_ldsscan_fold(gm_ldsscan_fold(sig[1], u), (uint32_t)s);
    }
    for (uint32_t i = 0; i < W / 2 / T; ++i) {
      const u32x2 v = ((const u32x2*)lds)[gm_ldsscan_w_read64(t, i)];  // < 20480
      sig[1] = gm_ldsscan_fold(gm_ldsscan_fold(sig[1], v.x), v.y);
    }
    __syncthreads();
    // 64-bit stores (8-byte aligned); ds_read2_b32
    for (uint32_t i = 0; i < W / 2 / T; ++i) {
      const uint32_t cell = gm_ldsscan_w_fill64(t, i);  // < 20480
      const u32x2 v = {gm_ldsscan_pattern(c.seed, H, r, 2, 2 * cell),
                       gm_ldsscan_pattern(c.seed, H, r, 2, 2 * cell + 1)};
      ((u32x2*)lds)[cell] = v;
    }
    __syncthreads();
    for (uint32_t i = 0; i < W / 2 / T; ++i) {
      const uint32_t x = gm_ldsscan_w_read2(t, i);  // x + 32 < 40960
      const uint32_t v0 = lds[x], v1 = lds[x + 32];
      sig[2] = gm_ldsscan_fold(gm_ldsscan_fold(sig[2], v0), v1);
    }
    __syncthreads();
    // 96-bit stores (16-byte aligned) and ds_write2_b32 for each slot's last word;
    // ds_read2st64_b32
    for (uint32_t i = 0; i < W / 4 / T; ++i) {
      const uint32_t q = gm_ldsscan_w_fill96(t, i);  // < 10240
      const u32x3 v = {gm_ldsscan_pattern(c.seed, H, r, 3, 4 * q),
                       gm_ldsscan_pattern(c.seed, H, r, 3, 4 * q + 1),
                       gm_ldsscan_pattern(c.seed, H, r, 3, 4 * q + 2)};
      *(u32x3*)(lds + 4 * q) = v;
    }
    for (uint32_t i = 0; i < W / 8 / T; ++i) {
      const uint32_t x = gm_ldsscan_w_write2(t, i);  // x + 32 < 40960
      const uint32_t v0 = gm_ldsscan_pattern(c.seed, H, r, 3, x);
      const uint32_t v1 = gm_ldsscan_pattern(c.seed, H, r, 3, x + 32);
      lds[x] = v0;
      lds[x + 32] = v1;
    }
    __syncthreads();
    for (uint32_t i = 0; i < W / 2 / T; ++i) {
      const uint32_t x = gm_ldsscan_w_read2st64(t, i);  // x + 64 < 40960
      const uint32_t v0 = lds[x], v1 = lds[x + 64];
      sig[2] = gm_ldsscan_fold(gm_ldsscan_fold(sig[2], v0), v1);
    }
    __syncthreads();
    // one byte, then one halfword into a filled word; the 32-bit read shows the rest untouched
    for (uint32_t i = 0; i < W / T; ++i) {
      const uint32_t a = gm_ldsscan_w_partial(t, i), v = gm_ldsscan_pattern(c.seed, H, r, 4, a);
      b8[4 * a + gm_ldsscan_w_partial_byte(v)] = (uint8_t)v;
      b16[2 * a + gm_ldsscan_w_partial_half(v)] = (uint16_t)(v >> 16);
    }
    __syncthreads();
    for (uint32_t i = 0; i < W / T; ++i) sig[3] = gm_ldsscan_fold(sig[3], lds[gm_ldsscan_w_reread(t, i)]);
    __syncthreads();
  }
}

// ================================================================================ atomic
#define GM_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define GM_RLX __ATOMIC_RELAXED

// At most GM_LDSSCAN_CAS_TRIES tries to add h by compare-and-swap; 1 if it gave up.
template <class V>
__device__ __forceinline__ uint32_t cas_add(V* p, V h) {
  uint32_t pending = 1;
  for (uint32_t n = 0; n < GM_LDSSCAN_CAS_TRIES; ++n) {
    if (pending) {
      V old = __hip_atomic_load(p, GM_RLX, GM_WG);
      if (__hip_atomic_compare_exchange_strong(p, &old, (V)(old + h), GM_RLX, GM_RLX, GM_WG))
        pending = 0;
    }
    if (!__any(pending)) break;
  }
  return pending;
}

// One contended group: `n`-th thread of those that share it. Only commutative operations, and
// no return is used.
__device__ __forceinline__ uint32_t contend(uint32_t* g, uint64_t seed, uint32_t r, uint32_t slot0,
                                            uint32_t t) {
  unsigned long long* g64 = (unsigned long long*)g;
  const auto op = [&](uint32_t x) { return gm_ldsscan_a_op(seed, r, slot0 + x, 0, t); };
  const auto op64 = [&](uint32_t k) { return gm_ldsscan_a_op64(seed, r, slot0 + 2 * k, 0, t); };
  (void)__hip_atomic_fetch_add(&g64[GM_LDSSCAN_A_ADD64], op64(GM_LDSSCAN_A_ADD64), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_min((long long*)&g64[GM_LDSSCAN_A_MIN64],
                               (long long)op64(GM_LDSSCAN_A_MIN64), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_max(&g64[GM_LDSSCAN_A_MAX64], op64(GM_LDSSCAN_A_MAX64), GM_RLX, GM_WG);
  uint32_t gave_up = cas_add(&g64[GM_LDSSCAN_A_CAS64], (unsigned long long)op64(GM_LDSSCAN_A_CAS64));
  (void)__hip_atomic_fetch_add(&g[GM_LDSSCAN_G_ADD], op(GM_LDSSCAN_G_ADD), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_sub(&g[GM_LDSSCAN_G_SUB], op(GM_LDSSCAN_G_SUB), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_min((int*)&g[GM_LDSSCAN_G_SMIN], (int)op(GM_LDSSCAN_G_SMIN), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_max((int*)&g[GM_LDSSCAN_G_SMAX], (int)op(GM_LDSSCAN_G_SMAX), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_min(&g[GM_LDSSCAN_G_UMIN], op(GM_LDSSCAN_G_UMIN), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_max(&g[GM_LDSSCAN_G_UMAX], op(GM_LDSSCAN_G_UMAX), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_and(&g[GM_LDSSCAN_G_AND], gm_ldsscan_a_and_op(op(GM_LDSSCAN_G_AND)), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_or(&g[GM_LDSSCAN_G_OR], gm_ldsscan_a_or_op(op(GM_LDSSCAN_G_OR)), GM_RLX, GM_WG);
  (void)__hip_atomic_fetch_xor(&g[GM_LDSSCAN_G_XOR], op(GM_LDSSCAN_G_XOR), GM_RLX, GM_WG);
  gave_up += cas_add(&g[GM_LDSSCAN_G_CAS], op(GM_LDSSCAN_G_CAS));
  (void)__hip_atomic_fetch_add((float*)&g[GM_LDSSCAN_G_FADD], gm_ldsscan_a_fop(op(GM_LDSSCAN_G_FADD)),
                               GM_RLX, GM_WG);
  return gave_up;
}

// The returning form of private kind k on *p with operand h (compare-and-swap: comparand cmp).
template <uint32_t k>
__device__ __forceinline__ uint32_t private32(uint32_t* p, uint32_t h, uint32_t cmp) {
  if constexpr (k == GM_LDSSCAN_A_ADD) return __hip_atomic_fetch_add(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_SUB) return __hip_atomic_fetch_sub(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_INC)
    return __builtin_amdgcn_atomic_inc32(p, gm_ldsscan_a_bound(h), GM_RLX, "workgroup");
  if constexpr (k == GM_LDSSCAN_A_DEC)
    return __builtin_amdgcn_atomic_dec32(p, gm_ldsscan_a_bound(h), GM_RLX, "workgroup");
  if constexpr (k == GM_LDSSCAN_A_SMIN) return (uint32_t)__hip_atomic_fetch_min((int*)p, (int)h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_SMAX) return (uint32_t)__hip_atomic_fetch_max((int*)p, (int)h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_UMIN) return __hip_atomic_fetch_min(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_UMAX) return __hip_atomic_fetch_max(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_AND) return __hip_atomic_fetch_and(p, gm_ldsscan_a_and_op(h), GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_OR) return __hip_atomic_fetch_or(p, gm_ldsscan_a_or_op(h), GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_XOR) return __hip_atomic_fetch_xor(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_XCHG) return __hip_atomic_exchange(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_CAS) {
    (void)__hip_atomic_compare_exchange_strong(p, &cmp, h, GM_RLX, GM_RLX, GM_WG);
    return cmp;  // the old value, whether it matched or not
  }
}
template <uint32_t k>
__device__ __forceinline__ unsigned long long private64(unsigned long long* p, unsigned long long h,
                                                        unsigned long long cmp) {
  if constexpr (k == GM_LDSSCAN_A_ADD64) return __hip_atomic_fetch_add(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_MIN64)
    return (unsigned long long)__hip_atomic_fetch_min((long long*)p, (long long)h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_MAX64) return __hip_atomic_fetch_max(p, h, GM_RLX, GM_WG);
  if constexpr (k == GM_LDSSCAN_A_CAS64) {
    (void)__hip_atomic_compare_exchange_strong(p, &cmp, h, GM_RLX, GM_RLX, GM_WG);
    return cmp;
  }
}

template <uint32_t k>
__device__ __forceinline__ void private32_steps(uint32_t* tab, uint64_t seed, uint32_t r, uint32_t t,
                                                uint32_t& olds) {
  if constexpr (k < GM_LDSSCAN_A_KINDS32) {
    const uint32_t word = GM_LDSSCAN_A_P32 + 256 * k + t;
    uint32_t cmp = gm_ldsscan_a_init_word(seed, r, word);
#pragma unroll
    for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
      const uint32_t h = gm_ldsscan_a_op(seed, r, k, s, t);
      olds = gm_ldsscan_fold(olds, private32<k>(&tab[word], h, cmp));
      cmp = ~h;
    }
    private32_steps<k + 1>(tab, seed, r, t, olds);
  }
}
template <uint32_t k>
__device__ __forceinline__ void private64_steps(uint32_t* tab, uint64_t seed, uint32_t r, uint32_t t,
                                                uint32_t& olds) {
  if constexpr (k < GM_LDSSCAN_A_KINDS64) {
    const uint32_t word = GM_LDSSCAN_A_P64 + 2 * (256 * k + t);
    unsigned long long cmp = (unsigned long long)gm_ldsscan_a_init_word(seed, r, word + 1) << 32 |
                             gm_ldsscan_a_init_word(seed, r, word);
#pragma unroll
    for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
      const unsigned long long h = gm_ldsscan_a_op64(seed, r, GM_LDSSCAN_A_SLOT_P64 + 2 * k, s, t);
      const unsigned long long old = private64<k>((unsigned long long*)&tab[word], h, cmp);
      olds = gm_ldsscan_fold(gm_ldsscan_fold(olds, (uint32_t)old), (uint32_t)(old >> 32));
      cmp = ~h;
    }
    private64_steps<k + 1>(tab, seed, r, t, olds);
  }
}

__device__ __forceinline__ void test_atomic(const Ctx& c, uint32_t sig[4]) {
  const uint32_t t = threadIdx.x, w = t >> 6;
  uint32_t* tab = c.lds;  // GM_LDSSCAN_A_TABLE_WORDS words of it
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < c.iters; ++r) {
    for (uint32_t a = t; a < GM_LDSSCAN_A_TABLE_WORDS; a += GM_CUSCAN_THREADS)
      tab[a] = gm_ldsscan_a_init_word(c.seed, r, a);
    __syncthreads();
    // (a) private: the old values are this thread's alone
    private32_steps<0>(tab, c.seed, r, t, sig[0]);
    private64_steps<0>(tab, c.seed, r, t, sig[0]);
#pragma unroll
    for (uint32_t s = 0; s < GM_LDSSCAN_A_STEPS; ++s) {
      const float old = __hip_atomic_fetch_add(
          (float*)&tab[GM_LDSSCAN_A_PF + t],
          gm_ldsscan_a_fop(gm_ldsscan_a_op(c.seed, r, GM_LDSSCAN_A_SLOT_PF, s, t)), GM_RLX, GM_WG);
      sig[0] = gm_ldsscan_fold(sig[0], gm_cuscan_f32_bits(old));
    }
    // (b) contended: the block's group, then the wave's (64 lanes of one instruction)
    uint32_t gave_up = contend(tab + GM_LDSSCAN_A_GROUPS, c.seed, r, GM_LDSSCAN_A_SLOT_BLOCK, t);
    gave_up += contend(tab + GM_LDSSCAN_A_GROUPS + (1 + w) * GM_LDSSCAN_G_WORDS, c.seed, r,
                       GM_LDSSCAN_A_SLOT_WAVE, t);
    // (c) tickets: the ticket itself is used and never folded. A wrong ticket stays inside the
    // bitmap.
#pragma unroll
    for (uint32_t k = 0; k < GM_LDSSCAN_A_TICKETS; ++k) {
      const uint32_t ticket = __hip_atomic_fetch_add(&tab[GM_LDSSCAN_A_TICKET], 1u, GM_RLX, GM_WG);
      (void)__hip_atomic_fetch_or(&tab[GM_LDSSCAN_A_BITMAP + (ticket >> 5) % GM_LDSSCAN_A_BITMAP_WORDS],
                                  1u << (ticket & 31), GM_RLX, GM_WG);
    }
    __syncthreads();
    // the final values
#pragma unroll
    for (uint32_t k = 0; k < GM_LDSSCAN_A_KINDS32; ++k)
      sig[1] = gm_ldsscan_fold(sig[1], tab[GM_LDSSCAN_A_P32 + 256 * k + t]);
#pragma unroll
    for (uint32_t k = 0; k < 2 * GM_LDSSCAN_A_KINDS64; ++k)
      sig[1] = gm_ldsscan_fold(sig[1], tab[GM_LDSSCAN_A_P64 + 2 * (256 * (k >> 1) + t) + (k & 1)]);
    sig[1] = gm_ldsscan_fold(sig[1], tab[GM_LDSSCAN_A_PF + t]);
    for (uint32_t x = 0; x < GM_LDSSCAN_G_USED; ++x)
      sig[2] = gm_ldsscan_fold(sig[2], tab[GM_LDSSCAN_A_GROUPS + x]);
    for (uint32_t x = 0; x < GM_LDSSCAN_G_USED; ++x)
      sig[2] = gm_ldsscan_fold(sig[2], tab[GM_LDSSCAN_A_GROUPS + (1 + w) * GM_LDSSCAN_G_WORDS + x]);
    sig[2] = gm_ldsscan_fold(sig[2], gave_up);  // 0
    sig[3] = gm_ldsscan_fold(sig[3], tab[GM_LDSSCAN_A_TICKET]);
    for (uint32_t x = 0; x < GM_LDSSCAN_A_BITMAP_WORDS; ++x)
      sig[3] = gm_ldsscan_fold(sig[3], tab[GM_LDSSCAN_A_BITMAP + x]);
    __syncthreads();  // the next round's initial values overwrite what was read here
  }
}

// ================================================================================ bank
__device__ __forceinline__ void test_bank(const Ctx& c, uint32_t sig[4]) {
  const uint32_t t = threadIdx.x, w = t >> 6, l = t & 63;
  constexpr uint32_t W = GM_LDSSCAN_WORDS, T = GM_CUSCAN_THREADS;
  uint32_t* lds = c.lds;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < c.iters; ++r) {
    // no two lanes of one instruction share a word: the schedule is a permutation
    for (uint32_t i = 0; i < W / T; ++i) {
      const uint32_t a = gm_ldsscan_b_word32(gm_ldsscan_b_g(w, i, 0), l, r, 0);  // < 40960
      lds[a] = gm_ldsscan_pattern(c.seed, GM_LDSSCAN_H_BANK, r, 0, a);
    }
    filled(c, GM_LDSSCAN_BANK, r == 0);
    for (uint32_t i = 0; i < W / T; ++i)
      sig[0] = gm_ldsscan_fold(sig[0], lds[gm_ldsscan_b_word32(gm_ldsscan_b_g(w, i, 1), l, r, 3)]);
    for (uint32_t i = 0; i < W / 2 / T; ++i) {
      const u32x2 v = ((const u32x2*)lds)[gm_ldsscan_b_elem64(gm_ldsscan_b_g(w, i, 2), l, r)];  // < 20480
      sig[1] = gm_ldsscan_fold(sig[1], v.x);
      sig[2] = gm_ldsscan_fold(sig[2], v.y);
    }
    for (uint32_t i = 0; i < GM_LDSSCAN_B_BCAST_STEPS; ++i) {
      const uint32_t g = gm_ldsscan_b_g(w, i, 0);
      sig[3] = gm_ldsscan_fold(sig[3], lds[gm_ldsscan_b_all(g, r)]);  // all three < 40960
      sig[3] = gm_ldsscan_fold(sig[3], lds[gm_ldsscan_b_half(g, l, r)]);
      sig[3] = gm_ldsscan_fold(sig[3], lds[gm_ldsscan_b_pair(g, l, r)]);
    }
    __syncthreads();
  }
}

// ================================================================================ tr16
// EXEC is all ones at the read: every trip count is uniform, there is no branch around it and
// all 256 threads get here.
__device__ __forceinline__ void test_tr16(const Ctx& c, uint32_t sig[4]) {
  const uint32_t t = threadIdx.x;
  uint32_t* lds = c.lds;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < c.iters; ++r) {
    for (uint32_t k = 0; k < GM_LDSSCAN_WORDS / 4 / GM_CUSCAN_THREADS; ++k) {
      const uint32_t v = k * 256 + t;  // < 10240
      const u32x4 p = {gm_ldsscan_pattern(c.seed, GM_LDSSCAN_H_TR16, r, 0, 4 * v),
                       gm_ldsscan_pattern(c.seed, GM_LDSSCAN_H_TR16, r, 0, 4 * v + 1),
                       gm_ldsscan_pattern(c.seed, GM_LDSSCAN_H_TR16, r, 0, 4 * v + 2),
                       gm_ldsscan_pattern(c.seed, GM_LDSSCAN_H_TR16, r, 0, 4 * v + 3)};
      ((u32x4*)lds)[v] = p;
    }
    filled(c, GM_LDSSCAN_TR16, r == 0);
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
      for (uint32_t i = 0; i < GM_LDSSCAN_T_STEPS; ++i) {
        // 8-byte aligned, and the block's last byte is inside the LDS: gm_ldsscan_t_origins
        const uint32_t at = gm_ldsscan_t_addr(k, 16 * i + (t >> 4), r, t & 15);
        const i16x4 e = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) i16x4*)((char*)lds + at));
        const uint32_t lo = (uint16_t)e.x | (uint32_t)(uint16_t)e.y << 16;
        const uint32_t hi = (uint16_t)e.z | (uint32_t)(uint16_t)e.w << 16;
        sig[k] = gm_ldsscan_fold(gm_ldsscan_fold(sig[k], lo), hi);
        sig[3] = gm_ldsscan_fold(sig[3], lo ^ gm_cuscan_rotl32(hi, 13));
      }
    __syncthreads();
  }
}

// ================================================================================ dma
__device__ __forceinline__ void test_dma(const Ctx& c, const uint32_t* __restrict__ arena,
                                         uint32_t sig[4]) {
  const uint32_t t = threadIdx.x, l = t & 63;
  const uint32_t w = __builtin_amdgcn_readfirstlane(t >> 6);
  uint32_t* lds = c.lds;
  sig[0] = sig[1] = sig[2] = sig[3] = 0;
  for (uint32_t r = 0; r < c.iters; ++r) {
    for (uint32_t i = 0; i < GM_LDSSCAN_D_CHUNKS / 4; ++i) {
      const uint32_t chunk = 4 * i + w;  // < 160, uniform in the wave
      // the source ends at most at byte 163840 of the arena: gm_ldsscan_d_src_byte
      if (gm_ldsscan_d_wide(chunk, r)) {
        __builtin_amdgcn_global_load_lds(
            (gbl_void*)((const char*)arena + gm_ldsscan_d_src_byte(chunk, r, l, 0)),
            (lds_void*)((char*)lds + gm_ldsscan_d_dst_byte(chunk, r, 0)), 16, 0, 0);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
          __builtin_amdgcn_global_load_lds(
              (gbl_void*)((const char*)arena + gm_ldsscan_d_src_byte(chunk, r, l, j)),
              (lds_void*)((char*)lds + gm_ldsscan_d_dst_byte(chunk, r, j)), 4, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t i = 0; i < GM_LDSSCAN_D_CHUNKS / 4; ++i)
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        uint32_t x, a;
        gm_ldsscan_d_item(4 * i + ((w + 1) & 3), r, 64 * j + l, x, a);  // x < 40960
        gm_ldsscan_d_fold(sig, lds[x], gm_ldsscan_d_arena(c.seed, a));
      }
    __syncthreads();  // the next round's loads overwrite what other waves read here
  }
}

// kCompare / !kCompare as k_cuscan: the scan, or one block's raw signature of the one test in
// p.tests.
template <bool kCompare>
__global__ __launch_bounds__(GM_CUSCAN_THREADS) void k_ldsscan(
    Params p, gm_ldsscan_poke_t poke, const uint32_t* __restrict__ arena,
    const uint32_t* __restrict__ expected, DevTable* tab, uint32_t* sig_out, uint32_t* where_out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[GM_CUSCAN_LDS_WORDS];
  const Where at = where_am_i();
  const Ctx c = {lds, p.seed, p.iters, poke};
  uint32_t failed = 0, bad = 0;
  uint32_t sig[4];
  if (p.tests & GM_LDSSCAN_WIDTH) {
    test_width(c, sig);
    finish<kCompare>(p, GM_LDSSCAN_WIDTH, GM_LDSSCAN_IX_WIDTH, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_LDSSCAN_ATOMIC) {
    test_atomic(c, sig);
    finish<kCompare>(p, GM_LDSSCAN_ATOMIC, GM_LDSSCAN_IX_ATOMIC, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_LDSSCAN_BANK) {
    test_bank(c, sig);
    finish<kCompare>(p, GM_LDSSCAN_BANK, GM_LDSSCAN_IX_BANK, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_LDSSCAN_TR16) {
    test_tr16(c, sig);
    finish<kCompare>(p, GM_LDSSCAN_TR16, GM_LDSSCAN_IX_TR16, at, sig, expected, tab, sig_out, failed, bad);
  }
  if (p.tests & GM_LDSSCAN_DMA) {
    test_dma(c, arena, sig);
    finish<kCompare>(p, GM_LDSSCAN_DMA, GM_LDSSCAN_IX_DMA, at, sig, expected, tab, sig_out, failed, bad);
  }
  book_block<kCompare>(lds, at, failed, bad, tab, where_out);
}

bool iters_ok(uint32_t, uint32_t iters) { return iters >= 1 && iters <= GM_LDSSCAN_MAX_ITERS; }

constexpr ScanArgs kArgs = {GM_LDSSCAN_ALL, iters_ok};

// a poke of one selected test that has data, inside the LDS image or the arena
bool poke_ok(const gm_ldsscan_poke_t* pk, uint32_t tests) {
  if (!one_bit_ok(kArgs, pk->test) || !(pk->test & tests) || pk->mask == 0) return false;
  return pk->test != GM_LDSSCAN_ATOMIC && pk->word_offset < GM_LDSSCAN_WORDS;
}

// the table of `test` in a run with `pk` (null: none): a poke of another test leaves it alone
void expected_of(uint32_t test, uint64_t seed, uint32_t iters, const gm_ldsscan_poke_t* pk,
                 uint32_t* out) {
  const bool mine = pk && pk->test == test;
  gm_ldsscan_expected_host(test, seed, iters, mine ? pk->word_offset : 0, mine ? pk->mask : 0, out);
}

// The arena every block reads, filled once per call; the host makes the dma test's poke.
struct Arena {
  DevBuf buf;
  int fill(uint64_t seed, const gm_ldsscan_poke_t* pk, hipStream_t stream) {
    std::vector<uint32_t> h(GM_LDSSCAN_ARENA_WORDS);
    for (uint32_t a = 0; a < GM_LDSSCAN_ARENA_WORDS; ++a) h[a] = gm_ldsscan_d_arena(seed, a);
    if (pk && pk->test == GM_LDSSCAN_DMA) h[pk->word_offset] ^= pk->mask;
    GM_CHECK(buf.alloc(GM_LDSSCAN_ARENA_BYTES));
    GM_CHECK(hipMemcpyAsync(buf.p, h.data(), GM_LDSSCAN_ARENA_BYTES, hipMemcpyHostToDevice, stream));
    GM_CHECK(hipStreamSynchronize(stream));  // h goes out of scope
    return 0;
  }
};

}  // namespace

extern "C" {

int gm_probe_ldsscan_expected(uint32_t test, uint64_t seed, uint32_t iters,
                              const gm_ldsscan_poke_t* poke, uint32_t* out) {
  if (!one_test_ok(kArgs, test, iters) || !out) return (int)hipErrorInvalidValue;
  // a poke of another test is a legal run in which this test's table is the clean one
  if (poke && !poke_ok(poke, GM_LDSSCAN_ALL)) return (int)hipErrorInvalidValue;
  expected_of(test, seed, iters, poke, out);
  return 0;
}

int gm_probe_ldsscan_geometry(uint32_t* lds_bytes, uint32_t* arena_bytes,
                              uint32_t* atomic_table_words, uint32_t tr16_strides[3]) {
  if (!lds_bytes || !arena_bytes || !atomic_table_words || !tr16_strides)
    return (int)hipErrorInvalidValue;
  *lds_bytes = GM_LDSSCAN_BYTES;
  *arena_bytes = GM_LDSSCAN_ARENA_BYTES;
  *atomic_table_words = GM_LDSSCAN_A_TABLE_WORDS;
  for (uint32_t k = 0; k < 3; ++k) tr16_strides[k] = gm_ldsscan_t_stride(k);
  return 0;
}

int gm_probe_ldsscan_signature(uint32_t test, uint64_t seed, uint32_t iters,
                               const gm_ldsscan_poke_t* poke, uint32_t* dev_out,
                               uint32_t* dev_where, void* stream) {
  if (!one_test_ok(kArgs, test, iters) || !signature_out_ok(dev_out, dev_where) ||
      (poke && !poke_ok(poke, test)))
    return (int)hipErrorInvalidValue;
  const Params p = params_of(seed, test, iters);
  Arena arena;
  if (int e = arena.fill(seed, poke, (hipStream_t)stream)) return e;
  hipLaunchKernelGGL(k_ldsscan<false>, dim3(1), dim3(GM_CUSCAN_THREADS), 0, (hipStream_t)stream, p,
                     poke ? *poke : gm_ldsscan_poke_t{}, (const uint32_t*)arena.buf.p,
                     (const uint32_t*)nullptr, (DevTable*)nullptr, dev_out, dev_where);
  GM_CHECK(hipGetLastError());
  // the arena is freed once the block that reads it is done
  GM_CHECK(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int gm_probe_ldsscan(int dev, uint32_t tests_mask, uint32_t iters, uint64_t seed, int min_rounds,
                     int max_rounds, const gm_cuscan_inject_t* inject, const gm_ldsscan_poke_t* poke,
                     gm_cuscan_result_t* out, gm_cuscan_cu_t* cus, int cus_cap, int* n_cus) {
  if (!scan_args_ok(kArgs, tests_mask, iters, min_rounds, max_rounds, inject, out, cus, cus_cap,
                    n_cus) ||
      (poke && !poke_ok(poke, tests_mask)))
    return (int)hipErrorInvalidValue;
  const Params p = params_of(seed, tests_mask, iters, inject);
  const gm_ldsscan_poke_t pk = poke ? *poke : gm_ldsscan_poke_t{};
  DeviceGuard g(dev);  // the arena is this device's, from the first launch to the read
  if (!g.ok) return (int)hipErrorInvalidDevice;
  Arena arena;
  return run_scan_with(
      dev, (const void*)k_ldsscan<true>, (size_t)GM_LDSSCAN_TESTS * GM_CUSCAN_SIG_WORDS,
      [&](uint32_t* exp) {
        // the clean table also under a poke: the poked word is what the compare is to find
        for (int t = 0; t < GM_LDSSCAN_TESTS; ++t)
          if (tests_mask & (1u << t))
            expected_of(1u << t, seed, iters, nullptr, exp + (size_t)t * GM_CUSCAN_SIG_WORDS);
      },
      [&](int blocks, const uint32_t* expected, DevTable* tab) {
        if (!arena.buf.p)
          if (int e = arena.fill(seed, poke, nullptr)) return e;
        hipLaunchKernelGGL(k_ldsscan<true>, dim3((unsigned)blocks), dim3(GM_CUSCAN_THREADS), 0,
                           nullptr, p, pk, (const uint32_t*)arena.buf.p, expected, tab,
                           (uint32_t*)nullptr, (uint32_t*)nullptr);
        return (int)hipGetLastError();
      },
      min_rounds, max_rounds, out, cus, cus_cap, n_cus);
}

int gm_probe_ldsscan_kernel_info(int* num_regs, int* scratch_bytes) {
  if (!num_regs || !scratch_bytes) return (int)hipErrorInvalidValue;
  hipFuncAttributes attr;
  GM_CHECK(hipFuncGetAttributes(&attr, (const void*)k_ldsscan<true>));
  *num_regs = attr.numRegs;
  *scratch_bytes = (int)attr.localSizeBytes;
  return 0;
}

}  // extern "C"
