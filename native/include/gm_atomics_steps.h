// gm_atomics_steps.h — the atomics family's operations, once: what one thread g does in step s of
// the add, ticket, CAS and swap tests, for the agent-scope kernels (native/hip/gm_atomics.hip),
// the system-scope kernels (native/hip/gm_hostsync.hip) and the host threads
// (gm_hostsync_host.h). Plain C++ with no HIP include. A step takes its atomic primitive from a
// policy class `Ops` with static members
//   fetch_add(T*, T)  exchange(u32*, u32)  load(const u64*)  cas(u64*, u64* old, u64 want)
// and, where Ops::kKinds is GM_ATOMICS_ADD_KINDS, fetch_xor/max/min/and/or and pk_add_bf16 for the
// other add kinds; a policy with kKinds 2 has the two integer adds only. Everything a step
// computes comes from the value functions of gm_atomics_ref.h and gm_hostsync_ref.h, which the
// host reference folds too. No step waits: the CAS loop ends after bound[w] failed exchanges
// whatever the other participants do. Every index is masked (a(g, s) < width, a power of two) or
// checked against its table (the ticket's room) before it is used.
#pragma once
#include <stdint.h>

#include "gm_hostsync_ref.h"

static_assert((int)GM_HOSTSYNC_ADD == (int)GM_ATOMICS_ADD &&
                  (int)GM_HOSTSYNC_TICKET == (int)GM_ATOMICS_TICKET &&
                  GM_HOSTSYNC_LINE_WORDS == GM_ATOMICS_LINE_WORDS,
              "the two tests share their steps");

// A negative control in the form the steps use. ADD, CAS, SWAP: H or the token of operation
// (a, b) = (g, s) is XORed with mask; TICKET: that draw marks its first slot twice; HANDOFF:
// word `word` of mailbox (a, b) = (block, round), host-sync: of direction `dir`.
struct gm_atomics_inj_t {
  uint32_t a = 0, b = 0, word = 0, mask = 0, dir = 0, on = 0;  // on 0: none
};
typedef gm_atomics_inj_t gm_hostsync_inj_t;

GM_ATOMICS_HD bool gm_atomics_inj_hit(const gm_atomics_inj_t& inj, uint32_t a, uint32_t b) {
  return inj.on && a == inj.a && b == inj.b;
}

// ---- ADD: one no-return operation of `kind` into a table of `width` words of 4 or 8 bytes
template <class Ops>
GM_ATOMICS_HD void gm_atomics_add_step(uint32_t kind, void* table, uint32_t width, uint64_t seed,
                                       const gm_atomics_inj_t& inj, uint32_t g, uint32_t s) {
  uint32_t h = gm_atomics_hash(seed, kind, 0, g, s);
  if (gm_atomics_inj_hit(inj, g, s)) h ^= inj.mask;
  const uint32_t w = gm_atomics_addr(g, s, width);
  uint32_t* p32 = (uint32_t*)table + w;
  uint64_t* p64 = (uint64_t*)table + w;
  if (kind == GM_ATOMICS_K_ADD_U64) {
    Ops::fetch_add(p64, gm_atomics_op64(seed, kind, h, g, s));
  } else if (Ops::kKinds == 2 || kind == GM_ATOMICS_K_ADD_U32) {
    Ops::fetch_add(p32, h);
  } else if constexpr (Ops::kKinds == GM_ATOMICS_ADD_KINDS) {
    switch (kind) {
      case GM_ATOMICS_K_XOR_U64: Ops::fetch_xor(p64, gm_atomics_op64(seed, kind, h, g, s)); break;
      case GM_ATOMICS_K_UMAX_U32: Ops::fetch_max(p32, h); break;
      case GM_ATOMICS_K_UMIN_U32: Ops::fetch_min(p32, h); break;
      case GM_ATOMICS_K_AND_U32: Ops::fetch_and(p32, ~gm_atomics_bit(h)); break;
      case GM_ATOMICS_K_OR_U32: Ops::fetch_or(p32, gm_atomics_bit(h)); break;
      case GM_ATOMICS_K_ADD_F32: Ops::fetch_add((float*)p32, (float)gm_atomics_small(h)); break;
      case GM_ATOMICS_K_ADD_F64: Ops::fetch_add((double*)p64, (double)gm_atomics_small(h)); break;
      case GM_ATOMICS_K_PK_ADD_BF16: Ops::pk_add_bf16(p32, h & 1u, (h >> 1) & 1u); break;
    }
  }
}

// ---- TICKET: a returning fetch-add of d = 1..4 on counter k, then one mark per ticket drawn;
// off[k] .. off[k + 1] are counter k's marks, n_marks in all. Returns the tickets that fell
// outside the counter's marks; `old` and `d` are what the draw got and took.
template <class Ops>
GM_ATOMICS_HD uint32_t gm_atomics_ticket_step(uint32_t* ctr, const uint64_t* off, uint32_t* marks,
                                              uint64_t n_marks, uint32_t counters, uint64_t seed,
                                              const gm_atomics_inj_t& inj, uint32_t g, uint32_t s,
                                              uint32_t& old, uint32_t& d) {
  d = gm_atomics_draw(gm_atomics_hash(seed, GM_ATOMICS_K_TICKET, 0, g, s));
  const uint32_t k = gm_atomics_addr(g, s, counters);
  const uint64_t base = off[k];
  // N_k, and never past the end of the marks whatever off[] holds
  const uint64_t room =
      base < n_marks && off[k + 1] - base <= n_marks - base ? off[k + 1] - base : 0;
  old = Ops::fetch_add(&ctr[k], d);
  uint32_t out_of_range = 0;
  for (uint32_t i = 0; i < d; ++i) {
    const uint64_t ticket = (uint64_t)old + i;
    if (ticket < room)
      Ops::fetch_add(&marks[base + ticket], 1u);
    else
      ++out_of_range;
  }
  if (gm_atomics_inj_hit(inj, g, s) && old < room) Ops::fetch_add(&marks[base + old], 1u);
  return out_of_range;
}

// ---- CAS: add u64 through a compare-exchange loop. Every failed exchange means that another
// participant's succeeded, and bound[w] operations go into word w in all, so a correct machine
// cannot fail bound[w] times: the loop ends after at most that many rounds whatever the others
// do. False: given up.
template <class Ops>
GM_ATOMICS_HD bool gm_atomics_cas_step(uint64_t* table, const uint32_t* bound, uint32_t width,
                                       uint64_t seed, const gm_atomics_inj_t& inj, uint32_t g,
                                       uint32_t s) {
  uint32_t h = gm_atomics_hash(seed, GM_ATOMICS_K_CAS, 0, g, s);
  if (gm_atomics_inj_hit(inj, g, s)) h ^= inj.mask;
  const uint64_t op = gm_atomics_op64(seed, GM_ATOMICS_K_CAS, h, g, s);
  const uint32_t w = gm_atomics_addr(g, s, width);
  const uint32_t limit = bound[w];
  uint64_t old = Ops::load(&table[w]);
  uint32_t fails = 0;
  while (!Ops::cas(&table[w], &old, old + op))
    if (++fails >= limit) return false;
  return true;
}

// ---- SWAP: the operation's token goes into its word; returns what the word held
template <class Ops>
GM_ATOMICS_HD uint32_t gm_hostsync_swap_step(uint32_t* words, uint32_t width,
                                             const gm_atomics_inj_t& inj, uint32_t g, uint32_t s) {
  uint32_t token = gm_hostsync_token(g, s);
  if (gm_atomics_inj_hit(inj, g, s)) token ^= inj.mask;
  return Ops::exchange(&words[gm_atomics_addr(g, s, width)], token);
}

// The policy of the host threads: the __atomic_* builtins, relaxed, on the words the kernel works
// on at system scope. PCIe AtomicOps carry add, swap and CAS, so the integer adds are all it has.
struct gm_atomics_host_ops {
  static constexpr uint32_t kKinds = 2;
  template <class T>
  static T fetch_add(T* p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
  static uint32_t exchange(uint32_t* p, uint32_t v) {
    return __atomic_exchange_n(p, v, __ATOMIC_RELAXED);
  }
  static uint64_t load(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static bool cas(uint64_t* p, uint64_t* old, uint64_t want) {
    return __atomic_compare_exchange_n(p, old, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
  }
};
