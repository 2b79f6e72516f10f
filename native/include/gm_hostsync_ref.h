// gm_hostsync_ref.h — the host-sync test's value functions and host reference, one definition for
// the host (gm_probe_hostsync_expected, the audits), the host threads (gm_hostsync_host.h) and the
// gfx950 kernels (native/hip/gm_hostsync.hip). The formulas are written out in gm_probe.h. The
// atomic tests reuse the atomics test's H, a(g, s), op64, draw, widths and caps
// (gm_atomics_ref.h) over blocks + host_threads virtual blocks; nothing of it is copied here.
#pragma once
#include <stdint.h>

#include <vector>

#include "gm_atomics_ref.h"

#define GM_HOSTSYNC_HD GM_CUSCAN_HD

enum {
  GM_HOSTSYNC_ADD = 1,
  GM_HOSTSYNC_TICKET = 2,
  GM_HOSTSYNC_SWAP = 4,
  GM_HOSTSYNC_CAS = 8,
  GM_HOSTSYNC_HANDOFF = 16,
  GM_HOSTSYNC_ATOMIC_TESTS = 15,
  GM_HOSTSYNC_ALL = 31,
};

// pseudo-kind of gm_probe_hostsync_expected beside the atomics kinds 0, 1, 10, 11 and 13
#define GM_HOSTSYNC_K_SWAP 14u

#define GM_HOSTSYNC_THREADS GM_ATOMICS_THREADS
#define GM_HOSTSYNC_MAX_BLOCKS 4096u       /* the driver also caps at the CU count */
#define GM_HOSTSYNC_DEFAULT_BLOCKS 16u     /* min(16, CUs): every block is resident */
#define GM_HOSTSYNC_MAX_HOST_THREADS 8u
#define GM_HOSTSYNC_DEFAULT_HOST_THREADS 2u
#define GM_HOSTSYNC_MAX_ITERS 1024u
#define GM_HOSTSYNC_DEFAULT_ITERS 4u
#define GM_HOSTSYNC_MAX_OPS (1ull << 20)   /* (blocks + host_threads) * 256 * iters */
#define GM_HOSTSYNC_MAX_SPREAD GM_ATOMICS_MAX_SPREAD
#define GM_HOSTSYNC_DEFAULT_SPREAD 4096u
#define GM_HOSTSYNC_MAX_ROUNDS 64u
#define GM_HOSTSYNC_DEFAULT_ROUNDS 8u
#define GM_HOSTSYNC_DEFAULT_LINES 16u
#define GM_HOSTSYNC_LINE_WORDS 1024u       /* 4 KiB: 16 bytes per thread */
#define GM_HOSTSYNC_FLAG_WORDS 32u         /* a flag has a 128-byte line of its own */
#define GM_HOSTSYNC_MAX_BUDGET_US 20000u
#define GM_HOSTSYNC_DEFAULT_BUDGET_US 2251u       /* max(1000, 8 x 281.36 us): BASELINE.md */
#define GM_HOSTSYNC_MAX_HOST_BUDGET_US 100000u
#define GM_HOSTSYNC_DEFAULT_HOST_BUDGET_US 5000u  /* max(5000, 8 x 0.13 us): BASELINE.md */
#define GM_HOSTSYNC_START_BOUND_US 2000000u       /* a host thread waits this long for `ready` */
#define GM_HOSTSYNC_MAX_MAILBOX_BYTES (1ull << 28) /* both directions together, pinned */
#define GM_HOSTSYNC_HASH_BASE 0x600u       /* 0x100 atomics, 0x200 mfma, 0x300 lane, 0x400 cache,
                                              0x500 lds */

// swap: the token operation (g, s) stores; never 0, which is what the words start with
GM_HOSTSYNC_HD uint32_t gm_hostsync_token(uint32_t g, uint32_t s) {
  return 1u + GM_ATOMICS_MAX_ITERS * g + s;
}

// hand-off payload word E(dir, b, r, word): dir 0 host to device, 1 device to host; b < 4096,
// r < 64, word < 16384
GM_HOSTSYNC_HD uint32_t gm_hostsync_payload(uint64_t seed, uint32_t dir, uint32_t b, uint32_t r,
                                            uint32_t word) {
  return gm_cuscan_hash(seed, GM_HOSTSYNC_HASH_BASE + dir, (b << 20) | (r << 14) | word);
}

// ------------------------------------------------------------------------------ host only

// blocks GPU blocks and host_threads host-played ones, `iters` steps each
inline bool gm_hostsync_geometry_ok(uint32_t blocks, uint32_t host_threads, uint32_t iters) {
  return blocks >= 1 && blocks <= GM_HOSTSYNC_MAX_BLOCKS &&
         host_threads <= GM_HOSTSYNC_MAX_HOST_THREADS && iters >= 1 &&
         iters <= GM_HOSTSYNC_MAX_ITERS &&
         (uint64_t)(blocks + host_threads) * GM_HOSTSYNC_THREADS * iters <= GM_HOSTSYNC_MAX_OPS;
}

inline bool gm_hostsync_handoff_ok(uint32_t blocks, uint32_t host_threads, uint32_t rounds,
                                   uint32_t lines, uint32_t budget_us, uint32_t host_budget_us) {
  if (blocks < 1 || blocks > GM_HOSTSYNC_MAX_BLOCKS || host_threads < 1 ||
      host_threads > GM_HOSTSYNC_MAX_HOST_THREADS || rounds < 1 ||
      rounds > GM_HOSTSYNC_MAX_ROUNDS || (lines != 1 && lines != 16) || budget_us < 1 ||
      budget_us > GM_HOSTSYNC_MAX_BUDGET_US || host_budget_us < 1 ||
      host_budget_us > GM_HOSTSYNC_MAX_HOST_BUDGET_US)
    return false;
  return 2ull * blocks * rounds * (lines * 4096ull + 128ull) <= GM_HOSTSYNC_MAX_MAILBOX_BYTES;
}

// The swap test's audit. `returned` holds what each of the total_blocks * 256 * iters operations
// got back, at g * iters + s; `words` the table after the last one. The values seen at word w
// (the returns of the operations into w and its final value) must be the tokens of those
// operations and one 0, each once: a swap chain hands every value on exactly once.
//   missing     a token of w, or its 0, was not seen
//   duplicates  a value of w was seen n > 1 times: n - 1
//   foreign     a value seen at w is neither a token of w nor 0
// first_bad_word (may be NULL): the lowest word with a foreign value, else with any error; ~0 none.
struct gm_hostsync_swap_audit_t {
  uint64_t missing = 0, duplicates = 0, foreign = 0;
  uint64_t first_bad_word = ~0ull, first_bad_value = 0;
};

inline gm_hostsync_swap_audit_t gm_hostsync_swap_audit(uint32_t total_blocks, uint32_t iters,
                                                       uint32_t width, const uint32_t* returned,
                                                       const uint32_t* words) {
  const uint32_t T = total_blocks * GM_HOSTSYNC_THREADS;
  std::vector<uint8_t> seen((size_t)T * iters, 0), zero(width, 0);
  gm_hostsync_swap_audit_t a;
  auto book = [&](uint32_t w, uint32_t v) {
    if (v == 0) {
      if (zero[w] < 255) ++zero[w];
      return;
    }
    const uint32_t g = (v - 1u) / GM_ATOMICS_MAX_ITERS, s = (v - 1u) % GM_ATOMICS_MAX_ITERS;
    if (g < T && s < iters && gm_atomics_addr(g, s, width) == w) {
      if (seen[(size_t)g * iters + s] < 255) ++seen[(size_t)g * iters + s];
    } else {
      ++a.foreign;
      if (w < a.first_bad_word) a.first_bad_word = w, a.first_bad_value = v;
    }
  };
  for (uint32_t g = 0; g < T; ++g)
    for (uint32_t s = 0; s < iters; ++s)
      book(gm_atomics_addr(g, s, width), returned[(size_t)g * iters + s]);
  for (uint32_t w = 0; w < width; ++w) book(w, words[w]);
  const bool named = a.first_bad_word != ~0ull;
  auto count = [&](uint32_t w, uint32_t v, uint32_t n) {
    if (n == 1) return;
    if (n == 0) ++a.missing; else a.duplicates += n - 1u;
    if (!named && w < a.first_bad_word) a.first_bad_word = w, a.first_bad_value = v;
  };
  for (uint32_t g = 0; g < T; ++g)
    for (uint32_t s = 0; s < iters; ++s)
      count(gm_atomics_addr(g, s, width), gm_hostsync_token(g, s), seen[(size_t)g * iters + s]);
  for (uint32_t w = 0; w < width; ++w) count(w, 0, zero[w]);
  return a;
}

// The ticket test's audit on the host, with gm_probe.h's TICKET definitions: n[k] is the host's
// final value of counter k, the marks of counter k lie at off[k] .. off[k] + n[k].
struct gm_hostsync_ticket_audit_t {
  uint64_t holes = 0, duplicates = 0, counter_errors = 0;
  uint64_t first_index = ~0ull, first_expected = 0, first_got = 0;
};

inline gm_hostsync_ticket_audit_t gm_hostsync_ticket_audit(const uint32_t* ctr, const uint32_t* n,
                                                           uint32_t counters,
                                                           const uint32_t* marks,
                                                           uint64_t n_marks) {
  gm_hostsync_ticket_audit_t a;
  for (uint64_t i = 0; i < n_marks; ++i) {
    if (marks[i] == 1) continue;
    ++(marks[i] == 0 ? a.holes : a.duplicates);
    if (a.first_index == ~0ull) a.first_index = i, a.first_expected = 1, a.first_got = marks[i];
  }
  for (uint32_t k = 0; k < counters; ++k)
    if (ctr[k] != n[k]) {
      ++a.counter_errors;
      if (a.first_index == ~0ull)
        a.first_index = n_marks + k, a.first_expected = n[k], a.first_got = ctr[k];
    }
  return a;
}
