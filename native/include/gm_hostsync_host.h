// gm_hostsync_host.h — the host threads' side of the host-sync test, in plain C++ with no HIP:
// the operations a thread makes as a host-played block of the atomic tests (the steps of
// gm_atomics_steps.h with its __atomic_* policy, on the words the kernel works on at system
// scope), and the host half of the hand-off
// (produce, release the flag, acquire the reply's flag, compare). gm_hostsync.hip runs these in
// std::threads against the kernel; native/tests/test_hostsync_host.cpp runs them against a CPU
// stand-in for the kernel. Every wait here is bounded: the start by GM_HOSTSYNC_START_BOUND_US,
// the CAS loop by a count, a flag poll by host_budget_us.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "gm_atomics_steps.h"

// What the launching thread and the host threads share besides the test's words. `ready` lies in
// the memory the kernel writes; `done` and `abort` are the launching thread's.
struct gm_hostsync_gate_t {
  const uint32_t* ready = nullptr;  // the kernel stores 1 at its start
  uint32_t done = 0;                // the kernel's end event is no longer hipErrorNotReady
  uint32_t abort = 0;               // the launch failed: do nothing
};

inline double gm_hostsync_now_us() {
  return std::chrono::duration<double, std::micro>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

// true: go; false: the launch was called off. Returns after the start bound at the latest.
inline bool gm_hostsync_wait_start(const gm_hostsync_gate_t* gate) {
  const double t0 = gm_hostsync_now_us();
  for (;;) {
    if (__atomic_load_n(&gate->abort, __ATOMIC_ACQUIRE)) return false;
    if (__atomic_load_n(gate->ready, __ATOMIC_ACQUIRE)) return true;
    if (gm_hostsync_now_us() - t0 >= (double)GM_HOSTSYNC_START_BOUND_US) return true;
  }
}

inline bool gm_hostsync_in_flight(const gm_hostsync_gate_t* gate) {
  return __atomic_load_n(&gate->done, __ATOMIC_RELAXED) == 0;
}

// ---- the atomic tests: the thread plays block `vblock`, g = 256 vblock + t, step by step with
// the steps of gm_atomics_steps.h over gm_atomics_host_ops. Each returns the operations it made
// while the kernel was still running.

// step(g, s) for every thread t of the block, steps outermost as on the GPU
template <class Step>
inline uint64_t gm_hostsync_host_block(uint32_t vblock, uint32_t iters,
                                       const gm_hostsync_gate_t* gate, Step step) {
  uint64_t flying = 0;
  for (uint32_t s = 0; s < iters; ++s)
    for (uint32_t t = 0; t < GM_HOSTSYNC_THREADS; ++t) {
      step(vblock * GM_HOSTSYNC_THREADS + t, s);
      flying += gm_hostsync_in_flight(gate);
    }
  return flying;
}

// kind GM_ATOMICS_K_ADD_U32 or GM_ATOMICS_K_ADD_U64
inline uint64_t gm_hostsync_host_add(uint32_t kind, void* table, uint32_t width, uint32_t vblock,
                                     uint32_t iters, uint64_t seed, const gm_hostsync_inj_t& inj,
                                     const gm_hostsync_gate_t* gate) {
  return gm_hostsync_host_block(vblock, iters, gate, [&](uint32_t g, uint32_t s) {
    gm_atomics_add_step<gm_atomics_host_ops>(kind, table, width, seed, inj, g, s);
  });
}

// off[k] .. off[k + 1] are counter k's marks, n_marks in all
inline uint64_t gm_hostsync_host_ticket(uint32_t* ctr, const uint64_t* off, uint32_t* marks,
                                        uint64_t n_marks, uint32_t counters, uint32_t vblock,
                                        uint32_t iters, uint64_t seed,
                                        const gm_hostsync_inj_t& inj,
                                        const gm_hostsync_gate_t* gate, uint64_t* out_of_range) {
  return gm_hostsync_host_block(vblock, iters, gate, [&](uint32_t g, uint32_t s) {
    uint32_t old, d;
    *out_of_range += gm_atomics_ticket_step<gm_atomics_host_ops>(ctr, off, marks, n_marks,
                                                                 counters, seed, inj, g, s, old, d);
  });
}

// returned: this thread's 256 * iters values, at t * iters + s
inline uint64_t gm_hostsync_host_swap(uint32_t* words, uint32_t width, uint32_t vblock,
                                      uint32_t iters, const gm_hostsync_inj_t& inj,
                                      const gm_hostsync_gate_t* gate, uint32_t* returned) {
  return gm_hostsync_host_block(vblock, iters, gate, [&](uint32_t g, uint32_t s) {
    returned[(size_t)(g - vblock * GM_HOSTSYNC_THREADS) * iters + s] =
        gm_hostsync_swap_step<gm_atomics_host_ops>(words, width, inj, g, s);
  });
}

// bound[w]: the operations into word w; a thread gives an operation up after that many failures
inline uint64_t gm_hostsync_host_cas(uint64_t* table, const uint32_t* bound, uint32_t width,
                                     uint32_t vblock, uint32_t iters, uint64_t seed,
                                     const gm_hostsync_inj_t& inj, const gm_hostsync_gate_t* gate,
                                     uint64_t* giveups) {
  return gm_hostsync_host_block(vblock, iters, gate, [&](uint32_t g, uint32_t s) {
    *giveups += !gm_atomics_cas_step<gm_atomics_host_ops>(table, bound, width, seed, inj, g, s);
  });
}

// ---- the hand-off. Mailbox m = b * rounds + r of either direction lies at word
// m * lines * 1024 of its payload, its flag at word m * 32 of its flags.
struct gm_hostsync_handoff_t {
  uint32_t* pay_h = nullptr;   // host to device: the host produces, the block consumes
  uint32_t* pay_d = nullptr;   // device to host
  uint32_t* flag_h = nullptr;
  uint32_t* flag_d = nullptr;
  uint32_t blocks = 0, host_threads = 0, rounds = 0, lines = 0, host_budget_us = 0;
  uint64_t seed = 0;
  gm_hostsync_inj_t inj;
};

struct gm_hostsync_bad_word_t {
  uint64_t index;  // b << 20 | r << 14 | word; a flag: 1 << 40 | b << 6 | r
  uint32_t expected, got, dir;
};

// what one host thread saw of the device-to-host direction
struct gm_hostsync_host_stats_t {
  uint64_t handoffs = 0, observed = 0, unseen = 0, stale = 0;
  double poll_max_us = 0;
  std::vector<double> rtt_us;  // flag stored (step 1) to reply's flag seen (step 4)
  std::vector<gm_hostsync_bad_word_t> bad;  // the first few
};

inline size_t gm_hostsync_box_words(const gm_hostsync_handoff_t& c) {
  return (size_t)c.lines * GM_HOSTSYNC_LINE_WORDS;
}

// Host thread j serves the blocks b with b % host_threads == j: per round it first produces for
// each of them, then waits for each one's reply, so that no block waits for another's round trip.
inline void gm_hostsync_host_serve(const gm_hostsync_handoff_t& c, uint32_t j,
                                   gm_hostsync_host_stats_t* st) {
  const size_t box = gm_hostsync_box_words(c);
  std::vector<double> sent(c.blocks, 0.0);
  for (uint32_t r = 0; r < c.rounds; ++r) {
    for (uint32_t b = j; b < c.blocks; b += c.host_threads) {
      const size_t m = (size_t)b * c.rounds + r;
      uint32_t* dst = c.pay_h + m * box;
      for (uint32_t word = 0; word < box; ++word)
        dst[word] = gm_hostsync_payload(c.seed, 0, b, r, word);
      if (c.inj.on && c.inj.dir == 0 && b == c.inj.a && r == c.inj.b && c.inj.word < box)
        dst[c.inj.word] ^= c.inj.mask;
      sent[b] = gm_hostsync_now_us();
      __atomic_store_n(&c.flag_h[m * GM_HOSTSYNC_FLAG_WORDS], r + 1u, __ATOMIC_RELEASE);
    }
    for (uint32_t b = j; b < c.blocks; b += c.host_threads) {
      const size_t m = (size_t)b * c.rounds + r;
      const uint32_t* flag = &c.flag_d[m * GM_HOSTSYNC_FLAG_WORDS];
      const double t0 = gm_hostsync_now_us();
      double waited = 0;
      bool seen = false;
      for (;;) {
        waited = gm_hostsync_now_us() - t0;
        if (waited > (double)c.host_budget_us) break;
        if ((__atomic_load_n(flag, __ATOMIC_ACQUIRE) & 0xFFFFu) == r + 1u) {
          seen = true;
          break;
        }
      }
      ++st->handoffs;
      if (!seen) {
        ++st->unseen;
        continue;
      }
      ++st->observed;
      st->rtt_us.push_back(t0 + waited - sent[b]);
      if (waited > st->poll_max_us) st->poll_max_us = waited;
      const uint32_t* src = c.pay_d + m * box;
      for (uint32_t word = 0; word < box; ++word) {
        const uint32_t e = gm_hostsync_payload(c.seed, 1, b, r, word), got = src[word];
        if (got == e) continue;
        ++st->stale;
        if (st->bad.size() < 4)
          st->bad.push_back({((uint64_t)b << 20) | ((uint64_t)r << 14) | word, e, got, 1u});
      }
    }
  }
}

// After the join and the stream's end: every payload word and every flag of both directions
// must be there. Returns the words and flags that are not; the first few go to *bad. The
// producer's negative control is in the data, so it is counted here too, once.
inline uint64_t gm_hostsync_host_audit(const gm_hostsync_handoff_t& c,
                                       std::vector<gm_hostsync_bad_word_t>* bad) {
  const size_t box = gm_hostsync_box_words(c);
  uint64_t lost = 0;
  auto book = [&](uint64_t index, uint32_t e, uint32_t got, uint32_t dir) {
    ++lost;
    if (bad && bad->size() < 4) bad->push_back({index, e, got, dir});
  };
  for (uint32_t dir = 0; dir < 2; ++dir)
    for (uint32_t b = 0; b < c.blocks; ++b)
      for (uint32_t r = 0; r < c.rounds; ++r) {
        const size_t m = (size_t)b * c.rounds + r;
        const uint32_t* src = (dir ? c.pay_d : c.pay_h) + m * box;
        for (uint32_t word = 0; word < box; ++word) {
          const uint32_t e = gm_hostsync_payload(c.seed, dir, b, r, word);
          if (src[word] != e)
            book(((uint64_t)b << 20) | ((uint64_t)r << 14) | word, e, src[word], dir);
        }
        const uint32_t f = (dir ? c.flag_d : c.flag_h)[m * GM_HOSTSYNC_FLAG_WORDS] & 0xFFFFu;
        if (f != r + 1u) book((1ull << 40) | ((uint64_t)b << 6) | r, r + 1u, f, dir);
      }
  return lost;
}

inline double gm_hostsync_median(std::vector<double> v) {
  if (v.empty()) return 0.0;
  const size_t mid = v.size() / 2;
  std::nth_element(v.begin(), v.begin() + mid, v.end());
  return v[mid];
}
