// gm_atomics.hip — cross-XCC atomics and coherence test for gfx950: do the memory-side atomic
// units behind the eight private L2s lose or double an operation, is a ticket handed out twice,
// and does the documented agent-scope release/acquire hand-off deliver every word?
//
// Formulas and the contract are in gm_probe.h, the value functions and the host reference in
// gm_atomics_ref.h, the per-step operations in gm_atomics_steps.h (here at agent scope) and the
// hand-off's pieces in gm_atomics_dev.h. No kernel here waits without a bound on another block:
// the known-answer kernels (k_add, k_ticket) do not wait, k_cas bounds its retries by the host's
// count of operations into the word, and k_handoff polls for at most budget_us of wall_clock64()
// and books "not seen" as a legal outcome. So a call ends on any device state, blocks run one
// after another included. Every index is masked or checked against its table before it is used.
#include "gm_probe.h"

#include <string.h>

#include <vector>

#include "gm_atomics_dev.h"

namespace {

#define GM_AGENT __HIP_MEMORY_SCOPE_AGENT
typedef DevOps<GM_AGENT> Ops;
typedef gm_atomics_inj_t Inj;

// s_getreg immediate: (size - 1) << 11 | offset << 6 | register; XCC_ID[3:0] of register 20
constexpr int kGetXcc = ((4 - 1) << 11) | (0 << 6) | 20;

struct DevTab {
  unsigned long long words_bad[GM_ATOMICS_NKINDS];
  unsigned long long holes, duplicates, counter_errors, order_violations, out_of_range, giveups;
  unsigned long long handoffs, observed, cross, unseen, stale, lost, poll_sum, poll_max;
  uint32_t pairs_observed[256], pairs_stale[256], xcc_blocks[16];
  uint32_t claims, pad;
  gm_atomics_record_t rec[GM_ATOMICS_MAX_RECORDS];
};

// Cold: entered per error only.
__device__ __noinline__ void report(DevTab* tab, uint32_t test, uint32_t kind, uint64_t index,
                                    uint64_t e, uint64_t g, uint32_t xp, uint32_t xc) {
  const unsigned int slot = atomicAdd(&tab->claims, 1u);
  if (slot < GM_ATOMICS_MAX_RECORDS) {
    gm_atomics_record_t* r = &tab->rec[slot];
    r->index = index;
    r->expected = e;
    r->got = g;
    r->test = test;
    r->kind = kind;
    r->xcc_producer = xp;
    r->xcc_consumer = xc;
  }
}

__global__ __launch_bounds__(kThreads) void k_census(DevTab* tab) {
  if (threadIdx.x == 0) atomicAdd(&tab->xcc_blocks[__builtin_amdgcn_s_getreg(kGetXcc) & 15], 1u);
}

// ---- ADD: one no-return operation per step; width a power of two, so a(g, s) < width
__global__ __launch_bounds__(kThreads) void k_add(uint32_t kind, void* table, uint32_t width,
                                                  uint32_t iters, uint64_t seed, Inj inj) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s)
    gm_atomics_add_step<Ops>(kind, table, width, seed, inj, g, s);
}

// ---- compare after the kernel boundary: table against the host's, words of 4 or 8 bytes
__global__ __launch_bounds__(kThreads) void k_compare(const void* table, const void* expected,
                                                      uint32_t width, uint32_t wide, uint32_t test,
                                                      uint32_t kind, DevTab* tab) {
  for (uint32_t w = blockIdx.x * kThreads + threadIdx.x; w < width; w += gridDim.x * kThreads) {
    const uint64_t got = wide ? ((const uint64_t*)table)[w] : ((const uint32_t*)table)[w];
    const uint64_t e = wide ? ((const uint64_t*)expected)[w] : ((const uint32_t*)expected)[w];
    if (got != e) {
      atomicAdd(&tab->words_bad[kind], 1ull);
      report(tab, test, kind, w, e, got, GM_ATOMICS_XCC_UNKNOWN, GM_ATOMICS_XCC_UNKNOWN);
    }
  }
}

// ---- CAS: the step's loop, bounded by the host's count of operations into the word
__global__ __launch_bounds__(kThreads) void k_cas(uint64_t* table, const uint32_t* bound,
                                                  uint32_t width, uint32_t iters, uint64_t seed,
                                                  Inj inj, DevTab* tab) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s)
    if (!gm_atomics_cas_step<Ops>(table, bound, width, seed, inj, g, s)) {
      atomicAdd(&tab->giveups, 1ull);
      return;
    }
}

// ---- TICKET: returning fetch-add; off[k] .. off[k + 1] are counter k's marks
__global__ __launch_bounds__(kThreads) void k_ticket(uint32_t* ctr, const uint64_t* off,
                                                     uint32_t* marks, uint64_t n_marks,
                                                     uint32_t counters, uint32_t iters,
                                                     uint64_t seed, Inj inj, DevTab* tab) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  uint32_t last[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) last[i] = 0;
  for (uint32_t s = 0; s < iters; ++s) {
    uint32_t old, d;
    const uint32_t out_of_range = gm_atomics_ticket_step<Ops>(ctr, off, marks, n_marks, counters,
                                                              seed, inj, g, s, old, d);
    if (out_of_range) atomicAdd(&tab->out_of_range, (unsigned long long)out_of_range);
    if (counters <= 16) {  // slot s mod K is this counter's: the thread was here K draws ago
      const uint32_t slot = s & (counters - 1u);
      uint32_t prev = 0;
#pragma unroll  // constant indices keep last[] in registers
      for (uint32_t i = 0; i < 16; ++i)
        if (i == slot) {
          prev = last[i];
          last[i] = old + d;
        }
      if (s >= counters && old < prev) atomicAdd(&tab->order_violations, 1ull);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_ticket_audit(const uint32_t* ctr, const uint64_t* off,
                                                           const uint32_t* marks, uint64_t n_marks,
                                                           uint32_t counters, DevTab* tab) {
  const uint64_t first = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = first; i < n_marks; i += step) {
    const uint32_t m = marks[i];
    if (m == 1) continue;
    atomicAdd(m == 0 ? &tab->holes : &tab->duplicates, 1ull);
    report(tab, GM_ATOMICS_TICKET, GM_ATOMICS_K_TICKET, i, 1, m, GM_ATOMICS_XCC_UNKNOWN,
           GM_ATOMICS_XCC_UNKNOWN);
  }
  for (uint64_t k = first; k < counters; k += step) {
    const uint64_t n = off[k + 1] - off[k];
    if (ctr[k] != n) {
      atomicAdd(&tab->counter_errors, 1ull);
      report(tab, GM_ATOMICS_TICKET, GM_ATOMICS_K_TICKET, n_marks + k, n, ctr[k],
             GM_ATOMICS_XCC_UNKNOWN, GM_ATOMICS_XCC_UNKNOWN);
    }
  }
}

// ---- HANDOFF
struct HandoffArgs {
  uint32_t* payload;  // mailbox m = b * rounds + r at word m * lines * 1024
  uint32_t* flags;    // its flag at word m * 32
  uint64_t seed, budget_ticks;
  uint32_t rounds, lines;
  Inj inj;
};

__global__ __launch_bounds__(kThreads) void k_handoff(HandoffArgs a, DevTab* tab) {
  __shared__ uint32_t lds[2];  // seen, flag value
  const uint32_t t = threadIdx.x, b = blockIdx.x, G = gridDim.x;
  const uint32_t xcc = __builtin_amdgcn_s_getreg(kGetXcc) & 15u;
  const uint32_t box_words = a.lines * GM_ATOMICS_LINE_WORDS;
  for (uint32_t r = 0; r < a.rounds; ++r) {
    // 1. produce the own mailbox and release its flag at agent scope
    const uint32_t mine = b * a.rounds + r;
    const bool hit = gm_atomics_inj_hit(a.inj, b, r);
    store_box(a.payload + (size_t)mine * box_words, a.lines, [&](uint32_t word) {
      const uint32_t v = gm_atomics_payload(a.seed, b, r, word);
      return hit && word == a.inj.word ? v ^ a.inj.mask : v;
    });
    release_flag<GM_AGENT>(&a.flags[(size_t)mine * GM_ATOMICS_FLAG_WORDS], (xcc << 16) | (r + 1u));

    // 2. consume the partner's, L1-warm
    const uint32_t p = gm_atomics_partner(b, r, G);
    const uint32_t theirs = p * a.rounds + r;
    const uint32_t* src = a.payload + (size_t)theirs * box_words;
    warm_box(src, a.lines);
    if (t == 0) {
      const uint32_t* flag = &a.flags[(size_t)theirs * GM_ATOMICS_FLAG_WORDS];
      const uint64_t t0 = wall_clock64();
      uint32_t f, seen = 0;
      uint64_t waited;
      do {  // bounded by wall-clock time: the producer may not be resident
        f = __hip_atomic_load(flag, GM_RLX, GM_AGENT);
        waited = wall_clock64() - t0;
        if ((f & 0xFFFFu) == r + 1u) {
          seen = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      } while (waited < a.budget_ticks);
      lds[0] = seen;
      lds[1] = f;
      atomicAdd(&tab->handoffs, 1ull);
      if (seen) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed
        const uint32_t px = (f >> 16) & 15u;
        atomicAdd(&tab->observed, 1ull);
        if (px != xcc) atomicAdd(&tab->cross, 1ull);
        atomicAdd(&tab->pairs_observed[px * 16 + xcc], 1u);
        atomicAdd(&tab->poll_sum, (unsigned long long)waited);
        atomicMax(&tab->poll_max, (unsigned long long)waited);
      } else {
        atomicAdd(&tab->unseen, 1ull);
      }
    }
    __syncthreads();
    const uint32_t seen = lds[0], px = (lds[1] >> 16) & 15u;
    if (seen)
      compare_box(
          src, a.lines, [&](uint32_t word) { return gm_atomics_payload(a.seed, p, r, word); },
          [&](uint32_t word, uint32_t e, uint32_t got) {
            atomicAdd(&tab->stale, 1ull);
            atomicAdd(&tab->pairs_stale[px * 16 + xcc], 1u);
            report(tab, GM_ATOMICS_HANDOFF, GM_ATOMICS_K_HANDOFF, ((uint64_t)theirs << 14) | word,
                   e, got, px, xcc);
          });
    __syncthreads();  // lds[] is rewritten in the next round
  }
}

// one block per mailbox, after the launch: every word and every flag must be there
__global__ __launch_bounds__(kThreads) void k_handoff_audit(HandoffArgs a, DevTab* tab) {
  const uint32_t t = threadIdx.x, m = blockIdx.x;
  const uint32_t b = m / a.rounds, r = m % a.rounds;
  const uint32_t f = a.flags[(size_t)m * GM_ATOMICS_FLAG_WORDS];
  compare_box(
      a.payload + (size_t)m * a.lines * GM_ATOMICS_LINE_WORDS, a.lines,
      [&](uint32_t word) { return gm_atomics_payload(a.seed, b, r, word); },
      [&](uint32_t word, uint32_t e, uint32_t got) {
        atomicAdd(&tab->lost, 1ull);
        report(tab, GM_ATOMICS_HANDOFF, GM_ATOMICS_K_HANDOFF, ((uint64_t)m << 14) | word, e, got,
               (f >> 16) & 15u, GM_ATOMICS_XCC_UNKNOWN);
      });
  if (t == 0 && (f & 0xFFFFu) != r + 1u) {
    atomicAdd(&tab->lost, 1ull);
    report(tab, GM_ATOMICS_HANDOFF, GM_ATOMICS_K_HANDOFF, (1ull << 40) | m, r + 1u,
           f & 0xFFFFu, (f >> 16) & 15u, GM_ATOMICS_XCC_UNKNOWN);
  }
}

// ---------------------------------------------------------------------------------- host side
bool one_test(uint32_t t) {
  return t == GM_ATOMICS_ADD || t == GM_ATOMICS_TICKET || t == GM_ATOMICS_CAS ||
         t == GM_ATOMICS_HANDOFF;
}

bool handoff_ok(uint32_t blocks, uint32_t rounds, uint32_t lines, uint32_t budget_us) {
  if (blocks < 1 || blocks > GM_ATOMICS_MAX_BLOCKS || rounds < 1 ||
      rounds > GM_ATOMICS_MAX_ROUNDS || (lines != 1 && lines != 16) || budget_us < 1 ||
      budget_us > GM_ATOMICS_MAX_BUDGET_US)
    return false;
  const uint64_t bytes = (uint64_t)blocks * rounds * (lines * 4096ull + 128ull);
  return bytes <= GM_ATOMICS_MAX_MAILBOX_BYTES;
}

// an injection into `test` of a run with this geometry
bool inject_ok(const gm_atomics_inject_t* in, uint32_t test, uint32_t blocks, uint32_t iters,
               uint32_t rounds, uint32_t lines) {
  if (in->test != test) return false;
  if (test == GM_ATOMICS_HANDOFF)
    return in->a < blocks && in->b < rounds && in->word < lines * GM_ATOMICS_LINE_WORDS &&
           in->mask != 0;
  return inject_step_ok(in, test, blocks * (uint32_t)kThreads, iters, GM_ATOMICS_ADD_KINDS);
}

unsigned grid_for(uint64_t n) {
  const uint64_t b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

// The launches of each test on given buffers; the callers have checked every argument.
int launch_add(uint32_t kind, void* table, uint32_t width, uint32_t blocks, uint32_t iters,
               uint64_t seed, Inj inj, hipStream_t st, Events* ev) {
  const size_t bytes = (size_t)width * (gm_atomics_is64(kind) ? 8 : 4);
  GM_CHECK(hipMemsetAsync(table, (int)gm_atomics_init_byte(kind), bytes, st));
  if (ev) GM_CHECK(hipEventRecord(ev->e0, st));
  hipLaunchKernelGGL(k_add, dim3(blocks), dim3(kThreads), 0, st, kind, table, width, iters, seed,
                     inj);
  GM_CHECK(hipGetLastError());
  if (ev) GM_CHECK(hipEventRecord(ev->e1, st));
  return 0;
}

int launch_cas(void* table, const void* bounds, uint32_t width, uint32_t blocks, uint32_t iters,
               uint64_t seed, Inj inj, hipStream_t st, DevTab* tab, Events* ev) {
  GM_CHECK(hipMemsetAsync(table, 0, (size_t)width * 8, st));
  if (ev) GM_CHECK(hipEventRecord(ev->e0, st));
  hipLaunchKernelGGL(k_cas, dim3(blocks), dim3(kThreads), 0, st, (uint64_t*)table,
                     (const uint32_t*)bounds, width, iters, seed, inj, tab);
  GM_CHECK(hipGetLastError());
  if (ev) GM_CHECK(hipEventRecord(ev->e1, st));
  return 0;
}

int launch_ticket(void* ctr, const void* off, void* marks, uint64_t n_marks, uint32_t counters,
                  uint32_t blocks, uint32_t iters, uint64_t seed, Inj inj, hipStream_t st,
                  DevTab* tab, Events* ev) {
  GM_CHECK(hipMemsetAsync(ctr, 0, (size_t)counters * 4, st));
  GM_CHECK(hipMemsetAsync(marks, 0, (size_t)n_marks * 4, st));
  if (ev) GM_CHECK(hipEventRecord(ev->e0, st));
  hipLaunchKernelGGL(k_ticket, dim3(blocks), dim3(kThreads), 0, st, (uint32_t*)ctr,
                     (const uint64_t*)off, (uint32_t*)marks, n_marks, counters, iters, seed, inj,
                     tab);
  GM_CHECK(hipGetLastError());
  if (ev) GM_CHECK(hipEventRecord(ev->e1, st));
  hipLaunchKernelGGL(k_ticket_audit, dim3(grid_for(n_marks)), dim3(kThreads), 0, st,
                     (const uint32_t*)ctr, (const uint64_t*)off, (const uint32_t*)marks, n_marks,
                     counters, tab);
  return (int)hipGetLastError();
}

int launch_handoff(void* payload, void* flags, uint32_t blocks, uint32_t rounds, uint32_t lines,
                   uint64_t budget_ticks, uint64_t seed, Inj inj, hipStream_t st, DevTab* tab,
                   Events* ev) {
  const size_t boxes = (size_t)blocks * rounds;
  // failing data in every mailbox and no flag raised before the launch
  GM_CHECK(hipMemsetAsync(payload, 0xA5, boxes * lines * 4096, st));
  GM_CHECK(hipMemsetAsync(flags, 0, boxes * 128, st));
  HandoffArgs a{};
  a.payload = (uint32_t*)payload;
  a.flags = (uint32_t*)flags;
  a.seed = seed;
  a.budget_ticks = budget_ticks;
  a.rounds = rounds;
  a.lines = lines;
  a.inj = inj;
  if (ev) GM_CHECK(hipEventRecord(ev->e0, st));
  hipLaunchKernelGGL(k_handoff, dim3(blocks), dim3(kThreads), 0, st, a, tab);
  GM_CHECK(hipGetLastError());
  if (ev) GM_CHECK(hipEventRecord(ev->e1, st));
  hipLaunchKernelGGL(k_handoff_audit, dim3((unsigned)boxes), dim3(kThreads), 0, st, a, tab);
  return (int)hipGetLastError();
}

void fill_result(const DevTab& h, double ticks_per_us, gm_atomics_result_t* out) {
  for (int k = 0; k < GM_ATOMICS_NKINDS; ++k) {
    out->kinds[k].words_in_error = h.words_bad[k];
    out->words_in_error += h.words_bad[k];
  }
  out->holes = h.holes;
  out->duplicates = h.duplicates;
  out->counter_errors = h.counter_errors;
  out->order_violations = h.order_violations;
  out->out_of_range = h.out_of_range;
  out->cas_giveups = h.giveups;
  out->handoffs = h.handoffs;
  out->observed = h.observed;
  out->observed_cross_xcc = h.cross;
  out->unseen = h.unseen;
  out->stale_words = h.stale;
  out->lost_words = h.lost;
  if (h.observed && ticks_per_us > 0) {
    out->poll_max_us = h.poll_max / ticks_per_us;
    out->poll_mean_us = (double)h.poll_sum / (double)h.observed / ticks_per_us;
  }
  for (int i = 0; i < 256; ++i) {
    out->pairs_observed[i / 16][i % 16] = h.pairs_observed[i];
    out->pairs_stale[i / 16][i % 16] = h.pairs_stale[i];
  }
  for (int i = 0; i < 16; ++i) {
    out->xcc_blocks[i] = h.xcc_blocks[i];
    out->xccs_seen += h.xcc_blocks[i] != 0;
  }
  out->records_filled = h.claims < GM_ATOMICS_MAX_RECORDS ? h.claims : GM_ATOMICS_MAX_RECORDS;
  for (uint32_t i = 0; i < out->records_filled; ++i) out->records[i] = h.rec[i];
}

// the table's counters into the result, after the stream has drained
int read_result(Tab<DevTab>& tab, hipStream_t st, double ticks_per_us, gm_atomics_result_t* out) {
  if (int e = tab.read(st)) return e;
  fill_result(tab.host, ticks_per_us, out);
  return 0;
}

void set_kind(gm_atomics_kind_t* k, uint64_t ops, uint32_t width, double ms) {
  k->ops = ops;
  k->width = width;
  k->ms = ms;
  k->gops = ms > 0 ? ops / ms * 1e-6 : 0.0;
}

}  // namespace

extern "C" {

int gm_probe_atomics_expected(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t width,
                              uint64_t seed, void* out, uint64_t out_bytes) {
  if (!out || kind > GM_ATOMICS_K_COUNT || kind == GM_ATOMICS_K_HANDOFF ||
      !gm_atomics_geometry_ok(blocks, iters) || !gm_atomics_width_ok(kind, blocks, iters, width) ||
      out_bytes != (uint64_t)width * (gm_atomics_is64(kind) ? 8 : 4))
    return (int)hipErrorInvalidValue;
  gm_atomics_expected_host(kind, blocks, iters, width, seed, 0, 0, 0, out);
  return 0;
}

int gm_probe_atomics_widths(uint32_t blocks, uint32_t iters, uint32_t spread,
                            uint32_t widths[GM_ATOMICS_NKINDS], uint64_t caps[GM_ATOMICS_NKINDS],
                            uint64_t max_adds[GM_ATOMICS_NKINDS]) {
  if (!gm_atomics_geometry_ok(blocks, iters) || !gm_atomics_pow2(spread) ||
      spread > GM_ATOMICS_MAX_SPREAD)
    return (int)hipErrorInvalidValue;
  for (uint32_t k = 0; k < GM_ATOMICS_NKINDS; ++k) {
    const uint32_t w = k == GM_ATOMICS_K_HANDOFF ? 0 : gm_atomics_width(k, blocks, iters, spread);
    if (w == 0 && k != GM_ATOMICS_K_HANDOFF) return (int)hipErrorInvalidValue;
    if (widths) widths[k] = w;
    if (caps) caps[k] = gm_atomics_cap(k);
    if (max_adds) max_adds[k] = w ? gm_atomics_max_adds(blocks, iters, w) : 0;
  }
  return 0;
}

uint32_t gm_probe_atomics_payload(uint64_t seed, uint32_t block, uint32_t round, uint32_t word) {
  return gm_atomics_payload(seed, block & 4095u, round & 63u, word & 16383u);
}

int gm_probe_atomics_add(uint32_t kind, void* dev_table, uint32_t width, uint32_t blocks,
                         uint32_t iters, uint64_t seed, const gm_atomics_inject_t* inject,
                         void* stream) {
  if (kind >= GM_ATOMICS_ADD_KINDS || !dev_table ||
      ((uintptr_t)dev_table & (gm_atomics_is64(kind) ? 7 : 3)) ||
      !gm_atomics_geometry_ok(blocks, iters) || !gm_atomics_width_ok(kind, blocks, iters, width) ||
      (inject && (!inject_ok(inject, GM_ATOMICS_ADD, blocks, iters, 0, 0) || inject->kind != kind)))
    return (int)hipErrorInvalidValue;
  return launch_add(kind, dev_table, width, blocks, iters, seed,
                    inj_for(inject, GM_ATOMICS_ADD, kind), (hipStream_t)stream, nullptr);
}

int gm_probe_atomics_cas(void* dev_table, const void* dev_bounds, uint32_t width, uint32_t blocks,
                         uint32_t iters, uint64_t seed, const gm_atomics_inject_t* inject,
                         void* stream, gm_atomics_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!dev_table || ((uintptr_t)dev_table & 7) || !dev_bounds || ((uintptr_t)dev_bounds & 3) ||
      !gm_atomics_geometry_ok(blocks, iters) ||
      !gm_atomics_width_ok(GM_ATOMICS_K_CAS, blocks, iters, width) ||
      (inject && !inject_ok(inject, GM_ATOMICS_CAS, blocks, iters, 0, 0)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  Tab<DevTab> tab;
  if (int e = tab.create(st)) return e;
  if (int e = launch_cas(dev_table, dev_bounds, width, blocks, iters, seed,
                         inj_for(inject, GM_ATOMICS_CAS, 0), st, tab.dev(), nullptr))
    return e;
  return read_result(tab, st, 0, out);
}

int gm_probe_atomics_ticket(void* dev_ctr, const void* dev_off, void* dev_marks, uint64_t marks,
                            uint32_t counters, uint32_t blocks, uint32_t iters, uint64_t seed,
                            const gm_atomics_inject_t* inject, void* stream,
                            gm_atomics_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  // every draw takes 1 to 4 tickets
  const uint64_t ops = (uint64_t)blocks * kThreads * iters;
  if (!dev_ctr || ((uintptr_t)dev_ctr & 3) || !dev_off || ((uintptr_t)dev_off & 7) ||
      !dev_marks || ((uintptr_t)dev_marks & 3) || !gm_atomics_geometry_ok(blocks, iters) ||
      !gm_atomics_pow2(counters) || counters > GM_ATOMICS_MAX_SPREAD || marks < ops ||
      marks > 4 * ops || (inject && !inject_ok(inject, GM_ATOMICS_TICKET, blocks, iters, 0, 0)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  Tab<DevTab> tab;
  if (int e = tab.create(st)) return e;
  if (int e = launch_ticket(dev_ctr, dev_off, dev_marks, marks, counters, blocks, iters, seed,
                            inj_for(inject, GM_ATOMICS_TICKET, 0), st, tab.dev(), nullptr))
    return e;
  out->tickets = ops;
  return read_result(tab, st, 0, out);
}

int gm_probe_atomics_handoff(void* dev_payload, void* dev_flags, uint32_t blocks, uint32_t rounds,
                             uint32_t lines, uint32_t budget_us, uint64_t seed,
                             const gm_atomics_inject_t* inject, void* stream,
                             gm_atomics_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!dev_payload || ((uintptr_t)dev_payload & 15) || !dev_flags || ((uintptr_t)dev_flags & 127) ||
      !handoff_ok(blocks, rounds, lines, budget_us) ||
      (inject && !inject_ok(inject, GM_ATOMICS_HANDOFF, blocks, 0, rounds, lines)))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  double per_us = 0;
  uint64_t ticks = 0;
  if (int e = budget_ticks_of(budget_us, &per_us, &ticks)) return e;
  Tab<DevTab> tab;
  if (int e = tab.create(st)) return e;
  if (int e = launch_handoff(dev_payload, dev_flags, blocks, rounds, lines, ticks, seed,
                             inj_for(inject, GM_ATOMICS_HANDOFF, 0), st, tab.dev(), nullptr))
    return e;
  return read_result(tab, st, per_us, out);
}

int gm_probe_atomics(int dev, uint32_t tests_mask, uint32_t blocks, uint32_t iters,
                     uint32_t spread, uint32_t rounds, uint32_t lines, uint32_t budget_us,
                     uint64_t seed, const gm_atomics_inject_t* inject, gm_atomics_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  const uint32_t probe_blocks = blocks ? blocks : 1;  // what does not depend on the count
  if (dev < 0 || tests_mask == 0 || (tests_mask & ~(uint32_t)GM_ATOMICS_ALL) ||
      blocks > GM_ATOMICS_MAX_BLOCKS || !gm_atomics_geometry_ok(probe_blocks, iters) ||
      !gm_atomics_pow2(spread) || spread > GM_ATOMICS_MAX_SPREAD ||
      !handoff_ok(probe_blocks, rounds, lines, budget_us) ||
      (inject && (!one_test(inject->test) || !(inject->test & tests_mask))) ||
      (inject && blocks &&
       !inject_ok(inject, inject->test, blocks, iters, rounds, lines)))
    return (int)hipErrorInvalidValue;
  DeviceGuard guard(dev);
  if (!guard.ok) return (int)hipErrorInvalidDevice;
  const double t0 = now_s();
  if (blocks == 0) {
    int cus = 0;
    if (int e = current_cus(&cus)) return e;
    if (cus <= 0) return (int)hipErrorInvalidDevice;
    blocks = (uint32_t)cus > GM_ATOMICS_MAX_BLOCKS ? GM_ATOMICS_MAX_BLOCKS : (uint32_t)cus;
    if (!gm_atomics_geometry_ok(blocks, iters) || !handoff_ok(blocks, rounds, lines, budget_us) ||
        (inject && !inject_ok(inject, inject->test, blocks, iters, rounds, lines)))
      return (int)hipErrorInvalidValue;
  }
  uint32_t widths[GM_ATOMICS_NKINDS];
  if (int e = gm_probe_atomics_widths(blocks, iters, spread, widths, nullptr, nullptr)) return e;
  out->blocks = blocks;
  out->iters = iters;
  out->spread = spread;
  out->rounds = rounds;
  out->lines = lines;
  out->budget_us = budget_us;
  const uint64_t ops = (uint64_t)blocks * kThreads * iters;
  double per_us = 0;
  uint64_t ticks = 0;
  if (int e = budget_ticks_of(budget_us, &per_us, &ticks)) return e;

  hipStream_t st = nullptr;
  Tab<DevTab> tab;
  if (int e = tab.create(st)) return e;
  Events ev[GM_ATOMICS_NKINDS];
  bool timed[GM_ATOMICS_NKINDS] = {};
  hipLaunchKernelGGL(k_census, dim3(blocks), dim3(kThreads), 0, st, tab.dev());
  GM_CHECK(hipGetLastError());

  // a table and the host's expectation of it, compared after the kernel boundary
  auto checked_table = [&](uint32_t kind, DevBuf& table, DevBuf& dexp,
                           std::vector<unsigned char>& h_exp) -> int {
    const uint32_t w = widths[kind];
    const size_t bytes = (size_t)w * (gm_atomics_is64(kind) ? 8 : 4);
    h_exp.resize(bytes);
    // the expectation never holds the injection: an injected run must differ from it
    gm_atomics_expected_host(kind, blocks, iters, w, seed, 0, 0, 0, h_exp.data());
    GM_CHECK(table.alloc(bytes));
    GM_CHECK(dexp.alloc(bytes));
    GM_CHECK(hipMemcpy(dexp.p, h_exp.data(), bytes, hipMemcpyHostToDevice));
    GM_CHECK(ev[kind].create());
    return 0;
  };
  auto compare = [&](uint32_t test, uint32_t kind, const DevBuf& table, const DevBuf& dexp) -> int {
    hipLaunchKernelGGL(k_compare, dim3(grid_for(widths[kind])), dim3(kThreads), 0, st,
                       (const void*)table.p, (const void*)dexp.p, widths[kind],
                       (uint32_t)gm_atomics_is64(kind), test, kind, tab.dev());
    return (int)hipGetLastError();
  };

  if (tests_mask & GM_ATOMICS_ADD) {
    for (uint32_t kind = 0; kind < GM_ATOMICS_ADD_KINDS; ++kind) {
      DevBuf table, dexp;
      std::vector<unsigned char> h_exp;
      if (int e = checked_table(kind, table, dexp, h_exp)) return e;
      if (int e = launch_add(kind, table.p, widths[kind], blocks, iters, seed,
                             inj_for(inject, GM_ATOMICS_ADD, kind), st, &ev[kind]))
        return e;
      if (int e = compare(GM_ATOMICS_ADD, kind, table, dexp)) return e;
      GM_CHECK(hipStreamSynchronize(st));  // the buffers are freed at the end of this scope
      timed[kind] = true;
    }
    out->tests_run |= GM_ATOMICS_ADD;
  }
  if (tests_mask & GM_ATOMICS_TICKET) {
    const uint32_t kind = GM_ATOMICS_K_TICKET, K = widths[kind];
    std::vector<uint32_t> n(K);
    gm_atomics_expected_host(kind, blocks, iters, K, seed, 0, 0, 0, n.data());
    std::vector<uint64_t> off((size_t)K + 1, 0);
    for (uint32_t k = 0; k < K; ++k) off[k + 1] = off[k] + n[k];
    DevBuf ctr, doff, marks;
    GM_CHECK(ctr.alloc((size_t)K * 4));
    GM_CHECK(doff.alloc(off.size() * 8));
    GM_CHECK(marks.alloc((size_t)off[K] * 4));
    GM_CHECK(hipMemcpy(doff.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    GM_CHECK(ev[kind].create());
    if (int e = launch_ticket(ctr.p, doff.p, marks.p, off[K], K, blocks, iters, seed,
                              inj_for(inject, GM_ATOMICS_TICKET, 0), st, tab.dev(), &ev[kind]))
      return e;
    GM_CHECK(hipStreamSynchronize(st));
    timed[kind] = true;
    out->tickets = ops;
    out->tests_run |= GM_ATOMICS_TICKET;
  }
  if (tests_mask & GM_ATOMICS_CAS) {
    const uint32_t kind = GM_ATOMICS_K_CAS, w = widths[kind];
    DevBuf table, dexp, bounds;
    std::vector<unsigned char> h_exp;
    if (int e = checked_table(kind, table, dexp, h_exp)) return e;
    std::vector<uint32_t> count;
    gm_atomics_counts(blocks, iters, w, count);
    GM_CHECK(bounds.alloc((size_t)w * 4));
    GM_CHECK(hipMemcpy(bounds.p, count.data(), (size_t)w * 4, hipMemcpyHostToDevice));
    if (int e = launch_cas(table.p, bounds.p, w, blocks, iters, seed,
                           inj_for(inject, GM_ATOMICS_CAS, 0), st, tab.dev(), &ev[kind]))
      return e;
    if (int e = compare(GM_ATOMICS_CAS, kind, table, dexp)) return e;
    GM_CHECK(hipStreamSynchronize(st));
    timed[kind] = true;
    out->tests_run |= GM_ATOMICS_CAS;
  }
  if (tests_mask & GM_ATOMICS_HANDOFF) {
    const uint32_t kind = GM_ATOMICS_K_HANDOFF;
    const size_t boxes = (size_t)blocks * rounds;
    DevBuf payload, flags;
    GM_CHECK(payload.alloc(boxes * lines * 4096));
    GM_CHECK(flags.alloc(boxes * 128));
    GM_CHECK(ev[kind].create());
    if (int e = launch_handoff(payload.p, flags.p, blocks, rounds, lines, ticks, seed,
                               inj_for(inject, GM_ATOMICS_HANDOFF, 0), st, tab.dev(), &ev[kind]))
      return e;
    GM_CHECK(hipStreamSynchronize(st));
    timed[kind] = true;
    out->tests_run |= GM_ATOMICS_HANDOFF;
  }

  if (int e = read_result(tab, st, per_us, out)) return e;
  for (uint32_t k = 0; k < GM_ATOMICS_NKINDS; ++k)
    if (timed[k]) {
      float ms = 0;  // a pair that cannot be read books no time; the counts stand
      (void)elapsed_ms(ev[k].e0, ev[k].e1, &ms);
      set_kind(&out->kinds[k], k == GM_ATOMICS_K_HANDOFF ? (uint64_t)blocks * rounds : ops,
               k == GM_ATOMICS_K_HANDOFF ? blocks * rounds : widths[k], ms);
    }
  out->seconds = now_s() - t0;
  return 0;
}

}  // extern "C"
