// gm_hostsync.hip — host-GPU atomics and hand-off test for gfx950: do system-scope atomics on
// pinned host memory (PCIe AtomicOps) lose or double an operation while host threads work on the
// same words, and does a release/acquire hand-off through a flag in host memory deliver every
// payload word, in both directions, while the kernel runs?
//
// Formulas and the contract are in gm_probe.h, the value functions and audits in
// gm_hostsync_ref.h, the host threads' side in gm_hostsync_host.h, the per-step operations in
// gm_atomics_steps.h (here at system scope) and the hand-off's pieces in gm_atomics_dev.h. Every
// shared word lies in PinnedBuf memory (mapped, coherent) and the kernels reach it through
// hipHostGetDevicePointer. No kernel and no host thread waits without a bound: the known-answer
// kernels do not wait, the CAS loops are bounded by the host's count of operations into the word,
// the kernel's flag poll by budget_us of wall_clock64(), the host's by host_budget_us, and a host
// thread's start by GM_HOSTSYNC_START_BOUND_US. Every index is masked or checked against its
// table before use.
#include "gm_probe.h"

#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "gm_atomics_dev.h"
#include "gm_hostsync_host.h"

namespace {

#define GM_SYS __HIP_MEMORY_SCOPE_SYSTEM
typedef DevOps<GM_SYS> Ops;
typedef gm_atomics_inj_t Inj;

// the kernels' own counters, in device memory: nothing the host threads touch
struct DevTab {
  unsigned long long out_of_range, giveups, handoffs, observed, unseen, stale, poll_max;
  uint32_t claims, pad;
  gm_hostsync_record_t rec[GM_HOSTSYNC_MAX_RECORDS];
};

__device__ __forceinline__ void announce(uint32_t* ready) {
  if (threadIdx.x == 0) __hip_atomic_store(ready, 1u, GM_RLX, GM_SYS);
}

// ---- ADD: one no-return operation per step; width a power of two, so a(g, s) < width
__global__ __launch_bounds__(kThreads) void k_add(uint32_t kind, void* table, uint32_t width,
                                                  uint32_t iters, uint64_t seed, Inj inj,
                                                  uint32_t* ready) {
  announce(ready);
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s)
    gm_atomics_add_step<Ops>(kind, table, width, seed, inj, g, s);
}

// ---- TICKET: returning fetch-add; off[k] .. off[k + 1] are counter k's marks
__global__ __launch_bounds__(kThreads) void k_ticket(uint32_t* ctr, const uint64_t* off,
                                                     uint32_t* marks, uint64_t n_marks,
                                                     uint32_t counters, uint32_t iters,
                                                     uint64_t seed, Inj inj, uint32_t* ready,
                                                     DevTab* tab) {
  announce(ready);
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s) {
    uint32_t old, d;
    const uint32_t out_of_range = gm_atomics_ticket_step<Ops>(ctr, off, marks, n_marks, counters,
                                                              seed, inj, g, s, old, d);
    if (out_of_range) atomicAdd(&tab->out_of_range, (unsigned long long)out_of_range);
  }
}

// ---- SWAP: returned[] is the launch's own, blocks * 256 * iters words in device memory
__global__ __launch_bounds__(kThreads) void k_swap(uint32_t* words, uint32_t width, uint32_t iters,
                                                   Inj inj, uint32_t* ready, uint32_t* returned) {
  announce(ready);
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s)
    returned[(size_t)g * iters + s] = gm_hostsync_swap_step<Ops>(words, width, inj, g, s);
}

// ---- CAS: the step's loop, bounded by the count of operations into the word, GPU's and host's
__global__ __launch_bounds__(kThreads) void k_cas(uint64_t* table, const uint32_t* bound,
                                                  uint32_t width, uint32_t iters, uint64_t seed,
                                                  Inj inj, uint32_t* ready, DevTab* tab) {
  announce(ready);
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t s = 0; s < iters; ++s)
    if (!gm_atomics_cas_step<Ops>(table, bound, width, seed, inj, g, s)) {
      atomicAdd(&tab->giveups, 1ull);
      return;
    }
}

// ---- HANDOFF: mailbox m = b * rounds + r of either direction at word m * lines * 1024, its
// flag at word m * 32; all four arrays in host memory
struct HandoffArgs {
  uint32_t *pay_h, *pay_d, *flag_h, *flag_d, *ready;
  uint64_t seed, budget_ticks;
  uint32_t rounds, lines;
  Inj inj;
};

__global__ __launch_bounds__(kThreads) void k_handoff(HandoffArgs a, DevTab* tab) {
  __shared__ uint32_t lds[1];  // seen
  announce(a.ready);
  const uint32_t t = threadIdx.x, b = blockIdx.x;
  const uint32_t box_words = a.lines * GM_HOSTSYNC_LINE_WORDS;
  for (uint32_t r = 0; r < a.rounds; ++r) {
    const size_t m = (size_t)b * a.rounds + r;
    // 2. consume the host's, L1-warm
    const uint32_t* src = a.pay_h + m * box_words;
    warm_box(src, a.lines);
    if (t == 0) {
      const uint32_t* flag = &a.flag_h[m * GM_HOSTSYNC_FLAG_WORDS];
      const uint64_t t0 = wall_clock64();
      uint32_t seen = 0;
      uint64_t waited;
      for (;;) {  // bounded by wall-clock time: the host thread may be descheduled
        waited = wall_clock64() - t0;
        if (waited > a.budget_ticks) break;
        if (__hip_atomic_load(flag, GM_RLX, GM_SYS) == r + 1u) {
          seen = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      lds[0] = seen;
      atomicAdd(&tab->handoffs, 1ull);
      if (seen) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed
        atomicAdd(&tab->observed, 1ull);
        atomicMax(&tab->poll_max, (unsigned long long)waited);
      } else {
        atomicAdd(&tab->unseen, 1ull);
      }
    }
    __syncthreads();
    const uint32_t seen = lds[0];
    if (seen)
      compare_box(
          src, a.lines, [&](uint32_t word) { return gm_hostsync_payload(a.seed, 0, b, r, word); },
          [&](uint32_t word, uint32_t e, uint32_t got) {
            atomicAdd(&tab->stale, 1ull);
            const unsigned int slot = atomicAdd(&tab->claims, 1u);
            if (slot < GM_HOSTSYNC_MAX_RECORDS) {
              gm_hostsync_record_t* rec = &tab->rec[slot];
              rec->index = ((uint64_t)b << 20) | ((uint64_t)r << 14) | word;
              rec->expected = e;
              rec->got = got;
              rec->test = GM_HOSTSYNC_HANDOFF;
              rec->kind = 0;  // host to device
              rec->where = GM_HOSTSYNC_WHERE_STALE;
              rec->pad = 0;
            }
          });
    // 3. produce the reply and release its flag at system scope
    const bool hit = a.inj.dir == 1 && gm_atomics_inj_hit(a.inj, b, r);
    store_box(a.pay_d + m * box_words, a.lines, [&](uint32_t word) {
      const uint32_t v = gm_hostsync_payload(a.seed, 1, b, r, word);
      return hit && word == a.inj.word ? v ^ a.inj.mask : v;
    });
    release_flag<GM_SYS>(&a.flag_d[m * GM_HOSTSYNC_FLAG_WORDS], (seen << 16) | (r + 1u));
    __syncthreads();  // lds[] is rewritten in the next round
  }
}

// ---------------------------------------------------------------------------------- host side
bool one_test(uint32_t t) {
  return t == GM_HOSTSYNC_ADD || t == GM_HOSTSYNC_TICKET || t == GM_HOSTSYNC_SWAP ||
         t == GM_HOSTSYNC_CAS || t == GM_HOSTSYNC_HANDOFF;
}

// an injection into `test` of a run with this geometry
bool inject_ok(const gm_hostsync_inject_t* in, uint32_t test, uint32_t blocks,
               uint32_t host_threads, uint32_t iters, uint32_t rounds, uint32_t lines) {
  if (in->test != test) return false;
  if (test == GM_HOSTSYNC_HANDOFF)
    return in->kind < 2 && in->a < blocks && in->b < rounds &&
           in->word < lines * GM_HOSTSYNC_LINE_WORDS && in->mask != 0;
  return inject_step_ok(in, test, (blocks + host_threads) * (uint32_t)kThreads, iters, Ops::kKinds);
}

void add_record(gm_hostsync_result_t* out, uint32_t test, uint32_t kind, uint64_t index,
                uint64_t e, uint64_t got, uint32_t where) {
  if (out->records_filled >= GM_HOSTSYNC_MAX_RECORDS) return;
  gm_hostsync_record_t* r = &out->records[out->records_filled++];
  r->index = index;
  r->expected = e;
  r->got = got;
  r->test = test;
  r->kind = kind;
  r->where = where;
  r->pad = 0;
}

// zeroed pinned host memory and the address the kernels use for it
struct Shared {
  PinnedBuf buf;
  void* dev = nullptr;
  int create(size_t bytes, int fill = 0) {
    GM_CHECK(buf.alloc(bytes));
    memset(buf.p, fill, bytes);
    GM_CHECK(hipHostGetDevicePointer(&dev, buf.p, 0));
    return dev ? 0 : (int)hipErrorInvalidValue;
  }
};

// the host threads of one launch, joined on every return path
struct Crew {
  std::vector<std::thread> threads;
  gm_hostsync_gate_t gate;
  void join() {
    for (std::thread& t : threads)
      if (t.joinable()) t.join();
  }
  ~Crew() {
    __atomic_store_n(&gate.abort, 1u, __ATOMIC_RELEASE);
    join();
  }
};

// One launch with host_threads host threads at work beside it: the threads start when the kernel
// has stored `ready` (or after the start bound), `work(j, gate)` returns the operations thread j
// made while the kernel's end event was still hipErrorNotReady. Returns after the join and the
// stream's end.
template <class Launch, class Work>
int contend(hipStream_t st, uint32_t host_threads, Shared& ready, Launch launch, Work work,
            uint64_t* in_flight, double* ms) {
  Event end;
  GM_CHECK(end.create());
  std::vector<uint64_t> made(host_threads, 0);
  Crew crew;
  crew.gate.ready = (const uint32_t*)ready.buf.p;
  for (uint32_t j = 0; j < host_threads; ++j)
    crew.threads.emplace_back([&crew, &made, &work, j] {
      if (gm_hostsync_wait_start(&crew.gate)) made[j] = work(j, &crew.gate);
    });
  const double t0 = now_s();
  int e = launch();
  if (!e) e = (int)hipEventRecord(end.e, st);
  if (e) return e;  // ~Crew calls the threads off
  hipError_t q;
  while ((q = hipEventQuery(end.e)) == hipErrorNotReady) std::this_thread::yield();
  (void)hipGetLastError();  // hipErrorNotReady is no error of the call
  __atomic_store_n(&crew.gate.done, 1u, __ATOMIC_RELEASE);
  crew.join();
  if (ms) *ms = (now_s() - t0) * 1e3;
  if (q != hipSuccess) return (int)q;
  GM_CHECK(hipStreamSynchronize(st));
  for (uint64_t v : made) *in_flight += v;
  return 0;
}

struct Ctx {
  hipStream_t st;
  uint32_t blocks, host_threads, iters;
  uint64_t seed;
  const gm_hostsync_inject_t* inject;
  gm_hostsync_result_t* out;
  uint32_t total() const { return blocks + host_threads; }
  uint64_t ops() const { return (uint64_t)total() * kThreads * iters; }
};

// ADD of one kind (0 u32, 1 u64) into a fresh table of `width` words; table_out (may be NULL)
// takes the final table
int run_add(const Ctx& c, uint32_t kind, uint32_t width, void* table_out) {
  const bool wide = kind == GM_ATOMICS_K_ADD_U64;
  const size_t bytes = (size_t)width * (wide ? 8 : 4);
  const Inj inj = inj_for(c.inject, GM_HOSTSYNC_ADD, kind);
  Shared table, ready;
  if (int e = table.create(bytes)) return e;
  if (int e = ready.create(128)) return e;
  double ms = 0;
  if (int e = contend(
          c.st, c.host_threads, ready,
          [&]() -> int {
            hipLaunchKernelGGL(k_add, dim3(c.blocks), dim3(kThreads), 0, c.st, kind, table.dev,
                               width, c.iters, c.seed, inj, (uint32_t*)ready.dev);
            return (int)hipGetLastError();
          },
          [&](uint32_t j, const gm_hostsync_gate_t* gate) {
            return gm_hostsync_host_add(kind, table.buf.p, width, c.blocks + j, c.iters, c.seed,
                                        inj, gate);
          },
          &c.out->host_ops_in_flight, &ms))
    return e;
  c.out->ms[0] += ms;
  // the expectation never holds the injection: an injected run must differ from it
  std::vector<unsigned char> exp(bytes);
  gm_atomics_expected_host(kind, c.total(), c.iters, width, c.seed, 0, 0, 0, exp.data());
  uint64_t bad = 0;
  for (uint32_t w = 0; w < width; ++w) {
    const uint64_t got =
        wide ? ((const uint64_t*)table.buf.p)[w] : ((const uint32_t*)table.buf.p)[w];
    const uint64_t e = wide ? ((const uint64_t*)exp.data())[w] : ((const uint32_t*)exp.data())[w];
    if (got == e) continue;
    ++bad;
    add_record(c.out, GM_HOSTSYNC_ADD, kind, w, e, got, 0);
  }
  (wide ? c.out->add_u64_errors : c.out->add_u32_errors) += bad;
  c.out->words_in_error += bad;
  if (table_out) memcpy(table_out, table.buf.p, bytes);
  return 0;
}

int run_ticket(const Ctx& c, uint32_t counters) {
  const Inj inj = inj_for(c.inject, GM_HOSTSYNC_TICKET, 0);
  std::vector<uint32_t> n(counters);
  gm_atomics_expected_host(GM_ATOMICS_K_TICKET, c.total(), c.iters, counters, c.seed, 0, 0, 0,
                           n.data());
  std::vector<uint64_t> off((size_t)counters + 1, 0);
  for (uint32_t k = 0; k < counters; ++k) off[k + 1] = off[k] + n[k];
  const uint64_t n_marks = off[counters];
  Shared ctr, marks, ready;
  DevBuf doff;
  Tab<DevTab> tab;
  if (int e = ctr.create((size_t)counters * 4)) return e;
  if (int e = marks.create((size_t)n_marks * 4)) return e;
  if (int e = ready.create(128)) return e;
  GM_CHECK(doff.alloc(off.size() * 8));
  GM_CHECK(hipMemcpy(doff.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  if (int e = tab.create(c.st)) return e;
  std::vector<uint64_t> oor(c.host_threads, 0);
  double ms = 0;
  if (int e = contend(
          c.st, c.host_threads, ready,
          [&]() -> int {
            hipLaunchKernelGGL(k_ticket, dim3(c.blocks), dim3(kThreads), 0, c.st,
                               (uint32_t*)ctr.dev, (const uint64_t*)doff.p, (uint32_t*)marks.dev,
                               n_marks, counters, c.iters, c.seed, inj, (uint32_t*)ready.dev,
                               tab.dev());
            return (int)hipGetLastError();
          },
          [&](uint32_t j, const gm_hostsync_gate_t* gate) {
            return gm_hostsync_host_ticket((uint32_t*)ctr.buf.p, off.data(),
                                           (uint32_t*)marks.buf.p, n_marks, counters,
                                           c.blocks + j, c.iters, c.seed, inj, gate, &oor[j]);
          },
          &c.out->host_ops_in_flight, &ms))
    return e;
  c.out->ms[1] += ms;
  if (int e = tab.read(c.st)) return e;
  const gm_hostsync_ticket_audit_t a = gm_hostsync_ticket_audit(
      (const uint32_t*)ctr.buf.p, n.data(), counters, (const uint32_t*)marks.buf.p, n_marks);
  c.out->tickets = c.ops();
  c.out->holes += a.holes;
  c.out->duplicates += a.duplicates;
  c.out->counter_errors += a.counter_errors;
  c.out->out_of_range += tab.host.out_of_range;
  for (uint64_t v : oor) c.out->out_of_range += v;
  if (a.first_index != ~0ull)
    add_record(c.out, GM_HOSTSYNC_TICKET, 0, a.first_index, a.first_expected, a.first_got, 0);
  return 0;
}

int run_swap(const Ctx& c, uint32_t width) {
  const Inj inj = inj_for(c.inject, GM_HOSTSYNC_SWAP, 0);
  const size_t gpu_ops = (size_t)c.blocks * kThreads * c.iters;
  const size_t per_thread = (size_t)kThreads * c.iters;
  Shared words, ready;
  DevBuf dret;
  if (int e = words.create((size_t)width * 4)) return e;
  if (int e = ready.create(128)) return e;
  GM_CHECK(dret.alloc(gpu_ops * 4));
  GM_CHECK(hipMemsetAsync(dret.p, 0xFF, gpu_ops * 4, c.st));  // no token: a skipped one shows
  std::vector<uint32_t> returned((size_t)c.ops(), 0xFFFFFFFFu);
  double ms = 0;
  if (int e = contend(
          c.st, c.host_threads, ready,
          [&]() -> int {
            hipLaunchKernelGGL(k_swap, dim3(c.blocks), dim3(kThreads), 0, c.st,
                               (uint32_t*)words.dev, width, c.iters, inj, (uint32_t*)ready.dev,
                               (uint32_t*)dret.p);
            return (int)hipGetLastError();
          },
          [&](uint32_t j, const gm_hostsync_gate_t* gate) {
            return gm_hostsync_host_swap((uint32_t*)words.buf.p, width, c.blocks + j, c.iters, inj,
                                         gate, returned.data() + gpu_ops + j * per_thread);
          },
          &c.out->host_ops_in_flight, &ms))
    return e;
  c.out->ms[2] += ms;
  GM_CHECK(hipMemcpy(returned.data(), dret.p, gpu_ops * 4, hipMemcpyDeviceToHost));
  const gm_hostsync_swap_audit_t a = gm_hostsync_swap_audit(
      c.total(), c.iters, width, returned.data(), (const uint32_t*)words.buf.p);
  c.out->swaps = c.ops();
  c.out->swap_missing += a.missing;
  c.out->swap_duplicates += a.duplicates;
  c.out->swap_foreign += a.foreign;
  if (a.first_bad_word != ~0ull)
    add_record(c.out, GM_HOSTSYNC_SWAP, 0, a.first_bad_word, 0, a.first_bad_value, 0);
  return 0;
}

// CAS into a fresh table of `width` words, already widened; table_out may be NULL
int run_cas(const Ctx& c, uint32_t width, void* table_out) {
  const Inj inj = inj_for(c.inject, GM_HOSTSYNC_CAS, 0);
  const size_t bytes = (size_t)width * 8;
  std::vector<uint32_t> count;
  gm_atomics_counts(c.total(), c.iters, width, count);
  Shared table, ready;
  DevBuf bounds;
  Tab<DevTab> tab;
  if (int e = table.create(bytes)) return e;
  if (int e = ready.create(128)) return e;
  GM_CHECK(bounds.alloc((size_t)width * 4));
  GM_CHECK(hipMemcpy(bounds.p, count.data(), (size_t)width * 4, hipMemcpyHostToDevice));
  if (int e = tab.create(c.st)) return e;
  std::vector<uint64_t> gave(c.host_threads, 0);
  double ms = 0;
  if (int e = contend(
          c.st, c.host_threads, ready,
          [&]() -> int {
            hipLaunchKernelGGL(k_cas, dim3(c.blocks), dim3(kThreads), 0, c.st,
                               (uint64_t*)table.dev, (const uint32_t*)bounds.p, width, c.iters,
                               c.seed, inj, (uint32_t*)ready.dev, tab.dev());
            return (int)hipGetLastError();
          },
          [&](uint32_t j, const gm_hostsync_gate_t* gate) {
            return gm_hostsync_host_cas((uint64_t*)table.buf.p, count.data(), width, c.blocks + j,
                                        c.iters, c.seed, inj, gate, &gave[j]);
          },
          &c.out->host_ops_in_flight, &ms))
    return e;
  c.out->ms[3] += ms;
  if (int e = tab.read(c.st)) return e;
  c.out->cas_giveups += tab.host.giveups;
  for (uint64_t v : gave) c.out->cas_giveups += v;
  c.out->cas_width = width;
  std::vector<uint64_t> exp(width);
  gm_atomics_expected_host(GM_ATOMICS_K_CAS, c.total(), c.iters, width, c.seed, 0, 0, 0,
                           exp.data());
  const uint64_t* got = (const uint64_t*)table.buf.p;
  for (uint32_t w = 0; w < width; ++w) {
    if (got[w] == exp[w]) continue;
    ++c.out->cas_errors;
    ++c.out->words_in_error;
    add_record(c.out, GM_HOSTSYNC_CAS, 0, w, exp[w], got[w], 0);
  }
  if (table_out) memcpy(table_out, table.buf.p, bytes);
  return 0;
}

int run_handoff(const Ctx& c, uint32_t rounds, uint32_t lines, uint32_t budget_us,
                uint32_t host_budget_us) {
  const Inj inj = inj_for(c.inject, GM_HOSTSYNC_HANDOFF, 0, true);
  const size_t boxes = (size_t)c.blocks * rounds;
  double per_us = 0;
  uint64_t ticks = 0;
  if (int e = budget_ticks_of(budget_us, &per_us, &ticks)) return e;
  Shared pay_h, pay_d, flag_h, flag_d, ready;
  Tab<DevTab> tab;
  // failing data in every mailbox and no flag raised before the launch
  if (int e = pay_h.create(boxes * lines * 4096, 0xA5)) return e;
  if (int e = pay_d.create(boxes * lines * 4096, 0xA5)) return e;
  if (int e = flag_h.create(boxes * 128)) return e;
  if (int e = flag_d.create(boxes * 128)) return e;
  if (int e = ready.create(128)) return e;
  if (int e = tab.create(c.st)) return e;
  gm_hostsync_handoff_t h;
  h.pay_h = (uint32_t*)pay_h.buf.p;
  h.pay_d = (uint32_t*)pay_d.buf.p;
  h.flag_h = (uint32_t*)flag_h.buf.p;
  h.flag_d = (uint32_t*)flag_d.buf.p;
  h.blocks = c.blocks;
  h.host_threads = c.host_threads;
  h.rounds = rounds;
  h.lines = lines;
  h.host_budget_us = host_budget_us;
  h.seed = c.seed;
  h.inj = inj;
  HandoffArgs a{};
  a.pay_h = (uint32_t*)pay_h.dev;
  a.pay_d = (uint32_t*)pay_d.dev;
  a.flag_h = (uint32_t*)flag_h.dev;
  a.flag_d = (uint32_t*)flag_d.dev;
  a.ready = (uint32_t*)ready.dev;
  a.seed = c.seed;
  a.budget_ticks = ticks;
  a.rounds = rounds;
  a.lines = lines;
  a.inj = inj;
  std::vector<gm_hostsync_host_stats_t> stats(c.host_threads);
  uint64_t unused = 0;
  double ms = 0;
  if (int e = contend(
          c.st, c.host_threads, ready,
          [&]() -> int {
            hipLaunchKernelGGL(k_handoff, dim3(c.blocks), dim3(kThreads), 0, c.st, a, tab.dev());
            return (int)hipGetLastError();
          },
          [&](uint32_t j, const gm_hostsync_gate_t*) {
            gm_hostsync_host_serve(h, j, &stats[j]);
            return (uint64_t)0;
          },
          &unused, &ms))
    return e;
  c.out->ms[4] += ms;
  if (int e = tab.read(c.st)) return e;
  gm_hostsync_dir_t* h2d = &c.out->dir[0];
  gm_hostsync_dir_t* d2h = &c.out->dir[1];
  h2d->handoffs = tab.host.handoffs;
  h2d->observed = tab.host.observed;
  h2d->unseen = tab.host.unseen;
  h2d->stale_words = tab.host.stale;
  h2d->poll_max_us = tab.host.poll_max / per_us;
  const uint32_t filled =
      tab.host.claims < GM_HOSTSYNC_MAX_RECORDS ? tab.host.claims : GM_HOSTSYNC_MAX_RECORDS;
  for (uint32_t i = 0; i < filled; ++i) {
    const gm_hostsync_record_t& r = tab.host.rec[i];
    add_record(c.out, r.test, r.kind, r.index, r.expected, r.got, r.where);
  }
  std::vector<double> rtt;
  for (const gm_hostsync_host_stats_t& s : stats) {
    d2h->handoffs += s.handoffs;
    d2h->observed += s.observed;
    d2h->unseen += s.unseen;
    d2h->stale_words += s.stale;
    if (s.poll_max_us > d2h->poll_max_us) d2h->poll_max_us = s.poll_max_us;
    rtt.insert(rtt.end(), s.rtt_us.begin(), s.rtt_us.end());
    for (const gm_hostsync_bad_word_t& w : s.bad)
      add_record(c.out, GM_HOSTSYNC_HANDOFF, w.dir, w.index, w.expected, w.got,
                 GM_HOSTSYNC_WHERE_STALE);
  }
  // a host thread that started late (the start bound) may have left hand-offs unserved
  d2h->unseen += boxes - d2h->handoffs;
  d2h->handoffs = boxes;
  if (!rtt.empty()) {
    c.out->rtt_median_us = gm_hostsync_median(rtt);
    c.out->rtt_max_us = *std::max_element(rtt.begin(), rtt.end());
  }
  std::vector<gm_hostsync_bad_word_t> lost;
  c.out->lost_words += gm_hostsync_host_audit(h, &lost);
  for (const gm_hostsync_bad_word_t& w : lost)
    add_record(c.out, GM_HOSTSYNC_HANDOFF, w.dir, w.index, w.expected, w.got,
               GM_HOSTSYNC_WHERE_LOST);
  return 0;
}

// the per-test entry points' frame: arguments checked by the caller; blocks against the device
int begin(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint64_t seed,
          const gm_hostsync_inject_t* inject, void* stream, gm_hostsync_result_t* out, Ctx* c) {
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  if (cus <= 0) return (int)hipErrorInvalidDevice;
  if (blocks > (uint32_t)cus) return (int)hipErrorInvalidValue;
  int dev = 0, native = 0;
  GM_CHECK(hipGetDevice(&dev));
  GM_CHECK(hipDeviceGetAttribute(&native, hipDeviceAttributeHostNativeAtomicSupported, dev));
  out->atomics_supported = native != 0;
  out->blocks = blocks;
  out->host_threads = host_threads;
  out->iters = iters;
  *c = Ctx{(hipStream_t)stream, blocks, host_threads, iters, seed, inject, out};
  return 0;
}

bool table_ok(uint32_t kind, uint32_t blocks, uint32_t host_threads, uint32_t iters,
              uint32_t width) {
  return gm_hostsync_geometry_ok(blocks, host_threads, iters) &&
         gm_atomics_width_ok(kind, blocks + host_threads, iters, width) &&
         width <= (kind == GM_ATOMICS_K_CAS ? GM_ATOMICS_MAX_WIDTH : GM_HOSTSYNC_MAX_SPREAD);
}

}  // namespace

extern "C" {

int gm_probe_hostsync_expected(uint32_t kind, uint32_t blocks, uint32_t host_threads,
                               uint32_t iters, uint32_t width, uint64_t seed, void* out,
                               uint64_t out_bytes) {
  const bool known = kind == GM_ATOMICS_K_ADD_U32 || kind == GM_ATOMICS_K_ADD_U64 ||
                     kind == GM_ATOMICS_K_TICKET || kind == GM_ATOMICS_K_CAS ||
                     kind == GM_ATOMICS_K_COUNT || kind == GM_HOSTSYNC_K_SWAP;
  if (!out || !known || !gm_hostsync_geometry_ok(blocks, host_threads, iters) ||
      !gm_atomics_pow2(width) || width > GM_ATOMICS_MAX_WIDTH)
    return (int)hipErrorInvalidValue;
  const uint32_t total = blocks + host_threads;
  if (kind == GM_HOSTSYNC_K_SWAP) {  // per operation g * iters + s: word << 32 | token
    const uint64_t ops = (uint64_t)total * kThreads * iters;
    if (out_bytes != ops * 8) return (int)hipErrorInvalidValue;
    uint64_t* o = (uint64_t*)out;
    for (uint32_t g = 0; g < total * (uint32_t)kThreads; ++g)
      for (uint32_t s = 0; s < iters; ++s)
        o[(size_t)g * iters + s] =
            ((uint64_t)gm_atomics_addr(g, s, width) << 32) | gm_hostsync_token(g, s);
    return 0;
  }
  if (!gm_atomics_width_ok(kind, total, iters, width) ||
      out_bytes != (uint64_t)width * (gm_atomics_is64(kind) ? 8 : 4))
    return (int)hipErrorInvalidValue;
  gm_atomics_expected_host(kind, total, iters, width, seed, 0, 0, 0, out);
  return 0;
}

int gm_probe_hostsync_cas_width(uint32_t blocks, uint32_t host_threads, uint32_t iters,
                                uint32_t spread, uint32_t* width) {
  if (!width || !gm_hostsync_geometry_ok(blocks, host_threads, iters) ||
      !gm_atomics_pow2(spread) || spread > GM_HOSTSYNC_MAX_SPREAD)
    return (int)hipErrorInvalidValue;
  *width = gm_atomics_width(GM_ATOMICS_K_CAS, blocks + host_threads, iters, spread);
  return *width ? 0 : (int)hipErrorInvalidValue;
}

uint32_t gm_probe_hostsync_payload(uint64_t seed, uint32_t dir, uint32_t block, uint32_t round,
                                   uint32_t word) {
  return gm_hostsync_payload(seed, dir & 1u, block & 4095u, round & 63u, word & 16383u);
}

int gm_probe_hostsync_supported(int dev, int* supported) {
  if (dev < 0 || !supported) return (int)hipErrorInvalidValue;
  return (int)hipDeviceGetAttribute(supported, hipDeviceAttributeHostNativeAtomicSupported, dev);
}

int gm_probe_hostsync_add(uint32_t kind, uint32_t blocks, uint32_t host_threads, uint32_t iters,
                          uint32_t width, uint64_t seed, const gm_hostsync_inject_t* inject,
                          void* stream, void* table_out, gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (kind > GM_ATOMICS_K_ADD_U64 || !table_ok(kind, blocks, host_threads, iters, width) ||
      (inject && (!inject_ok(inject, GM_HOSTSYNC_ADD, blocks, host_threads, iters, 0, 0) ||
                  inject->kind != kind)))
    return (int)hipErrorInvalidValue;
  Ctx c;
  if (int e = begin(blocks, host_threads, iters, seed, inject, stream, out, &c)) return e;
  return run_add(c, kind, width, table_out);
}

int gm_probe_hostsync_ticket(uint32_t blocks, uint32_t host_threads, uint32_t iters,
                             uint32_t counters, uint64_t seed, const gm_hostsync_inject_t* inject,
                             void* stream, gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!table_ok(GM_ATOMICS_K_TICKET, blocks, host_threads, iters, counters) ||
      (inject && !inject_ok(inject, GM_HOSTSYNC_TICKET, blocks, host_threads, iters, 0, 0)))
    return (int)hipErrorInvalidValue;
  Ctx c;
  if (int e = begin(blocks, host_threads, iters, seed, inject, stream, out, &c)) return e;
  return run_ticket(c, counters);
}

int gm_probe_hostsync_swap(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint32_t width,
                           uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                           gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!table_ok(GM_ATOMICS_K_ADD_U32, blocks, host_threads, iters, width) ||
      (inject && !inject_ok(inject, GM_HOSTSYNC_SWAP, blocks, host_threads, iters, 0, 0)))
    return (int)hipErrorInvalidValue;
  Ctx c;
  if (int e = begin(blocks, host_threads, iters, seed, inject, stream, out, &c)) return e;
  return run_swap(c, width);
}

int gm_probe_hostsync_cas(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint32_t width,
                          uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                          void* table_out, gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!table_ok(GM_ATOMICS_K_CAS, blocks, host_threads, iters, width) ||
      (inject && !inject_ok(inject, GM_HOSTSYNC_CAS, blocks, host_threads, iters, 0, 0)))
    return (int)hipErrorInvalidValue;
  Ctx c;
  if (int e = begin(blocks, host_threads, iters, seed, inject, stream, out, &c)) return e;
  return run_cas(c, width, table_out);
}

int gm_probe_hostsync_handoff(uint32_t blocks, uint32_t host_threads, uint32_t rounds,
                              uint32_t lines, uint32_t budget_us, uint32_t host_budget_us,
                              uint64_t seed, const gm_hostsync_inject_t* inject, void* stream,
                              gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!gm_hostsync_handoff_ok(blocks, host_threads, rounds, lines, budget_us, host_budget_us) ||
      (inject && !inject_ok(inject, GM_HOSTSYNC_HANDOFF, blocks, host_threads, 0, rounds, lines)))
    return (int)hipErrorInvalidValue;
  Ctx c;
  if (int e = begin(blocks, host_threads, 0, seed, inject, stream, out, &c)) return e;
  out->rounds = rounds;
  out->lines = lines;
  out->budget_us = budget_us;
  out->host_budget_us = host_budget_us;
  return run_handoff(c, rounds, lines, budget_us, host_budget_us);
}

int gm_probe_hostsync(int dev, uint32_t tests_mask, uint32_t blocks, uint32_t host_threads,
                      uint32_t iters, uint32_t spread, uint32_t rounds, uint32_t lines,
                      uint32_t budget_us, uint32_t host_budget_us, uint64_t seed,
                      const gm_hostsync_inject_t* inject, gm_hostsync_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  const uint32_t probe_blocks = blocks ? blocks : 1;  // what does not depend on the count
  if (dev < 0 || tests_mask == 0 || (tests_mask & ~(uint32_t)GM_HOSTSYNC_ALL) ||
      blocks > GM_HOSTSYNC_MAX_BLOCKS ||
      !gm_hostsync_geometry_ok(probe_blocks, host_threads, iters) || !gm_atomics_pow2(spread) ||
      spread > GM_HOSTSYNC_MAX_SPREAD ||
      // the hand-off's arguments are checked even when it is not run, but it alone needs a thread
      !gm_hostsync_handoff_ok(probe_blocks, host_threads ? host_threads : 1, rounds, lines,
                              budget_us, host_budget_us) ||
      ((tests_mask & GM_HOSTSYNC_HANDOFF) && host_threads == 0) ||
      (inject && (!one_test(inject->test) || !(inject->test & tests_mask))) ||
      (inject && blocks &&
       !inject_ok(inject, inject->test, blocks, host_threads, iters, rounds, lines)))
    return (int)hipErrorInvalidValue;
  DeviceGuard guard(dev);
  if (!guard.ok) return (int)hipErrorInvalidDevice;
  const double t0 = now_s();
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  if (cus <= 0) return (int)hipErrorInvalidDevice;
  if (blocks == 0)
    blocks =
        (uint32_t)cus < GM_HOSTSYNC_DEFAULT_BLOCKS ? (uint32_t)cus : GM_HOSTSYNC_DEFAULT_BLOCKS;
  if (blocks > (uint32_t)cus || !gm_hostsync_geometry_ok(blocks, host_threads, iters) ||
      !gm_hostsync_handoff_ok(blocks, host_threads ? host_threads : 1, rounds, lines, budget_us,
                              host_budget_us) ||
      (inject && !inject_ok(inject, inject->test, blocks, host_threads, iters, rounds, lines)))
    return (int)hipErrorInvalidValue;
  const uint32_t cas_width =
      gm_atomics_width(GM_ATOMICS_K_CAS, blocks + host_threads, iters, spread);
  if (cas_width == 0) return (int)hipErrorInvalidValue;
  int native = 0;
  GM_CHECK(hipDeviceGetAttribute(&native, hipDeviceAttributeHostNativeAtomicSupported, dev));
  out->atomics_supported = native != 0;
  if (!native) {  // the link carries no AtomicOps: the hand-off alone decides
    out->tests_skipped = tests_mask & GM_HOSTSYNC_ATOMIC_TESTS;
    tests_mask &= ~(uint32_t)GM_HOSTSYNC_ATOMIC_TESTS;
    if (inject && (inject->test & out->tests_skipped)) return (int)hipErrorInvalidValue;
  }
  out->blocks = blocks;
  out->host_threads = host_threads;
  out->iters = iters;
  out->spread = spread;
  out->rounds = rounds;
  out->lines = lines;
  out->budget_us = budget_us;
  out->host_budget_us = host_budget_us;
  Stream stream;
  GM_CHECK(stream.create());
  const Ctx c{stream.s, blocks, host_threads, iters, seed, inject, out};
  if (tests_mask & GM_HOSTSYNC_ADD) {
    if (int e = run_add(c, GM_ATOMICS_K_ADD_U32, spread, nullptr)) return e;
    if (int e = run_add(c, GM_ATOMICS_K_ADD_U64, spread, nullptr)) return e;
    out->tests_run |= GM_HOSTSYNC_ADD;
  }
  if (tests_mask & GM_HOSTSYNC_TICKET) {
    if (int e = run_ticket(c, spread)) return e;
    out->tests_run |= GM_HOSTSYNC_TICKET;
  }
  if (tests_mask & GM_HOSTSYNC_SWAP) {
    if (int e = run_swap(c, spread)) return e;
    out->tests_run |= GM_HOSTSYNC_SWAP;
  }
  if (tests_mask & GM_HOSTSYNC_CAS) {
    if (int e = run_cas(c, cas_width, nullptr)) return e;
    out->tests_run |= GM_HOSTSYNC_CAS;
  }
  if (tests_mask & GM_HOSTSYNC_HANDOFF) {
    if (int e = run_handoff(c, rounds, lines, budget_us, host_budget_us)) return e;
    out->tests_run |= GM_HOSTSYNC_HANDOFF;
  }
  out->seconds = now_s() - t0;
  return 0;
}

}  // extern "C"
