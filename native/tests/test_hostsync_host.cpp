// The host-sync test's host side (include/gm_hostsync_ref.h, include/gm_hostsync_host.h) on its
// own, under ASan/UBSan (or TSan: make test_hostsync_host SAN=-fsanitize=thread): the swap audit
// on constructed chains, the atomics fold with host-played blocks against a naive loop, the
// host-thread operations against each other, and the hand-off protocol against a CPU stand-in for
// the kernel: a second set of std::threads doing the block's side with the same value functions
// and the __atomic_* builtins. No GPU, nothing else linked.
#include <stdio.h>
#include <string.h>

#include <array>
#include <thread>
#include <vector>

#include "gm_hostsync_host.h"
#include "gm_hostsync_ref.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      ++failures;                                                 \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
    }                                                             \
  } while (0)

static const uint64_t kSeed = 0x243F6A8885A308D3ull;

// ---- the swap audit on chains built one operation after the other
static void swap_chain(uint32_t total, uint32_t iters, uint32_t width, std::vector<uint32_t>& ret,
                       std::vector<uint32_t>& words) {
  const uint32_t T = total * GM_HOSTSYNC_THREADS;
  ret.assign((size_t)T * iters, 0);
  words.assign(width, 0);
  for (uint32_t g = T; g-- > 0;)  // any order is a legal one
    for (uint32_t s = 0; s < iters; ++s) {
      uint32_t& w = words[(g + 97u * s) % width];
      ret[(size_t)g * iters + s] = w;
      w = 1u + 1024u * g + s;
    }
}

static void check_swap_audit() {
  for (uint32_t width : {1u, 64u, 4096u}) {
    std::vector<uint32_t> ret, words;
    swap_chain(3, 3, width, ret, words);
    gm_hostsync_swap_audit_t a = gm_hostsync_swap_audit(3, 3, width, ret.data(), words.data());
    CHECK(a.missing == 0 && a.duplicates == 0 && a.foreign == 0 && a.first_bad_word == ~0ull);

    // one altered token: operation (300, 2) stored its token XOR 0x10, so whoever came next at
    // that word (or the final word) holds a value that is no token: s = 18 >= iters
    const uint32_t token = gm_hostsync_token(300, 2), w = (300u + 97u * 2u) % width;
    std::vector<uint32_t> r2 = ret, w2 = words;
    bool hit = false;
    for (uint32_t& v : r2)
      if (v == token) v ^= 0x10u, hit = true;
    if (!hit) {
      CHECK(w2[w] == token);
      w2[w] ^= 0x10u;
    }
    a = gm_hostsync_swap_audit(3, 3, width, r2.data(), w2.data());
    CHECK(a.missing == 1 && a.foreign == 1 && a.duplicates == 0);
    CHECK(a.first_bad_word == w && a.first_bad_value == (token ^ 0x10u));

    // a repeated value: an operation got what another had already got; the value it should
    // have got is then missing as well
    r2 = ret;
    const size_t op0 = 97 * 3 + 0, op1 = 0 * 3 + 1;  // (97, 0) and (0, 1) go to the same word
    CHECK(gm_atomics_addr(97, 0, width) == gm_atomics_addr(0, 1, width));
    CHECK(r2[op0] != r2[op1]);
    r2[op1] = r2[op0];
    a = gm_hostsync_swap_audit(3, 3, width, r2.data(), words.data());
    CHECK(a.duplicates == 1 && a.missing == 1 && a.foreign == 0);

    // a lost 0: the first operation into a word got a token instead
    r2 = ret;
    for (size_t i = 0; i < r2.size(); ++i)
      if (r2[i] == 0) {
        r2[i] = 0xFFFFFFFFu;
        break;
      }
    a = gm_hostsync_swap_audit(3, 3, width, r2.data(), words.data());
    CHECK(a.missing == 1 && a.foreign == 1 && a.duplicates == 0);
  }
  CHECK(gm_hostsync_token(0, 0) == 1 && gm_hostsync_token(300, 2) == 307203u);
}

// ---- the atomics fold over blocks + host_threads against a naive loop
static void check_fold(uint32_t blocks, uint32_t host_threads, uint32_t iters, uint32_t spread) {
  const uint32_t total = blocks + host_threads, T = total * GM_HOSTSYNC_THREADS;
  CHECK(gm_hostsync_geometry_ok(blocks, host_threads, iters));
  for (uint32_t kind : {(uint32_t)GM_ATOMICS_K_ADD_U32, (uint32_t)GM_ATOMICS_K_ADD_U64,
                        (uint32_t)GM_ATOMICS_K_TICKET, (uint32_t)GM_ATOMICS_K_CAS}) {
    const uint32_t width = gm_atomics_width(kind, total, iters, spread);
    CHECK(width >= spread);
    std::vector<uint64_t> naive(width, 0), ref(width, 0);
    for (uint32_t g = 0; g < T; ++g)
      for (uint32_t s = 0; s < iters; ++s) {
        const uint32_t h = gm_cuscan_hash(kSeed, 0x100u + kind, g * 1024u + s);
        const uint64_t hi = gm_cuscan_hash(kSeed, 0x120u + kind, g * 1024u + s);
        uint64_t& w = naive[(g + 97u * s) % width];
        if (kind == GM_ATOMICS_K_ADD_U32) w = (uint32_t)(w + h);
        else if (kind == GM_ATOMICS_K_TICKET) w += 1u + (h & 3u);
        else w += (hi << 32) | h;
      }
    if (gm_atomics_is64(kind)) {
      gm_atomics_expected_host(kind, total, iters, width, kSeed, 0, 0, 0, ref.data());
    } else {
      std::vector<uint32_t> r32(width);
      gm_atomics_expected_host(kind, total, iters, width, kSeed, 0, 0, 0, r32.data());
      for (uint32_t w = 0; w < width; ++w) ref[w] = r32[w];
    }
    CHECK(naive == ref);
  }
}

// ---- the host-thread operations: every block played by a host thread, all at once, must give
// the reference's tables and clean audits
static void check_host_ops(uint32_t total, uint32_t iters, uint32_t spread) {
  uint32_t ready = 1;
  gm_hostsync_gate_t gate;
  gate.ready = &ready;
  const gm_hostsync_inj_t none;
  auto all = [&](auto fn) {
    std::vector<std::thread> th;
    for (uint32_t j = 0; j < total; ++j) th.emplace_back([&, j] { fn(j); });
    for (std::thread& t : th) t.join();
  };
  CHECK(gm_hostsync_wait_start(&gate));
  for (uint32_t kind : {(uint32_t)GM_ATOMICS_K_ADD_U32, (uint32_t)GM_ATOMICS_K_ADD_U64}) {
    std::vector<uint64_t> table(spread, 0), exp(spread, 0);  // u32 uses the front half
    std::vector<uint64_t> flying(total, 0);
    all([&](uint32_t j) {
      flying[j] = gm_hostsync_host_add(kind, table.data(), spread, j, iters, kSeed, none, &gate);
    });
    gm_atomics_expected_host(kind, total, iters, spread, kSeed, 0, 0, 0, exp.data());
    CHECK(table == exp);
    CHECK(flying[0] == (uint64_t)GM_HOSTSYNC_THREADS * iters);  // done was never set
  }
  {  // an injected add differs from the clean table in exactly one word
    std::vector<uint32_t> table(spread, 0), exp(spread, 0);
    gm_hostsync_inj_t inj;
    inj.a = 300 % (total * GM_HOSTSYNC_THREADS), inj.b = iters - 1, inj.mask = 0x10, inj.on = 1;
    all([&](uint32_t j) {
      gm_hostsync_host_add(GM_ATOMICS_K_ADD_U32, table.data(), spread, j, iters, kSeed, inj, &gate);
    });
    gm_atomics_expected_host(GM_ATOMICS_K_ADD_U32, total, iters, spread, kSeed, 0, 0, 0,
                             exp.data());
    uint32_t bad = 0;
    for (uint32_t w = 0; w < spread; ++w) bad += table[w] != exp[w];
    CHECK(bad == 1);
  }
  {  // ticket, clean and with the control
    std::vector<uint32_t> n(spread);
    gm_atomics_expected_host(GM_ATOMICS_K_TICKET, total, iters, spread, kSeed, 0, 0, 0, n.data());
    std::vector<uint64_t> off((size_t)spread + 1, 0);
    for (uint32_t k = 0; k < spread; ++k) off[k + 1] = off[k] + n[k];
    for (int control = 0; control < 2; ++control) {
      std::vector<uint32_t> ctr(spread, 0), marks(off[spread], 0);
      std::vector<uint64_t> oor(total, 0);
      gm_hostsync_inj_t inj;
      inj.a = 7, inj.b = 0, inj.on = control;
      all([&](uint32_t j) {
        gm_hostsync_host_ticket(ctr.data(), off.data(), marks.data(), off[spread], spread, j,
                                iters, kSeed, inj, &gate, &oor[j]);
      });
      const gm_hostsync_ticket_audit_t a =
          gm_hostsync_ticket_audit(ctr.data(), n.data(), spread, marks.data(), off[spread]);
      CHECK(a.holes == 0 && a.counter_errors == 0 && a.duplicates == (uint64_t)control);
      for (uint64_t v : oor) CHECK(v == 0);
    }
  }
  {  // swap, clean and with the control
    for (int control = 0; control < 2; ++control) {
      std::vector<uint32_t> words(spread, 0), ret((size_t)total * GM_HOSTSYNC_THREADS * iters);
      gm_hostsync_inj_t inj;
      inj.a = 7, inj.b = 0, inj.mask = 0x40000000u, inj.on = control;
      all([&](uint32_t j) {
        gm_hostsync_host_swap(words.data(), spread, j, iters, inj, &gate,
                              ret.data() + (size_t)j * GM_HOSTSYNC_THREADS * iters);
      });
      const gm_hostsync_swap_audit_t a =
          gm_hostsync_swap_audit(total, iters, spread, ret.data(), words.data());
      CHECK(a.missing == (uint64_t)control && a.foreign == (uint64_t)control && a.duplicates == 0);
    }
  }
  {  // cas
    const uint32_t width = gm_atomics_width(GM_ATOMICS_K_CAS, total, iters, spread);
    std::vector<uint32_t> count;
    gm_atomics_counts(total, iters, width, count);
    std::vector<uint64_t> table(width, 0), exp(width, 0), gave(total, 0);
    all([&](uint32_t j) {
      gm_hostsync_host_cas(table.data(), count.data(), width, j, iters, kSeed, none, &gate,
                           &gave[j]);
    });
    gm_atomics_expected_host(GM_ATOMICS_K_CAS, total, iters, width, kSeed, 0, 0, 0, exp.data());
    CHECK(table == exp);
    for (uint64_t v : gave) CHECK(v == 0);
  }
  // a launch that was called off starts nothing
  uint32_t never = 0;
  gm_hostsync_gate_t off_gate;
  off_gate.ready = &never;
  off_gate.abort = 1;
  CHECK(!gm_hostsync_wait_start(&off_gate));
}

// ---- the hand-off against a CPU stand-in for the kernel
struct StandIn {
  uint64_t handoffs = 0, observed = 0, unseen = 0, stale = 0;
};

// the block's side of gm_probe.h's steps 2 and 3 for block b; answer false: never raise a flag
static void block_side(const gm_hostsync_handoff_t& c, uint32_t b, double budget_us, bool answer,
                       StandIn* st) {
  const size_t box = gm_hostsync_box_words(c);
  for (uint32_t r = 0; r < c.rounds; ++r) {
    const size_t m = (size_t)b * c.rounds + r;
    const uint32_t* flag = &c.flag_h[m * GM_HOSTSYNC_FLAG_WORDS];
    const double t0 = gm_hostsync_now_us();
    bool seen = false;
    while (gm_hostsync_now_us() - t0 <= budget_us)
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == r + 1u) {
        seen = true;
        break;
      }
    ++st->handoffs;
    if (seen) {
      ++st->observed;
      const uint32_t* src = c.pay_h + m * box;
      for (uint32_t word = 0; word < box; ++word)
        st->stale += src[word] != gm_hostsync_payload(c.seed, 0, b, r, word);
    } else {
      ++st->unseen;
    }
    if (!answer) continue;
    uint32_t* dst = c.pay_d + m * box;
    for (uint32_t word = 0; word < box; ++word) {
      uint32_t v = gm_hostsync_payload(c.seed, 1, b, r, word);
      if (c.inj.on && c.inj.dir == 1 && b == c.inj.a && r == c.inj.b && word == c.inj.word)
        v ^= c.inj.mask;
      dst[word] = v;
    }
    __atomic_store_n(&c.flag_d[m * GM_HOSTSYNC_FLAG_WORDS], ((uint32_t)seen << 16) | (r + 1u),
                     __ATOMIC_RELEASE);
  }
}

struct HandoffRun {
  StandIn gpu;
  gm_hostsync_host_stats_t host;
  uint64_t lost = 0;
  std::vector<gm_hostsync_bad_word_t> bad;
};

static HandoffRun handoff(uint32_t blocks, uint32_t host_threads, uint32_t rounds, uint32_t lines,
                          const gm_hostsync_inj_t& inj, bool answer, uint32_t host_budget_us,
                          double budget_us) {
  const size_t boxes = (size_t)blocks * rounds, box = (size_t)lines * GM_HOSTSYNC_LINE_WORDS;
  std::vector<uint32_t> pay_h(boxes * box, 0xA5A5A5A5u), pay_d(boxes * box, 0xA5A5A5A5u);
  std::vector<uint32_t> flag_h(boxes * GM_HOSTSYNC_FLAG_WORDS, 0),
      flag_d(boxes * GM_HOSTSYNC_FLAG_WORDS, 0);
  gm_hostsync_handoff_t c;
  c.pay_h = pay_h.data(), c.pay_d = pay_d.data();
  c.flag_h = flag_h.data(), c.flag_d = flag_d.data();
  c.blocks = blocks, c.host_threads = host_threads, c.rounds = rounds, c.lines = lines;
  c.host_budget_us = host_budget_us, c.seed = kSeed, c.inj = inj;
  std::vector<StandIn> gpu(blocks);
  std::vector<gm_hostsync_host_stats_t> host(host_threads);
  std::vector<std::thread> th;
  for (uint32_t b = 0; b < blocks; ++b)
    th.emplace_back([&, b] { block_side(c, b, budget_us, answer, &gpu[b]); });
  for (uint32_t j = 0; j < host_threads; ++j)
    th.emplace_back([&, j] { gm_hostsync_host_serve(c, j, &host[j]); });
  for (std::thread& t : th) t.join();
  HandoffRun out;
  for (const StandIn& s : gpu) {
    out.gpu.handoffs += s.handoffs, out.gpu.observed += s.observed;
    out.gpu.unseen += s.unseen, out.gpu.stale += s.stale;
  }
  for (const gm_hostsync_host_stats_t& s : host) {
    out.host.handoffs += s.handoffs, out.host.observed += s.observed;
    out.host.unseen += s.unseen, out.host.stale += s.stale;
    out.host.rtt_us.insert(out.host.rtt_us.end(), s.rtt_us.begin(), s.rtt_us.end());
    out.host.bad.insert(out.host.bad.end(), s.bad.begin(), s.bad.end());
    if (s.poll_max_us > out.host.poll_max_us) out.host.poll_max_us = s.poll_max_us;
  }
  out.lost = gm_hostsync_host_audit(c, &out.bad);
  return out;
}

static void check_handoff() {
  const gm_hostsync_inj_t none;
  // generous budgets: a loaded build machine must not make a clean run look unseen
  const uint32_t host_budget = 5000000;
  const double budget = 5e6;
  const std::array<uint32_t, 4> shapes[] = {{1, 1, 1, 1}, {2, 1, 3, 16}, {5, 2, 3, 1}};
  for (const auto& [blocks, threads, rounds, lines] : shapes) {
    const HandoffRun r = handoff(blocks, threads, rounds, lines, none, true, host_budget, budget);
    const uint64_t n = (uint64_t)blocks * rounds;
    CHECK(r.gpu.handoffs == n && r.gpu.observed == n && r.gpu.unseen == 0 && r.gpu.stale == 0);
    CHECK(r.host.handoffs == n && r.host.observed == n && r.host.unseen == 0);
    CHECK(r.host.stale == 0 && r.lost == 0 && r.host.rtt_us.size() == n);
    CHECK(r.host.poll_max_us <= host_budget && gm_hostsync_median(r.host.rtt_us) > 0);
  }
  for (uint32_t dir = 0; dir < 2; ++dir) {  // exactly one stale word, in that direction
    gm_hostsync_inj_t inj;
    inj.dir = dir, inj.a = 1, inj.b = 2, inj.word = 1500, inj.mask = 0x100, inj.on = 1;
    const HandoffRun r = handoff(2, 1, 3, 16, inj, true, host_budget, budget);
    CHECK(r.gpu.stale == (dir == 0) && r.host.stale == (dir == 1) && r.lost == 1);
    CHECK(r.gpu.observed == 6 && r.host.observed == 6);
    CHECK(!r.bad.empty() && r.bad.back().dir == dir &&
          r.bad.back().index == ((1ull << 20) | (2ull << 14) | 1500u) &&
          (r.bad.back().expected ^ r.bad.back().got) == 0x100u);
    if (dir == 1) CHECK(r.host.bad.size() == 1 && r.host.bad[0].index == r.bad.back().index);
  }
  {  // a stand-in that never answers: the budgets bound the host, every reply is unseen
    const HandoffRun r = handoff(2, 1, 2, 1, none, false, 2000, 2e6);
    CHECK(r.host.handoffs == 4 && r.host.unseen == 4 && r.host.observed == 0);
    CHECK(r.host.stale == 0 && r.gpu.observed == 4);
    CHECK(r.lost == 2 * 2 * (1024 + 1));  // nothing of the replies is there, flags included
  }
  CHECK(gm_hostsync_payload(kSeed, 1, 3, 2, 1500) ==
        gm_cuscan_hash(kSeed, 0x601u, (3u << 20) | (2u << 14) | 1500u));
  CHECK(gm_hostsync_payload(kSeed, 0, 3, 2, 1500) != gm_hostsync_payload(kSeed, 1, 3, 2, 1500));
}

static void check_limits() {
  CHECK(gm_hostsync_geometry_ok(1, 0, 1) && gm_hostsync_geometry_ok(16, 2, 4));
  CHECK(!gm_hostsync_geometry_ok(0, 1, 1) && !gm_hostsync_geometry_ok(1, 9, 1));
  CHECK(!gm_hostsync_geometry_ok(1, 0, 0) && !gm_hostsync_geometry_ok(1, 0, 1025));
  CHECK(gm_hostsync_geometry_ok(4, 0, 1024) && !gm_hostsync_geometry_ok(4, 1, 1024));  // 2^20
  CHECK(gm_hostsync_handoff_ok(16, 2, 8, 16, 2000, 10000));
  CHECK(!gm_hostsync_handoff_ok(16, 0, 8, 16, 2000, 10000));
  CHECK(!gm_hostsync_handoff_ok(16, 2, 65, 16, 2000, 10000));
  CHECK(!gm_hostsync_handoff_ok(16, 2, 8, 2, 2000, 10000));
  CHECK(!gm_hostsync_handoff_ok(16, 2, 8, 16, 20001, 10000));
  CHECK(!gm_hostsync_handoff_ok(16, 2, 8, 16, 2000, 0));
  CHECK(!gm_hostsync_handoff_ok(4096, 2, 64, 16, 2000, 10000));  // 32 GiB of mailboxes
}

int main() {
  check_swap_audit();
  check_fold(1, 0, 1, 1);
  check_fold(2, 1, 3, 64);
  check_fold(9, 3, 3, 1);
  check_host_ops(3, 3, 1);
  check_host_ops(4, 2, 64);
  check_handoff();
  check_limits();
  if (failures) {
    fprintf(stderr, "test_hostsync_host: %d failure(s)\n", failures);
    return 1;
  }
  printf("test_hostsync_host: ok\n");
  return 0;
}
