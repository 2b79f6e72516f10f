// The atomics test's host reference (include/gm_atomics_ref.h) on its own, under ASan/UBSan:
// the folds against a second, differently ordered fold, the per-word counts against brute force,
// the width rule and the caps, and what the reference refuses; and the steps the kernels and the
// host threads run (include/gm_atomics_steps.h) over a serial policy against that reference and
// the host audits. No GPU, nothing else linked.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "gm_atomics_ref.h"
#include "gm_atomics_steps.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      ++failures;                                                 \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
    }                                                             \
  } while (0)

static const uint64_t kSeed = 0x243F6A8885A308D3ull;

// the same operations, last thread first: they commute, so the table must not change
static void fold_reversed(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t width,
                          std::vector<uint64_t>& out) {
  const uint32_t T = blocks * GM_ATOMICS_THREADS;
  out.assign(width, gm_atomics_init_byte(kind) ? 0xFFFFFFFFull : 0ull);
  std::vector<int64_t> sum(width, 0);
  std::vector<uint32_t> lo(width, 0), hi(width, 0);
  for (uint32_t g = T; g-- > 0;)
    for (uint32_t s = iters; s-- > 0;) {
      const uint32_t h = gm_atomics_hash(kSeed, kind, 0, g, s);
      const uint32_t w = (g + 97u * s) % width;
      const uint64_t op = ((uint64_t)gm_atomics_hash(kSeed, kind, 1, g, s) << 32) | h;
      switch (kind) {
        case GM_ATOMICS_K_ADD_U32: out[w] = (uint32_t)(out[w] + h); break;
        case GM_ATOMICS_K_ADD_U64:
        case GM_ATOMICS_K_CAS: out[w] += op; break;
        case GM_ATOMICS_K_XOR_U64: out[w] ^= op; break;
        case GM_ATOMICS_K_UMAX_U32: if (h > out[w]) out[w] = h; break;
        case GM_ATOMICS_K_UMIN_U32: if (h < out[w]) out[w] = h; break;
        case GM_ATOMICS_K_AND_U32: out[w] &= ~(uint64_t)gm_atomics_bit(h) & 0xFFFFFFFFull; break;
        case GM_ATOMICS_K_OR_U32: out[w] |= gm_atomics_bit(h); break;
        case GM_ATOMICS_K_ADD_F32:
        case GM_ATOMICS_K_ADD_F64: sum[w] += (int)(h % 9u) - 4; break;
        case GM_ATOMICS_K_PK_ADD_BF16: lo[w] += h & 1u, hi[w] += (h >> 1) & 1u; break;
        case GM_ATOMICS_K_TICKET: out[w] += 1u + (h & 3u); break;
        case GM_ATOMICS_K_COUNT: out[w] += 1; break;
      }
    }
  for (uint32_t w = 0; w < width; ++w) {
    if (kind == GM_ATOMICS_K_ADD_F32) out[w] = gm_atomics_f32_bits((float)sum[w]);
    if (kind == GM_ATOMICS_K_ADD_F64) out[w] = gm_atomics_f64_bits((double)sum[w]);
    if (kind == GM_ATOMICS_K_PK_ADD_BF16)
      out[w] = (gm_atomics_f32_bits((float)lo[w]) >> 16) |
               (gm_atomics_f32_bits((float)hi[w]) & 0xFFFF0000u);
  }
}

static void check_folds(uint32_t blocks, uint32_t iters, uint32_t spread) {
  for (uint32_t kind = 0; kind <= GM_ATOMICS_K_COUNT; ++kind) {
    if (kind == GM_ATOMICS_K_HANDOFF) continue;
    const uint32_t width = gm_atomics_width(kind, blocks, iters, spread);
    CHECK(width >= spread && gm_atomics_pow2(width));
    CHECK(gm_atomics_width_ok(kind, blocks, iters, width));
    std::vector<uint64_t> want;
    fold_reversed(kind, blocks, iters, width, want);
    // exactly the bytes the caller is promised: ASan sees one word too many
    if (gm_atomics_is64(kind)) {
      std::vector<uint64_t> got(width, 0x5555555555555555ull);
      gm_atomics_expected_host(kind, blocks, iters, width, kSeed, 0, 0, 0, got.data());
      for (uint32_t w = 0; w < width; ++w) CHECK(got[w] == want[w]);
    } else {
      std::vector<uint32_t> got(width, 0x55555555u);
      gm_atomics_expected_host(kind, blocks, iters, width, kSeed, 0, 0, 0, got.data());
      for (uint32_t w = 0; w < width; ++w) CHECK(got[w] == (uint32_t)want[w]);
    }
  }
}

// ---- the family's steps (include/gm_atomics_steps.h), which the kernels and the host threads
// run, over a serial policy: plain reads and writes on one thread, every kind
struct SerialOps {
  static constexpr uint32_t kKinds = GM_ATOMICS_ADD_KINDS;
  template <class T, class F>
  static T apply(T* p, F f) {
    const T old = *p;
    *p = f(old);
    return old;
  }
  template <class T>
  static T fetch_add(T* p, T v) { return apply(p, [v](T o) { return (T)(o + v); }); }
  static uint64_t fetch_xor(uint64_t* p, uint64_t v) {
    return apply(p, [v](uint64_t o) { return o ^ v; });
  }
  static uint32_t fetch_max(uint32_t* p, uint32_t v) {
    return apply(p, [v](uint32_t o) { return o > v ? o : v; });
  }
  static uint32_t fetch_min(uint32_t* p, uint32_t v) {
    return apply(p, [v](uint32_t o) { return o < v ? o : v; });
  }
  static uint32_t fetch_and(uint32_t* p, uint32_t v) {
    return apply(p, [v](uint32_t o) { return o & v; });
  }
  static uint32_t fetch_or(uint32_t* p, uint32_t v) {
    return apply(p, [v](uint32_t o) { return o | v; });
  }
  // a bf16 is the upper half of an f32; the halves' sums stay within GM_ATOMICS_BF16_CAP = 128,
  // integers of at most 8 significant bits, so adding in float and cutting is exact
  static void pk_add_bf16(uint32_t* p, uint32_t lo, uint32_t hi) {
    auto f32 = [](uint32_t bits) {
      float f;
      memcpy(&f, &bits, 4);
      return f;
    };
    const float a = f32(*p << 16) + (float)lo, b = f32(*p & 0xFFFF0000u) + (float)hi;
    *p = (gm_atomics_f32_bits(a) >> 16) | (gm_atomics_f32_bits(b) & 0xFFFF0000u);
  }
  static uint32_t exchange(uint32_t* p, uint32_t v) {
    return apply(p, [v](uint32_t) { return v; });
  }
  static uint64_t load(const uint64_t* p) { return *p; }
  static bool cas(uint64_t* p, uint64_t* old, uint64_t want) {
    if (*p != *old) return *old = *p, false;
    return *p = want, true;
  }
};

// every (g, s) of the geometry through step(g, s)
template <class Step>
static void every_step(uint32_t blocks, uint32_t iters, Step step) {
  for (uint32_t s = 0; s < iters; ++s)
    for (uint32_t g = 0; g < blocks * GM_ATOMICS_THREADS; ++g) step(g, s);
}

// words of `kind`'s table after the steps that differ from the reference's clean table
static uint32_t table_diff(uint32_t kind, uint32_t blocks, uint32_t iters, uint32_t width,
                           const gm_atomics_inj_t& inj) {
  const uint32_t wb = gm_atomics_is64(kind) ? 8 : 4;
  // exactly the bytes a kernel's table has: ASan sees a step one word too far
  std::vector<unsigned char> got((size_t)width * wb, (unsigned char)gm_atomics_init_byte(kind)),
      want((size_t)width * wb);
  gm_atomics_expected_host(kind, blocks, iters, width, kSeed, 0, 0, 0, want.data());
  uint64_t giveups = 0;
  if (kind == GM_ATOMICS_K_CAS) {
    std::vector<uint32_t> bound;
    gm_atomics_counts(blocks, iters, width, bound);
    every_step(blocks, iters, [&](uint32_t g, uint32_t s) {
      giveups += !gm_atomics_cas_step<SerialOps>((uint64_t*)got.data(), bound.data(), width, kSeed,
                                                 inj, g, s);
    });
  } else {
    every_step(blocks, iters, [&](uint32_t g, uint32_t s) {
      gm_atomics_add_step<SerialOps>(kind, got.data(), width, kSeed, inj, g, s);
    });
  }
  CHECK(giveups == 0);
  uint32_t differ = 0;
  for (uint32_t w = 0; w < width; ++w)
    differ += memcmp(&got[(size_t)w * wb], &want[(size_t)w * wb], wb) != 0;
  return differ;
}

// the ticket step over every (g, s): the host audit of its counters and marks
static gm_hostsync_ticket_audit_t ticket_run(uint32_t blocks, uint32_t iters, uint32_t counters,
                                             const gm_atomics_inj_t& inj) {
  std::vector<uint32_t> n(counters);
  gm_atomics_expected_host(GM_ATOMICS_K_TICKET, blocks, iters, counters, kSeed, 0, 0, 0, n.data());
  std::vector<uint64_t> off((size_t)counters + 1, 0);
  for (uint32_t k = 0; k < counters; ++k) off[k + 1] = off[k] + n[k];
  std::vector<uint32_t> ctr(counters, 0), marks(off[counters], 0);
  uint64_t out_of_range = 0, drawn = 0;
  every_step(blocks, iters, [&](uint32_t g, uint32_t s) {
    uint32_t old = ~0u, d = 0;
    out_of_range += gm_atomics_ticket_step<SerialOps>(ctr.data(), off.data(), marks.data(),
                                                      off[counters], counters, kSeed, inj, g, s,
                                                      old, d);
    CHECK(d >= 1 && d <= 4 && (uint64_t)old + d <= n[gm_atomics_addr(g, s, counters)]);
    drawn += d;
  });
  CHECK(out_of_range == 0 && drawn == off[counters]);
  return gm_hostsync_ticket_audit(ctr.data(), n.data(), counters, marks.data(), off[counters]);
}

static gm_hostsync_swap_audit_t swap_run(uint32_t blocks, uint32_t iters, uint32_t width,
                                         const gm_atomics_inj_t& inj) {
  std::vector<uint32_t> words(width, 0), ret((size_t)blocks * GM_ATOMICS_THREADS * iters);
  every_step(blocks, iters, [&](uint32_t g, uint32_t s) {
    ret[(size_t)g * iters + s] = gm_hostsync_swap_step<SerialOps>(words.data(), width, inj, g, s);
  });
  return gm_hostsync_swap_audit(blocks, iters, width, ret.data(), words.data());
}

static void check_steps(uint32_t blocks, uint32_t iters, uint32_t spread) {
  const gm_atomics_inj_t none;
  for (uint32_t kind = 0; kind <= GM_ATOMICS_K_CAS; ++kind) {
    if (kind == GM_ATOMICS_K_TICKET) continue;
    const uint32_t width = gm_atomics_width(kind, blocks, iters, spread);
    CHECK(table_diff(kind, blocks, iters, width, none) == 0);
  }
  const gm_hostsync_ticket_audit_t t = ticket_run(blocks, iters, spread, none);
  CHECK(t.holes == 0 && t.duplicates == 0 && t.counter_errors == 0 && t.first_index == ~0ull);
  const gm_hostsync_swap_audit_t w = swap_run(blocks, iters, spread, none);
  CHECK(w.missing == 0 && w.duplicates == 0 && w.foreign == 0);
}

int main() {
  // the steps at the same shapes, and with a negative control at g = 300, s = 2: one word of
  // add and CAS (the kinds where every mask changes the word), one duplicate ticket, one token
  check_steps(1, 1, 1);
  check_steps(2, 3, 64);
  check_steps(9, 3, 1);
  check_steps(9, 2, 4096);
  {
    gm_atomics_inj_t inj;
    inj.a = 300, inj.b = 2, inj.mask = 0x10000u, inj.on = 1;
    for (uint32_t kind : {(uint32_t)GM_ATOMICS_K_ADD_U32, (uint32_t)GM_ATOMICS_K_ADD_U64,
                          (uint32_t)GM_ATOMICS_K_XOR_U64, (uint32_t)GM_ATOMICS_K_CAS})
      CHECK(table_diff(kind, 2, 3, gm_atomics_width(kind, 2, 3, 64), inj) == 1);
    const gm_hostsync_ticket_audit_t t = ticket_run(2, 3, 64, inj);
    CHECK(t.duplicates == 1 && t.holes == 0 && t.counter_errors == 0);
    inj.mask = 0x40000000u;  // no token of any thread of the run
    const gm_hostsync_swap_audit_t w = swap_run(2, 3, 64, inj);
    CHECK(w.missing == 1 && w.foreign == 1 && w.duplicates == 0);
  }

  // geometry
  CHECK(gm_atomics_geometry_ok(1, 1) && gm_atomics_geometry_ok(4096, 64));
  CHECK(!gm_atomics_geometry_ok(0, 1) && !gm_atomics_geometry_ok(4097, 1));
  CHECK(!gm_atomics_geometry_ok(1, 0) && !gm_atomics_geometry_ok(1, 1025));
  CHECK(!gm_atomics_geometry_ok(4096, 65));  // T * iters > 2^26
  CHECK(gm_atomics_pow2(1) && gm_atomics_pow2(65536) && !gm_atomics_pow2(0) && !gm_atomics_pow2(96));

  // folds, counts and widths at the shapes the GPU tests use
  check_folds(1, 1, 1);
  check_folds(2, 3, 64);
  check_folds(9, 3, 1);
  check_folds(9, 2, 4096);

  // the width rule: bf16 at (9, 3, 1) has 6912 adds, so at least 54 words: 64
  CHECK(gm_atomics_width(GM_ATOMICS_K_PK_ADD_BF16, 9, 3, 1) == 64);
  CHECK(gm_atomics_max_adds(9, 3, 64) == 108);
  CHECK(gm_atomics_width(GM_ATOMICS_K_PK_ADD_BF16, 1, 1, 1) == 2);    // 256 adds
  CHECK(gm_atomics_width(GM_ATOMICS_K_PK_ADD_BF16, 9, 2, 4096) == 4096);
  CHECK(gm_atomics_width(GM_ATOMICS_K_ADD_F32, 9, 3, 1) == 1);
  CHECK(gm_atomics_width(GM_ATOMICS_K_ADD_U32, 4096, 64, 1) == 1);     // no cap
  // 2^26 adds into one word break the float cap of 2^22 - 1: the table widens to 32 words
  CHECK(gm_atomics_width(GM_ATOMICS_K_ADD_F64, 4096, 64, 1) == 32);
  CHECK(gm_atomics_max_adds(4096, 64, 32) == (1u << 21));
  // every busiest word is counted, not estimated: 3 blocks over 512 words is uneven
  {
    std::vector<uint32_t> c;
    gm_atomics_counts(3, 5, 512, c);
    uint64_t total = 0;
    for (uint32_t v : c) total += v;
    CHECK(total == 3u * 256u * 5u);
  }

  // refusals: a width that breaks a cap, no power of two, too wide
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_PK_ADD_BF16, 9, 3, 32));
  CHECK(gm_atomics_width_ok(GM_ATOMICS_K_PK_ADD_BF16, 9, 3, 64));
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_ADD_F32, 4096, 64, 16));
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_ADD_F64, 4096, 64, 16));
  CHECK(gm_atomics_width_ok(GM_ATOMICS_K_ADD_F32, 4096, 64, 32));
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_ADD_U32, 1, 1, 0));
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_ADD_U32, 1, 1, 96));
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_ADD_U32, 1, 1, GM_ATOMICS_MAX_WIDTH * 2));
  CHECK(gm_atomics_cap(GM_ATOMICS_K_CAS) == 1024 && gm_atomics_cap(GM_ATOMICS_K_PK_ADD_BF16) == 128);
  CHECK(gm_atomics_cap(GM_ATOMICS_K_TICKET) == 0 && gm_atomics_cap(GM_ATOMICS_K_XOR_U64) == 0);
  CHECK(gm_atomics_width(GM_ATOMICS_K_CAS, 9, 3, 1) == 8);  // 6912 operations: 864 a word
  CHECK(!gm_atomics_width_ok(GM_ATOMICS_K_CAS, 9, 3, 4));

  // a negative control changes exactly one word of add, xor and CAS
  for (uint32_t kind : {(uint32_t)GM_ATOMICS_K_ADD_U32, (uint32_t)GM_ATOMICS_K_ADD_U64,
                        (uint32_t)GM_ATOMICS_K_XOR_U64, (uint32_t)GM_ATOMICS_K_CAS}) {
    const uint32_t width = 64, wb = gm_atomics_is64(kind) ? 8 : 4;
    std::vector<unsigned char> a(width * wb), b(width * wb);
    gm_atomics_expected_host(kind, 2, 3, width, kSeed, 0, 0, 0, a.data());
    gm_atomics_expected_host(kind, 2, 3, width, kSeed, 300, 2, 0x10000u, b.data());
    uint32_t differ = 0;
    for (uint32_t w = 0; w < width; ++w) differ += memcmp(&a[w * wb], &b[w * wb], wb) != 0;
    CHECK(differ == 1);
    CHECK(memcmp(&a[gm_atomics_addr(300, 2, width) * wb], &b[gm_atomics_addr(300, 2, width) * wb],
                 wb) != 0);
  }

  // hand-off: the partner is never the block itself, and every block is read once per round
  for (uint32_t G : {2u, 9u, 256u})
    for (uint32_t r = 0; r < 64; ++r) {
      std::vector<uint32_t> readers(G, 0);
      for (uint32_t b = 0; b < G; ++b) {
        const uint32_t p = gm_atomics_partner(b, r, G);
        CHECK(p < G && p != b);
        ++readers[p];
      }
      for (uint32_t b = 0; b < G; ++b) CHECK(readers[b] == 1);
    }
  CHECK(gm_atomics_partner(0, 5, 1) == 0);
  CHECK(gm_atomics_payload(kSeed, 1, 2, 3) != gm_atomics_payload(kSeed, 1, 2, 4));
  CHECK(gm_atomics_payload(kSeed, 4095, 63, 16383) != gm_atomics_payload(kSeed, 4095, 63, 16382));

  if (failures) {
    fprintf(stderr, "test_atomics_host: %d failure(s)\n", failures);
    return 1;
  }
  printf("test_atomics_host: ok\n");
  return 0;
}
