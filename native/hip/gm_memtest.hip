// gm_memtest.hip — HBM pattern test for gfx950: does the VRAM hold what is written to it?
//
// Three kinds of launch of the pattern-stream kernel (gm_pattern_stream.h), 8 loads in flight per
// lane, CUs × 2 blocks:
//   fill           writes P (or ~P)
//   verify_invert  reads and checks P, writes ~P over the same words
//   verify         reads and checks
// All three walk the region in the same order: what was written first is read first, after
// everything else has gone through the caches. Inside one launch the blocks run in whatever
// order the dispatcher picks; there is no ascending or descending direction as in a CPU march
// test.
#include <atomic>
#include <deque>

#include "gm_pattern_stream.h"

namespace {

constexpr int kInFlight = 8;          // 16-B accesses per lane per unrolled step
constexpr int kBlocksPerCu = 2;       // gm_probe_hbm_read's default geometry
constexpr size_t kStepElems = (size_t)kInFlight * 256;  // 16-B elements per block per step

std::atomic<int> g_nt_store{1};

// The store variant picks the writing kernels; verify stores nothing and has one.
int launch(int mode, uint32_t pattern, int cus, hipStream_t s, void* ptr, uint64_t bytes,
           const Args& a, DevResult* res) {
  const size_t n = bytes / 16;
  const size_t blocks = (size_t)(cus > 0 ? cus : 1) * kBlocksPerCu;
  const StreamLaunch l{gm_pattern_chunks(n, blocks, kStepElems), s, ptr, nullptr, n, a, res};
  const bool nt = g_nt_store.load() != 0;
  const bool known = dispatch_pattern(pattern, [&](auto p) {
    constexpr uint32_t P = decltype(p)::value;
    if (mode == kCheck)
      l.run<P, kCheck, kInFlight, false, false>();
    else if (mode == kWrite)
      nt ? l.run<P, kWrite, kInFlight, true, false>() : l.run<P, kWrite, kInFlight, false, false>();
    else
      nt ? l.run<P, kCheckInvert, kInFlight, true, false>()
         : l.run<P, kCheckInvert, kInFlight, false, false>();
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

struct Piece {
  DevBuf buf;
  uint64_t bytes = 0, base = 0;
};

}  // namespace

extern "C" {

int gm_probe_mem_info(int dev, uint64_t* free_bytes, uint64_t* total_bytes) {
  *free_bytes = *total_bytes = 0;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  size_t f = 0, t = 0;
  GM_CHECK(hipMemGetInfo(&f, &t));
  *free_bytes = f;
  *total_bytes = t;
  return 0;
}

int gm_probe_memtest_expected(uint32_t pattern, uint64_t seed, uint32_t pass,
                              uint64_t base_offset, uint64_t n_words, uint64_t* out) {
  if (!one_pattern(pattern) || (base_offset & 7) || (n_words && !out))
    return (int)hipErrorInvalidValue;
  for (uint64_t i = 0; i < n_words; ++i)
    out[i] = gm_memtest_expected(pattern, seed, pass, base_offset + 8 * i);
  return 0;
}

int gm_probe_memtest_store_variant(int nontemporal) {
  if (nontemporal == 0 || nontemporal == 1) return g_nt_store.exchange(nontemporal);
  return g_nt_store.load();
}

int gm_probe_memtest_fill(void* ptr, uint64_t bytes, uint32_t pattern, int invert, uint64_t seed,
                          uint32_t pass, uint64_t base_offset, void* stream) {
  if (!buffer_ok(ptr, bytes, pattern, base_offset)) return (int)hipErrorInvalidValue;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass};
  return launch(kWrite, pattern, cus, (hipStream_t)stream, ptr, bytes, a, nullptr);
}

int gm_probe_memtest_verify(void* ptr, uint64_t bytes, uint32_t pattern, int invert,
                            int write_inverse, uint64_t seed, uint32_t pass,
                            uint64_t base_offset, void* stream, gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!buffer_ok(ptr, bytes, pattern, base_offset)) return (int)hipErrorInvalidValue;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  hipStream_t s = (hipStream_t)stream;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass};
  return checked_launch(s, bytes, out, [&](DevResult* res) {
    return launch(write_inverse ? kCheckInvert : kCheck, pattern, cus, s, ptr, bytes, a, res);
  });
}

int gm_probe_memtest(int dev, uint64_t bytes, uint64_t chunk_bytes, uint32_t pattern_mask,
                     int passes, uint64_t seed, uint64_t flip_offset, uint64_t flip_mask,
                     gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (bytes == 0 || (bytes & 15) || (chunk_bytes & 15) || pattern_mask == 0 ||
      (pattern_mask & ~(uint32_t)GM_MEMTEST_ALL) || passes <= 0)
    return (int)hipErrorInvalidValue;
  if (flip_mask && ((flip_offset & 7) || flip_offset + 8 > bytes || flip_offset + 8 < 8))
    return (int)hipErrorInvalidValue;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  int cus = 0;
  if (int e = current_cus(&cus)) return e;
  const double t0 = now_s();
  if (chunk_bytes == 0) chunk_bytes = 8ull << 30;

  // the region: allocations of at most chunk_bytes, each with its global base offset
  std::deque<Piece> pieces;  // a deque never relocates its owning elements
  uint64_t have = 0;
  hipError_t alloc_err = hipSuccess;
  while (have < bytes) {
    uint64_t want = bytes - have < chunk_bytes ? bytes - have : chunk_bytes;
    const uint64_t floor = want < (256ull << 20) ? want : (256ull << 20);
    pieces.emplace_back();
    Piece& p = pieces.back();
    for (;;) {
      alloc_err = p.buf.alloc(want);
      if (alloc_err == hipSuccess) break;
      (void)hipGetLastError();
      p.buf.p = nullptr;
      want = (want / 2) & ~15ull;
      if (want < floor) break;
    }
    if (alloc_err != hipSuccess) {
      pieces.pop_back();
      break;
    }
    p.bytes = want;
    p.base = have;
    have += want;
  }
  if (pieces.empty()) return (int)(alloc_err != hipSuccess ? alloc_err : hipErrorOutOfMemory);

  DevBuf dres;
  GM_CHECK(dres.alloc(sizeof(DevResult)));
  GM_CHECK(hipMemset(dres.p, 0, sizeof(DevResult)));
  Events ev;
  GM_CHECK(ev.create());
  {
    // untimed first launch: the code object is loaded here, not between a timed pair of events
    const uint64_t warm = pieces[0].bytes < 65536 ? pieces[0].bytes : 65536;
    if (int e = launch(kWrite, GM_MEMTEST_SOLID, cus, nullptr, pieces[0].buf.p, warm,
                       Args{0, seed, 0, 0}, nullptr))
      return e;
    GM_CHECK(hipStreamSynchronize(nullptr));
  }
  double ms_kind[3] = {0, 0, 0};
  uint64_t launches_kind[3] = {0, 0, 0};  // whole-region sweeps per kind

  // one sweep of the whole region with one kind of kernel, timed by an event pair
  auto sweep = [&](int mode, uint32_t pattern, bool invert, uint32_t pass) -> int {
    int e = (int)hipEventRecord(ev.e0, nullptr);
    for (size_t k = 0; k < pieces.size() && !e; ++k) {
      const Args a{pieces[k].base, seed, invert ? ~0ull : 0ull, pass};
      e = launch(mode, pattern, cus, nullptr, pieces[k].buf.p, pieces[k].bytes, a,
                 (DevResult*)dres.p);
    }
    if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
    if (!e) e = (int)hipEventSynchronize(ev.e1);
    float ms = 0;
    if (!e) e = elapsed_ms(ev.e0, ev.e1, &ms);
    ms_kind[mode] += ms;
    ++launches_kind[mode];
    return e;
  };
  auto flip = [&]() -> int {
    for (Piece& p : pieces) {
      if (flip_offset < p.base || flip_offset + 8 > p.base + p.bytes) continue;
      if (int e = xor_device_word((char*)p.buf.p + (flip_offset - p.base), flip_mask)) return e;
    }
    return 0;
  };

  int e = 0;
  for (uint32_t pattern = 1; pattern <= GM_MEMTEST_RANDOM && !e; pattern <<= 1) {
    if (!(pattern_mask & pattern)) continue;
    for (int pass = 0; pass < passes && !e; ++pass) {
      e = sweep(kWrite, pattern, false, (uint32_t)pass);
      if (!e && flip_mask) e = flip();
      if (!e) e = sweep(kCheckInvert, pattern, false, (uint32_t)pass);
      if (!e) e = sweep(kCheck, pattern, true, (uint32_t)pass);
    }
  }
  if (e) return e;
  DevResult h;
  GM_CHECK(hipMemcpy(&h, dres.p, sizeof(h), hipMemcpyDeviceToHost));
  export_errors(h, out);
  out->bytes_tested = have;
  out->allocations = (uint32_t)pieces.size();
  const double b = (double)have;
  if (ms_kind[kWrite] > 0) out->write_gbps = b * launches_kind[kWrite] / (ms_kind[kWrite] * 1e-3) / 1e9;
  if (ms_kind[kCheck] > 0)
    out->read_gbps = b * launches_kind[kCheck] / (ms_kind[kCheck] * 1e-3) / 1e9;
  if (ms_kind[kCheckInvert] > 0)
    out->rw_gbps = 2.0 * b * launches_kind[kCheckInvert] / (ms_kind[kCheckInvert] * 1e-3) / 1e9;
  out->seconds = now_s() - t0;
  return 0;
}

}  // extern "C"
