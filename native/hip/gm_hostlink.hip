// gm_hostlink.hip — host-link (PCIe) data and bandwidth test for gfx950: do bytes arrive intact
// between pinned host memory and the GPU, and how fast?
//
// Three kinds of launch of the pattern-stream kernel (gm_pattern_stream.h) walk pinned host
// memory through its device mapping:
//   kread   reads and checks every 64-bit word against the memtest pattern
//   kwrite  writes the pattern
//   kcopy   reads one host buffer, checks it, writes what it read to a second host buffer
// The link is narrow and latency-bound next to HBM, so the geometry is not memtest's: a caller-
// chosen number of 256-thread blocks (a few tens fill the link and leave the other CUs alone),
// U of 4 or 8, nontemporal accesses. Lane l of a wave touches base + 16 l: one wave-instruction
// is 1 KiB of contiguous host memory.
// The driver (gm_probe_hostlink) adds the copy-engine legs and the timing.
#include <atomic>

#include "gm_hostlink_host.h"
#include "gm_pattern_stream.h"

namespace {

constexpr int kDefaultUnroll = 8;
constexpr int kDefaultBlocks = 16;

std::atomic<int> g_unroll{kDefaultUnroll};

// `from` (kCheck, kCopy) and `to` (kWrite, kCopy) are device addresses of `bytes` each.
// Nontemporal stores, the negative control compiled in, U from gm_probe_hostlink_unroll.
int launch(int mode, uint32_t pattern, int blocks, hipStream_t s, const void* from, void* to,
           uint64_t bytes, const Args& a, DevResult* res) {
  const int u = g_unroll.load();
  const size_t n = bytes / 16;
  const StreamLaunch l{gm_pattern_chunks(n, (size_t)blocks, (size_t)u * 256), s,
                       mode == kCheck ? const_cast<void*>(from) : to, from, n, a, res};
  const bool known = dispatch_pattern(pattern, [&](auto p) {
    constexpr uint32_t P = decltype(p)::value;
    if (mode == kCheck)
      u == 4 ? l.run<P, kCheck, 4, true, true>() : l.run<P, kCheck, 8, true, true>();
    else if (mode == kWrite)
      u == 4 ? l.run<P, kWrite, 4, true, true>() : l.run<P, kWrite, 8, true, true>();
    else
      u == 4 ? l.run<P, kCopy, 4, true, true>() : l.run<P, kCopy, 8, true, true>();
  });
  return known ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

bool one_leg(uint32_t l) { return l != 0 && (l & (l - 1)) == 0 && (l & ~(uint32_t)GM_HOSTLINK_ALL) == 0; }

bool buffer_ok(const void* ptr, uint64_t bytes, uint32_t pattern, uint64_t base_offset,
               int blocks) {
  return buffer_ok(ptr, bytes, pattern, base_offset) && (uintptr_t)ptr + bytes >= (uintptr_t)ptr &&
         blocks >= 1 && blocks <= GM_HOSTLINK_MAX_BLOCKS;
}

// Device address of pinned host memory [host, host + bytes); an error for anything else.
int device_view(const void* host, uint64_t bytes, void** dev) {
  const char* ends[2] = {(const char*)host, (const char*)host + bytes - 1};
  for (const char* p : ends) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return (int)e;
    }
    if (at.type != hipMemoryTypeHost) return (int)hipErrorInvalidValue;
  }
  *dev = nullptr;
  GM_CHECK(hipHostGetDevicePointer(dev, const_cast<void*>(host), 0));
  return *dev ? 0 : (int)hipErrorInvalidValue;
}

const char* const kLegNames[GM_HOSTLINK_LEGS] = {"h2d", "d2h", "bidir", "kread", "kwrite", "kduplex"};

// Everything one call of the driver holds.
struct Run {
  uint64_t bytes = 0, seed = 0, flip_offset = 0, flip_mask = 0;
  uint32_t flip_leg = 0;
  int iters = 1, blocks = kDefaultBlocks;
  PinnedBuf ha, hb;
  DevBuf da, db, dres, dscratch;
  void *ha_dev = nullptr, *hb_dev = nullptr;
  Stream s1, s2;
  Event start, end1, end2;
  gm_hostlink_result_t* out = nullptr;
  double host_s = 0;

  uint64_t words() const { return bytes / 8; }
  bool flips(uint32_t leg) const { return flip_mask != 0 && flip_leg == leg; }

  void add_record(uint32_t leg, uint32_t pattern, uint32_t pass, uint64_t o, uint64_t e,
                  uint64_t g) {
    if (out->records_filled >= GM_HOSTLINK_MAX_RECORDS) return;
    gm_hostlink_record_t* r = &out->records[out->records_filled++];
    r->offset = o;
    r->expected = e;
    r->got = g;
    r->leg = leg;
    r->pattern = pattern;
    r->pass = pass;
  }
  void add_errors(uint32_t leg, gm_hostlink_leg_t* side, uint64_t w, uint64_t bits,
                  uint64_t stuck) {
    int idx = 0;
    while ((1u << idx) != leg) ++idx;
    out->legs[idx].words_in_error += w;
    if (side) side->words_in_error += w;
    out->words_in_error += w;
    out->bit_errors += bits;
    out->stuck_mask |= stuck;
  }
  void add_time(gm_hostlink_leg_t* l, uint64_t moved, float ms) {
    l->bytes += moved;
    l->ms += ms;
  }

  // host compare of hb against P
  void host_check(uint32_t leg, gm_hostlink_leg_t* side, uint32_t pattern, uint32_t pass) {
    const double t = now_s();
    gm_hl_host_cmp_t c;
    gm_hl_host_compare((const uint64_t*)hb.p, words(), pattern, 0, seed, pass, 0, &c);
    host_s += now_s() - t;
    add_errors(leg, side, c.words, c.bits, c.stuck);
    for (uint32_t i = 0; i < c.records_filled; ++i)
      add_record(leg, pattern, pass, c.offset[i], c.expected[i], c.got[i]);
  }
  void take(uint32_t leg, gm_hostlink_leg_t* side, const gm_memtest_result_t& r) {
    add_errors(leg, side, r.words_in_error, r.bit_errors, r.stuck_mask);
    for (uint32_t i = 0; i < r.records_filled; ++i)
      add_record(leg, r.records[i].pattern, r.records[i].pass, r.records[i].offset,
                 r.records[i].expected, r.records[i].got);
  }
  // device verify of db against P
  int device_check(uint32_t leg, gm_hostlink_leg_t* side, uint32_t pattern, uint32_t pass) {
    gm_memtest_result_t r;
    if (int e = gm_probe_memtest_verify(db.p, bytes, pattern, 0, 0, seed, pass, 0, s1.s, &r))
      return e;
    take(leg, side, r);
    return 0;
  }
  // what the last checked kernel launch booked in dres
  int kernel_check(uint32_t leg, hipStream_t s) {
    DevResult h;
    GM_CHECK(hipMemcpyAsync(&h, dres.p, sizeof(h), hipMemcpyDeviceToHost, s));
    GM_CHECK(hipStreamSynchronize(s));
    gm_memtest_result_t r;
    memset(&r, 0, sizeof(r));
    export_errors(h, &r);
    take(leg, nullptr, r);
    return 0;
  }

  void host_fill(uint32_t pattern, uint32_t pass) {
    const double t = now_s();
    gm_hl_host_fill((uint64_t*)ha.p, words(), pattern, 0, seed, pass, 0);
    host_s += now_s() - t;
  }
  void host_poison() {
    const double t = now_s();
    gm_hl_host_poison((uint64_t*)hb.p, words(), 0xA5);
    host_s += now_s() - t;
  }
  void flip_host_source() { ((uint64_t*)ha.p)[flip_offset / 8] ^= flip_mask; }
  int flip_device_source() { return xor_device_word((char*)da.p + flip_offset, flip_mask); }
  // db = ~P, da = P (device side, as the HBM test does it)
  int device_poison(uint32_t pattern, uint32_t pass) {
    if (int e = gm_probe_memtest_fill(db.p, bytes, pattern, 1, seed, pass, 0, s1.s)) return e;
    return (int)hipStreamSynchronize(s1.s);
  }
  int device_source(uint32_t pattern, uint32_t pass) {
    if (int e = gm_probe_memtest_fill(da.p, bytes, pattern, 0, seed, pass, 0, s1.s)) return e;
    return (int)hipStreamSynchronize(s1.s);
  }

  // `iters` repeats of op(k) on s1 between two events, after one untimed op(-1).
  template <class Op>
  int timed(gm_hostlink_leg_t* l, uint64_t moved_per_iter, Op op) {
    if (int e = op(-1)) return e;
    GM_CHECK(hipStreamSynchronize(s1.s));
    GM_CHECK(hipEventRecord(start.e, s1.s));
    for (int k = 0; k < iters; ++k)
      if (int e = op(k)) return e;
    GM_CHECK(hipEventRecord(end1.e, s1.s));
    GM_CHECK(hipEventSynchronize(end1.e));
    float ms = 0;
    if (int e = elapsed_ms(start.e, end1.e, &ms)) return e;
    add_time(l, moved_per_iter * (uint64_t)iters, ms);
    return 0;
  }

  Args args(uint32_t pass, bool flip) const {
    return Args{0, seed, 0, pass, flip ? flip_offset : 0, flip ? flip_mask : 0};
  }
  // the result of the last timed launch (k == iters - 1) is the one that counts
  DevResult* result_for(int k) const {
    return (DevResult*)(k == iters - 1 ? dres.p : dscratch.p);
  }

  int leg_h2d(uint32_t pattern, uint32_t pass) {
    if (flips(GM_HOSTLINK_H2D)) flip_host_source();
    int e = device_poison(pattern, pass);
    if (!e)
      e = timed(&out->legs[0], bytes, [&](int) {
        return (int)hipMemcpyAsync(db.p, ha.p, bytes, hipMemcpyHostToDevice, s1.s);
      });
    if (flips(GM_HOSTLINK_H2D)) flip_host_source();
    return e ? e : device_check(GM_HOSTLINK_H2D, nullptr, pattern, pass);
  }
  int leg_d2h(uint32_t pattern, uint32_t pass) {
    if (int e = device_source(pattern, pass)) return e;
    if (flips(GM_HOSTLINK_D2H))
      if (int e = flip_device_source()) return e;
    host_poison();
    if (int e = timed(&out->legs[1], bytes, [&](int) {
          return (int)hipMemcpyAsync(hb.p, da.p, bytes, hipMemcpyDeviceToHost, s1.s);
        }))
      return e;
    host_check(GM_HOSTLINK_D2H, nullptr, pattern, pass);
    return 0;
  }
  int leg_bidir(uint32_t pattern, uint32_t pass) {
    if (int e = device_source(pattern, pass)) return e;
    if (int e = device_poison(pattern, pass)) return e;
    host_poison();
    const bool f = flips(GM_HOSTLINK_BIDIR);
    if (f) flip_host_source();
    auto both = [&]() -> int {
      GM_CHECK(hipMemcpyAsync(db.p, ha.p, bytes, hipMemcpyHostToDevice, s1.s));
      GM_CHECK(hipMemcpyAsync(hb.p, da.p, bytes, hipMemcpyDeviceToHost, s2.s));
      return 0;
    };
    auto run = [&]() -> int {
      if (int e = both()) return e;
      GM_CHECK(hipStreamSynchronize(s1.s));
      GM_CHECK(hipStreamSynchronize(s2.s));
      // one start for both streams: s2 does not begin before s1's start event
      GM_CHECK(hipEventRecord(start.e, s1.s));
      GM_CHECK(hipStreamWaitEvent(s2.s, start.e, 0));
      for (int k = 0; k < iters; ++k)
        if (int e = both()) return e;
      GM_CHECK(hipEventRecord(end1.e, s1.s));
      GM_CHECK(hipEventRecord(end2.e, s2.s));
      GM_CHECK(hipEventSynchronize(end1.e));
      GM_CHECK(hipEventSynchronize(end2.e));
      float m1 = 0, m2 = 0;
      if (int e = elapsed_ms(start.e, end1.e, &m1)) return e;
      if (int e = elapsed_ms(start.e, end2.e, &m2)) return e;
      const uint64_t moved = bytes * (uint64_t)iters;
      add_time(&out->bidir_h2d, moved, m1);
      add_time(&out->bidir_d2h, moved, m2);
      add_time(&out->legs[2], 2 * moved, m1 > m2 ? m1 : m2);
      return 0;
    };
    const int e = run();
    if (e) {  // nothing may still be writing the buffers when they are freed
      (void)hipStreamSynchronize(s1.s);
      (void)hipStreamSynchronize(s2.s);
    }
    if (f) flip_host_source();
    if (e) return e;
    if (int e2 = device_check(GM_HOSTLINK_BIDIR, &out->bidir_h2d, pattern, pass)) return e2;
    host_check(GM_HOSTLINK_BIDIR, &out->bidir_d2h, pattern, pass);
    return 0;
  }
  int leg_kernel(uint32_t leg, int idx, int mode, uint32_t pattern, uint32_t pass) {
    const bool f = flips(leg);
    const bool reads = mode != kWrite, writes = mode != kCheck;
    if (f && mode == kCheck) flip_host_source();
    if (writes) host_poison();
    int e = 0;
    if (reads) {
      e = (int)hipMemsetAsync(dres.p, 0, sizeof(DevResult), s1.s);
      if (!e) e = (int)hipMemsetAsync(dscratch.p, 0, sizeof(DevResult), s1.s);
    }
    const Args a = args(pass, f && writes);
    if (!e)
      e = timed(&out->legs[idx], bytes * (reads && writes ? 2 : 1), [&](int k) {
        return launch(mode, pattern, blocks, s1.s, ha_dev, hb_dev, bytes, a, result_for(k));
      });
    if (e) (void)hipStreamSynchronize(s1.s);
    if (f && mode == kCheck) flip_host_source();
    if (e) return e;
    if (reads)
      if (int e2 = kernel_check(leg, s1.s)) return e2;
    if (writes) host_check(leg, nullptr, pattern, pass);
    return 0;
  }
};

int set_stage(gm_hostlink_result_t* out, const char* stage, int err) {
  memset(out->stage, 0, sizeof(out->stage));
  if (err) strncpy(out->stage, stage, sizeof(out->stage) - 1);
  return err;
}

}  // namespace

extern "C" {

int gm_probe_hostlink_geometry(uint32_t* step_bytes, uint32_t* default_blocks) {
  if (step_bytes) *step_bytes = (uint32_t)g_unroll.load() * 256u * 16u;
  if (default_blocks) *default_blocks = kDefaultBlocks;
  return 0;
}

int gm_probe_hostlink_unroll(int u) {
  if (u == 4 || u == 8) return g_unroll.exchange(u);
  return g_unroll.load();
}

int gm_probe_hostlink_kwrite(void* host_ptr, uint64_t bytes, uint32_t pattern, int invert,
                             uint64_t seed, uint32_t pass, uint64_t base_offset, int blocks,
                             uint64_t flip_offset, uint64_t flip_mask, void* stream) {
  if (!buffer_ok(host_ptr, bytes, pattern, base_offset, blocks) || (flip_offset & 7))
    return (int)hipErrorInvalidValue;
  void* dev = nullptr;
  if (int e = device_view(host_ptr, bytes, &dev)) return e;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass, flip_offset, flip_mask};
  return launch(kWrite, pattern, blocks, (hipStream_t)stream, nullptr, dev, bytes, a, nullptr);
}

int gm_probe_hostlink_kread(const void* host_ptr, uint64_t bytes, uint32_t pattern, int invert,
                            uint64_t seed, uint32_t pass, uint64_t base_offset, int blocks,
                            void* stream, gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!buffer_ok(host_ptr, bytes, pattern, base_offset, blocks)) return (int)hipErrorInvalidValue;
  void* dev = nullptr;
  if (int e = device_view(host_ptr, bytes, &dev)) return e;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass};
  hipStream_t s = (hipStream_t)stream;
  return checked_launch(s, bytes, out, [&](DevResult* res) {
    return launch(kCheck, pattern, blocks, s, dev, nullptr, bytes, a, res);
  });
}

int gm_probe_hostlink_kcopy(const void* src_host, void* dst_host, uint64_t bytes, uint32_t pattern,
                            int invert, uint64_t seed, uint32_t pass, uint64_t base_offset,
                            int blocks, uint64_t flip_offset, uint64_t flip_mask, void* stream,
                            gm_memtest_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (!buffer_ok(src_host, bytes, pattern, base_offset, blocks) ||
      !buffer_ok(dst_host, bytes, pattern, base_offset, blocks) || (flip_offset & 7))
    return (int)hipErrorInvalidValue;
  const uintptr_t sa = (uintptr_t)src_host, da = (uintptr_t)dst_host;
  if (sa < da + bytes && da < sa + bytes) return (int)hipErrorInvalidValue;
  void *sdev = nullptr, *ddev = nullptr;
  if (int e = device_view(src_host, bytes, &sdev)) return e;
  if (int e = device_view(dst_host, bytes, &ddev)) return e;
  const Args a{base_offset, seed, invert ? ~0ull : 0ull, pass, flip_offset, flip_mask};
  hipStream_t s = (hipStream_t)stream;
  return checked_launch(s, bytes, out, [&](DevResult* res) {
    return launch(kCopy, pattern, blocks, s, sdev, ddev, bytes, a, res);
  });
}

int gm_probe_hostlink(int dev, uint64_t bytes, uint32_t legs_mask, uint32_t pattern_mask,
                      int passes, int iters, int blocks, uint64_t seed, uint32_t flip_leg,
                      uint64_t flip_offset, uint64_t flip_mask, gm_hostlink_result_t* out) {
  if (!out) return (int)hipErrorInvalidValue;
  memset(out, 0, sizeof(*out));
  if (dev < 0 || bytes == 0 || (bytes & 15) || legs_mask == 0 ||
      (legs_mask & ~(uint32_t)GM_HOSTLINK_ALL) || pattern_mask == 0 ||
      (pattern_mask & ~(uint32_t)GM_MEMTEST_ALL) || passes <= 0 || iters < 1 || iters > 1024 ||
      blocks < 0 || blocks > GM_HOSTLINK_MAX_BLOCKS)
    return set_stage(out, "args", (int)hipErrorInvalidValue);
  if (flip_mask && (!one_leg(flip_leg) || !(flip_leg & legs_mask) || (flip_offset & 7) ||
                    flip_offset + 8 > bytes || flip_offset + 8 < 8))
    return set_stage(out, "args", (int)hipErrorInvalidValue);
  DeviceGuard g(dev);
  if (!g.ok) return set_stage(out, "device", (int)hipErrorInvalidDevice);
  const double t0 = now_s();

  Run r;
  r.out = out;
  r.bytes = bytes;
  r.seed = seed;
  r.iters = iters;
  r.blocks = blocks ? blocks : kDefaultBlocks;
  r.flip_leg = flip_leg;
  r.flip_offset = flip_offset;
  r.flip_mask = flip_mask;
  out->bytes = bytes;
  for (PinnedBuf* b : {&r.ha, &r.hb}) {
    const hipError_t e = b->alloc(bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      b->p = nullptr;
      return set_stage(out, "pin", (int)e);
    }
    out->pinned_bytes += bytes;
  }
  for (DevBuf* b : {&r.da, &r.db}) {
    const hipError_t e = b->alloc(bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      b->p = nullptr;
      return set_stage(out, "alloc", (int)e);
    }
  }
  int e = (int)r.dres.alloc(sizeof(DevResult));
  if (!e) e = (int)r.dscratch.alloc(sizeof(DevResult));
  if (!e) e = (int)r.s1.create();
  if (!e) e = (int)r.s2.create();
  if (!e) e = (int)r.start.create();
  if (!e) e = (int)r.end1.create();
  if (!e) e = (int)r.end2.create();
  if (!e) e = (int)hipHostGetDevicePointer(&r.ha_dev, r.ha.p, 0);
  if (!e) e = (int)hipHostGetDevicePointer(&r.hb_dev, r.hb.p, 0);
  if (e) return set_stage(out, "setup", e);
  out->setup_seconds = now_s() - t0;

  const char* stage = "";
  for (uint32_t pattern = 1; pattern <= GM_MEMTEST_RANDOM && !e; pattern <<= 1) {
    if (!(pattern_mask & pattern)) continue;
    for (int pass = 0; pass < passes && !e; ++pass) {
      const uint32_t ps = (uint32_t)pass;
      r.host_fill(pattern, ps);
      for (int idx = 0; idx < GM_HOSTLINK_LEGS && !e; ++idx) {
        const uint32_t leg = 1u << idx;
        if (!(legs_mask & leg)) continue;
        stage = kLegNames[idx];
        switch (leg) {
          case GM_HOSTLINK_H2D: e = r.leg_h2d(pattern, ps); break;
          case GM_HOSTLINK_D2H: e = r.leg_d2h(pattern, ps); break;
          case GM_HOSTLINK_BIDIR: e = r.leg_bidir(pattern, ps); break;
          case GM_HOSTLINK_KREAD: e = r.leg_kernel(leg, idx, kCheck, pattern, ps); break;
          case GM_HOSTLINK_KWRITE: e = r.leg_kernel(leg, idx, kWrite, pattern, ps); break;
          default: e = r.leg_kernel(leg, idx, kCopy, pattern, ps); break;
        }
      }
    }
  }
  if (e) {
    (void)hipDeviceSynchronize();  // the buffers are freed on return
    return set_stage(out, stage, e);
  }
  out->legs_run = legs_mask;
  gm_hostlink_leg_t* all[GM_HOSTLINK_LEGS + 2] = {&out->legs[0], &out->legs[1], &out->legs[2],
                                                  &out->legs[3], &out->legs[4], &out->legs[5],
                                                  &out->bidir_h2d, &out->bidir_d2h};
  for (gm_hostlink_leg_t* l : all)
    if (l->ms > 0) l->gbps = (double)l->bytes / (l->ms * 1e-3) / 1e9;
  out->seconds = now_s() - t0;
  out->host_seconds = r.host_s;
  out->transfer_seconds = out->seconds - r.host_s - out->setup_seconds;
  return set_stage(out, "", 0);
}

}  // extern "C"
