// gm_gemm_shared.h — what the two burn-in GEMMs (gm_gemm.hip: bf16, gm_mxgemm.hip: block-scaled
// fp8 / fp4) share: the XCD-aware block → tile map, the compare kernel and the bit-exact burn-in
// loop with its flip control; and for the attributed burn-in the traced blocks' bookkeeping, the
// per-tile compare and the traced loop. In an anonymous namespace, like gm_probe_common.h: each
// translation unit gets its own copy.
#pragma once

#include <stddef.h>

#include "gm_burnin_attr.h"
#include "gm_probe_common.h"
#include "gm_where.h"

namespace {

// XCD-aware block → output tile (gm_gemm_tile_map, gm_burnin_attr.h) of this block. r = 0, the
// default and a constant in the plain kernels, folds away; the traced kernels pass the
// iteration's rotation, 0 <= r < gridDim.x.
template <int TM, int TN, int kGroupM>
__device__ __forceinline__ void gemm_tile_of(int M, int N, int& tm, int& tn, int r = 0) {
  gm_gemm_tile_map<TM, TN, kGroupM>((int)blockIdx.x, (int)gridDim.x, M, N, r, tm, tn);
}

// What a traced GEMM takes besides its operands: the rotation, where each block stores the id
// of the CU it ran on, and the injection (mask 0: none). The injected id is inj_id or, where
// inj_id_at is set, the word there: the burn-in's `first` is an entry of the warm-up's CU map,
// read on the device, so no host round trip stands between the warm-up and the loop.
struct GemmTrace {
  int r;
  uint32_t* cu_of_tile;
  const uint32_t* inj_id_at;
  uint32_t inj_id, inj_mask;
};

// A traced block's bookkeeping, once its tile is known: thread 0 (lane 0 of wave 0, the owner
// of the tile's element (0, 0) in the 16x16 epilogue map) stores the block's CU id under the
// tile. Returns what this thread XORs into the bf16 bits of element (0, 0) on their way out:
// the injection's mask in thread 0 of a block on the injected CU, else 0.
__device__ __forceinline__ uint32_t trace_block(const GemmTrace& tr, int tile) {
  const uint32_t id = where_am_i().id;
  if (threadIdx.x != 0) return 0;
  tr.cu_of_tile[tile] = id;
  if (tr.inj_mask == 0) return 0;
  return id == (tr.inj_id_at ? *tr.inj_id_at : tr.inj_id) ? tr.inj_mask : 0;
}

// bf16(v) with `flip` XORed into its bits.
__device__ __forceinline__ __bf16 bf16_flipped(float v, uint32_t flip) {
  const __bf16 b = (__bf16)v;
  const uint16_t bits = (uint16_t)(__builtin_bit_cast(uint16_t, b) ^ flip);
  return __builtin_bit_cast(__bf16, bits);
}

// Number of 16-B words that differ between a and b: one ballot + popcount per wave, one
// atomic per wave.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_count_diff(const u32x4* __restrict__ a,
                                                    const u32x4* __restrict__ b, size_t n,
                                                    unsigned long long* count) {
  unsigned long long local = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const u32x4 x = __builtin_nontemporal_load(&a[i]), y = __builtin_nontemporal_load(&b[i]);
    local += (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, kWave);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(count, local);
}

// The one launch of the compare kernel: the burn-in loop and gm_probe_count_diff share it.
inline int launch_count_diff(const void* a, const void* b, size_t vec, void* count, hipStream_t s) {
  hipLaunchKernelGGL(k_count_diff, dim3(2048), dim3(256), 0, s, (const u32x4*)a, (const u32x4*)b,
                     vec, (unsigned long long*)count);
  return (int)hipGetLastError();
}

// The flips of a burn-in over an n × n bf16 result: in range, nonzero masks, no element twice.
inline bool burn_in_flips_ok(size_t elems, int n_flips, const uint64_t* flip_elems,
                             const uint16_t* flip_masks) {
  if (n_flips < 0 || (n_flips > 0 && (!flip_elems || !flip_masks))) return false;
  for (int i = 0; i < n_flips; ++i) {
    if (flip_elems[i] >= elems || flip_masks[i] == 0) return false;
    for (int j = 0; j < i; ++j)  // a repeated element could cancel its own flip
      if (flip_elems[j] == flip_elems[i]) return false;
  }
  return true;
}

// The burn-in proper, on the current device with the operands already filled: gemm(c) launches
// one n³ GEMM into the n × n bf16 buffer c on the null stream and returns a HIP error code. The
// first result is the reference; the flips are applied to it; every later result is compared with
// it. *tflops counts 2 n³ per GEMM over the wall time, compare kernels included.
template <class Gemm>
int burn_in_loop(int n, double seconds, int n_flips, const uint64_t* flip_elems,
                 const uint16_t* flip_masks, Gemm gemm, double* tflops, uint64_t* mismatches,
                 int* iters) {
  const size_t elems = (size_t)n * n;
  DevBuf dref, dc, dcount;
  GM_CHECK(dref.alloc(elems * 2));
  GM_CHECK(dc.alloc(elems * 2));
  GM_CHECK(dcount.alloc(sizeof(unsigned long long)));
  GM_CHECK(hipMemset(dcount.p, 0, sizeof(unsigned long long)));
  int e = gemm(dref.p);  // the reference result
  if (e) return e;
  // Negative control: corrupt the finished reference, through the host like the memtest's flip.
  // The blocking copies on the null stream wait for the GEMM; the loop below is untouched.
  for (int i = 0; i < n_flips; ++i) {
    uint16_t* at = (uint16_t*)dref.p + flip_elems[i];
    uint16_t v = 0;
    GM_CHECK(hipMemcpy(&v, at, sizeof(v), hipMemcpyDeviceToHost));
    v ^= flip_masks[i];
    GM_CHECK(hipMemcpy(at, &v, sizeof(v), hipMemcpyHostToDevice));
  }
  Events ev;
  GM_CHECK(ev.create());
  GM_CHECK(hipEventRecord(ev.e0, nullptr));
  const double t0 = now_s();
  const size_t vec = elems / 8;  // 16-B compares
  int done = 0;
  // Batches of 8 GEMMs, each result compared bit-for-bit with the first one: the kernel is
  // deterministic (fixed reduction order, no atomics), so any difference is a hardware fault.
  while (!e) {
    for (int i = 0; i < 8 && !e; ++i) {
      e = gemm(dc.p);
      if (!e) e = launch_count_diff(dc.p, dref.p, vec, dcount.p, nullptr);
      ++done;
    }
    if (!e) e = (int)hipDeviceSynchronize();
    const double el = now_s() - t0;
    if (el >= seconds) break;
  }
  if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
  if (!e) e = (int)hipEventSynchronize(ev.e1);
  float ms = 0;
  if (!e) e = elapsed_ms(ev.e0, ev.e1, &ms);
  unsigned long long bad = 0;
  if (!e) e = (int)hipMemcpy(&bad, dcount.p, sizeof(bad), hipMemcpyDeviceToHost);
  if (e) return e;
  *iters = done;
  *mismatches = bad;
  // compare kernels are included in the wall time; they move 2 × n² × 2 B per GEMM (about 2 %
  // of a bf16 GEMM's time at 8192³, more of the shorter MX ones: profiles/mxgemm/)
  if (ms > 0) *tflops = 2.0 * n * (double)n * n * done / (ms * 1e-3) / 1e12;
  return 0;
}

// ------------------------------------------------------------------ attributed burn-in
// (contract: gm_probe.h, "attributed burn-in")

// What the per-tile compare accumulates over a run: gm_burnin_state_t (gm_probe.h) with the
// total as the type atomicAdd takes.
struct AttrState {
  unsigned long long total;  // differing 16-B words, k_count_diff's unit and total
  uint32_t cursor, pad;      // events so far; the first GM_BURNIN_LOG_CAP of them are in log[]
  gm_burnin_event_t log[GM_BURNIN_LOG_CAP];
};
static_assert(sizeof(AttrState) == sizeof(gm_burnin_state_t) &&
                  offsetof(AttrState, total) == offsetof(gm_burnin_state_t, total) &&
                  offsetof(AttrState, cursor) == offsetof(gm_burnin_state_t, cursor) &&
                  offsetof(AttrState, log) == offsetof(gm_burnin_state_t, log),
              "the published layout is the kernel's");

// The per-tile maps of a run, device pointers: tiles entries each, seen GM_CUSCAN_IDS.
struct AttrMaps {
  const uint32_t *cu, *ref_cu;  // this iteration's CU of every tile, the reference's
  uint32_t *exonerated, *moved, *seen;
};

// One block per 256 × 256 bf16 tile of the n × n results a and b (b the reference): the tile's
// differing 16-B words, 32 per row. Thread 0 then books the tile. Plain stores of 1 for the three
// marks (every writer stores the same value); atomics only on the total and the log cursor.
// An id of GM_CUSCAN_IDS or more in either map (0xFFFFFFFF: the block stored nothing) is no CU:
// the tile marks nothing in seen, and its event carries the ids as read, for the host to refuse.
__global__ __launch_bounds__(256) void k_count_diff_tiles(const u32x4* __restrict__ a,
                                                          const u32x4* __restrict__ b, int n,
                                                          uint32_t iteration, AttrMaps maps,
                                                          AttrState* st) {
  constexpr int kRowWords = kBurninTile / 8;  // 16-B words of one tile row
  __shared__ uint32_t wave_sum[4];
  const int ntn = n / kBurninTile, tile = blockIdx.x;
  const size_t row_words = (size_t)n / 8;
  const size_t base =
      (size_t)(tile / ntn) * kBurninTile * row_words + (size_t)(tile % ntn) * kRowWords;
  uint32_t local = 0;
  for (int w = threadIdx.x; w < kBurninTile * kRowWords; w += blockDim.x) {
    const size_t i = base + (size_t)(w / kRowWords) * row_words + (w % kRowWords);
    const u32x4 x = __builtin_nontemporal_load(&a[i]), y = __builtin_nontemporal_load(&b[i]);
    local += (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
  }
  for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, kWave);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t words = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
  const uint32_t cu = maps.cu[tile], ref = maps.ref_cu[tile];
  if (cu < GM_CUSCAN_IDS && ref < GM_CUSCAN_IDS) maps.seen[cu] = 1;
  if (cu != ref) maps.moved[tile] = 1;
  if (words == 0) {
    if (cu != ref) maps.exonerated[tile] = 1;  // another CU reproduced the reference's bits
    return;
  }
  atomicAdd(&st->total, (unsigned long long)words);
  const uint32_t slot = atomicAdd(&st->cursor, 1u);
  if (slot < GM_BURNIN_LOG_CAP)
    st->log[slot] = gm_burnin_event_t{iteration, (uint32_t)tile, cu, ref, words};
}

// The one launch of the per-tile compare, one block per tile of the n × n results: the traced
// loop and gm_probe_count_diff_tiles share it.
inline int launch_count_diff_tiles(const void* a, const void* b, int n, uint32_t iteration,
                                   const AttrMaps& maps, void* state, hipStream_t s) {
  const int tiles = (n / kBurninTile) * (n / kBurninTile);
  hipLaunchKernelGGL(k_count_diff_tiles, dim3(tiles), dim3(256), 0, s, (const u32x4*)a,
                     (const u32x4*)b, n, iteration, maps, (AttrState*)state);
  return (int)hipGetLastError();
}

// The injection of an attributed burn-in, checked: NULL, or an id and a 16-bit mask.
inline bool burn_in_inject_ok(const gm_burnin_inject_t* in) {
  return !in || (in->mask >= 1 && in->mask <= 0xFFFF && (in->first || in->id < GM_CUSCAN_IDS));
}

// burn_in_loop's sibling: gemm(c, trace) launches one traced n³ GEMM on the null stream.
template <class Gemm>
int burn_in_attr_loop(int n, double seconds, int n_flips, const uint64_t* flip_elems,
                      const uint16_t* flip_masks, const gm_burnin_inject_t* inject, Gemm gemm,
                      double* tflops, uint64_t* mismatches, int* iters, gm_burnin_attr_t* attr,
                      gm_burnin_blamed_t* blamed, int blamed_cap) {
  const size_t elems = (size_t)n * n;
  const int tiles = (n / kBurninTile) * (n / kBurninTile), grid = tiles;
  const int step = gm_burnin_step(grid);
  const size_t map_bytes = (size_t)tiles * sizeof(uint32_t);
  const size_t seen_bytes = GM_CUSCAN_IDS * sizeof(uint32_t);
  DevBuf dref, dc, dst, dcu, dref_cu, dwarm, dexon, dmoved, dseen;
  GM_CHECK(dref.alloc(elems * 2));
  GM_CHECK(dc.alloc(elems * 2));
  GM_CHECK(dst.alloc(sizeof(AttrState)));
  GM_CHECK(dcu.alloc(map_bytes));
  GM_CHECK(dref_cu.alloc(map_bytes));
  GM_CHECK(dwarm.alloc(map_bytes));
  GM_CHECK(dexon.alloc(map_bytes));
  GM_CHECK(dmoved.alloc(map_bytes));
  GM_CHECK(dseen.alloc(seen_bytes));
  GM_CHECK(hipMemset(dst.p, 0, sizeof(AttrState)));
  GM_CHECK(hipMemset(dcu.p, 0xFF, map_bytes));
  GM_CHECK(hipMemset(dref_cu.p, 0xFF, map_bytes));
  GM_CHECK(hipMemset(dwarm.p, 0xFF, map_bytes));
  GM_CHECK(hipMemset(dexon.p, 0, map_bytes));
  GM_CHECK(hipMemset(dmoved.p, 0, map_bytes));
  GM_CHECK(hipMemset(dseen.p, 0, seen_bytes));

  // Warm-up, outside the timing and without the injection: one whole iteration, GEMM and
  // compare (of its result with itself: no word differs, and its map is its own reference, so
  // it marks nothing but the CUs it saw). It loads both kernels' code and leaves `first`, the CU
  // of its tile 0, in dwarm[0], where the injection reads it on the device. From here on the
  // stream holds GEMM, compare, GEMM, compare ... without a host round trip in between (the
  // flips' copies apart), the sequence of launches the timed loop continues. The compare goes
  // through launch_count_diff_tiles, the launch gm_probe_count_diff_tiles is tested through.
  const auto compare = [&](const void* c, const void* cu, const void* ref_cu, uint32_t iteration) {
    const AttrMaps maps{(const uint32_t*)cu, (const uint32_t*)ref_cu, (uint32_t*)dexon.p,
                        (uint32_t*)dmoved.p, (uint32_t*)dseen.p};
    return launch_count_diff_tiles(c, dref.p, n, iteration, maps, dst.p, nullptr);
  };
  GemmTrace tr{0, (uint32_t*)dwarm.p, nullptr, 0, 0};
  int e = gemm(dref.p, tr);
  if (!e) e = compare(dref.p, dwarm.p, dwarm.p, 0);
  if (e) return e;
  if (inject) {
    if (inject->first) tr.inj_id_at = (const uint32_t*)dwarm.p;
    tr.inj_id = inject->id;
    tr.inj_mask = inject->mask;
  }
  // The reference result and its CU map, then the same compare: it books the reference's CUs.
  tr.cu_of_tile = (uint32_t*)dref_cu.p;
  e = gemm(dref.p, tr);
  if (!e) e = compare(dref.p, dref_cu.p, dref_cu.p, 0);
  if (e) return e;
  for (int i = 0; i < n_flips; ++i) {  // as in burn_in_loop
    uint16_t* at = (uint16_t*)dref.p + flip_elems[i];
    uint16_t v = 0;
    GM_CHECK(hipMemcpy(&v, at, sizeof(v), hipMemcpyDeviceToHost));
    v ^= flip_masks[i];
    GM_CHECK(hipMemcpy(at, &v, sizeof(v), hipMemcpyHostToDevice));
  }
  tr.cu_of_tile = (uint32_t*)dcu.p;
  Events ev;
  GM_CHECK(ev.create());
  GM_CHECK(hipEventRecord(ev.e0, nullptr));
  const double t0 = now_s();
  int done = 0;
  // Batches of 8 as in burn_in_loop; GEMM and compare in order on the one stream, so the next
  // GEMM overwrites the result and the CU map only after the compare has read them.
  while (!e) {
    for (int i = 0; i < 8 && !e; ++i) {
      tr.r = gm_burnin_rotation(grid, step, done + 1);
      e = gemm(dc.p, tr);
      if (!e) e = compare(dc.p, dcu.p, dref_cu.p, (uint32_t)(done + 1));
      ++done;
    }
    if (!e) e = (int)hipDeviceSynchronize();
    if (now_s() - t0 >= seconds) break;
  }
  if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
  if (!e) e = (int)hipEventSynchronize(ev.e1);
  float ms = 0;
  if (!e) e = elapsed_ms(ev.e0, ev.e1, &ms);
  if (e) return e;

  std::vector<unsigned char> raw(sizeof(AttrState));
  std::vector<uint32_t> exon(tiles), moved(tiles), seen(GM_CUSCAN_IDS);
  uint32_t first = 0;
  GM_CHECK(hipMemcpy(&first, dwarm.p, sizeof(first), hipMemcpyDeviceToHost));
  if (first >= GM_CUSCAN_IDS) return (int)hipErrorUnknown;  // tile 0's block stored no id
  GM_CHECK(hipMemcpy(raw.data(), dst.p, sizeof(AttrState), hipMemcpyDeviceToHost));
  GM_CHECK(hipMemcpy(exon.data(), dexon.p, map_bytes, hipMemcpyDeviceToHost));
  GM_CHECK(hipMemcpy(moved.data(), dmoved.p, map_bytes, hipMemcpyDeviceToHost));
  GM_CHECK(hipMemcpy(seen.data(), dseen.p, seen_bytes, hipMemcpyDeviceToHost));
  const AttrState* st = (const AttrState*)raw.data();
  std::vector<uint8_t> exonerated(tiles);
  for (int t = 0; t < tiles; ++t) exonerated[t] = exon[t] != 0;
  const GmBurninBlame blame = gm_burnin_blame(st->log, st->cursor, exonerated.data(), tiles);
  // an event between ids that are no CU's (a block stored none) blames nobody: no verdict
  if (blame.bad_event) return (int)hipErrorUnknown;
  for (int t = 0; t < tiles; ++t) attr->tiles_moved += moved[t] != 0;
  for (uint32_t id = 0; id < GM_CUSCAN_IDS; ++id) attr->cus_seen += seen[id] != 0;
  attr->tiles = (uint32_t)tiles;
  attr->grid = (uint32_t)grid;
  attr->step = (uint32_t)step;
  attr->rotations = (uint32_t)(done < grid ? done : grid);  // step is coprime to the grid
  attr->first_id = first;
  attr->inject_id = !inject ? GM_CUSCAN_ANY : inject->first ? first : inject->id;
  gm_burnin_store_blame(blame, st->log, attr, blamed, blamed_cap);
  *iters = done;
  *mismatches = st->total;
  if (ms > 0) *tflops = 2.0 * n * (double)n * n * done / (ms * 1e-3) / 1e12;
  return 0;
}

}  // namespace
