// gm_gemm_shared.h — what the two burn-in GEMMs (gm_gemm.hip: bf16, gm_mxgemm.hip: block-scaled
// fp8 / fp4) share: the 256² tile frame of their kernels (geometry, per-thread coordinates,
// operand stage, tile pick, epilogue; the schedules stay with the kernels), the compare kernels
// and the burn-in driver: one front for the plain and the attributed entry points of either
// format, its two loops, their flip control and timed batches. In an anonymous namespace, like
// gm_probe_common.h: each translation unit gets its own copy.
#pragma once

#include <stddef.h>

#include "gm_burnin_attr.h"
#include "gm_probe_common.h"
#include "gm_where.h"

namespace {

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

// ------------------------------------------------------------------ the 256² tile frame
// The geometry all three kernel bodies have (design notes: gm_gemm.hip): a 256×256 output tile,
// 512 threads = 8 waves as 2(M)×4(N), each wave 128×64 as 8×4 16x16 accumulators; a K-tile is 128
// bytes of every row (64 bf16, 128 fp8, 256 fp4), so one operand's stage is 32 KiB whatever the
// format, and the byte layout below is the same for all of them.
namespace tile256 {
constexpr int TM = 256, TN = 256, kRowBytes = 128, kThreads = 512, kGroupM = 8;
constexpr int kTileBytes = TM * kRowBytes;    // 32 KiB: one operand, one stage
constexpr int kStageBytes = 2 * kTileBytes;   // A + Bt
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void gbl_void;
}  // namespace tile256

// A thread's coordinates in the tile, computed once. The XOR swizzle of the 16-B chunk index
// with (row>>1)&7 removes the bank conflicts of the 16-row ds_read_b128 fragment reads; it is
// applied to the per-lane GLOBAL source address (schunk) and to the LDS read address (foff0),
// and the two are only ever changed together, here.
struct TileLane {
  int lane, wave, wm, wn;  // wave (uniform) = 4 wm + wn
  // Staging: wave w moves 1 KiB chunks c = w + 8i (i = 0..3) of each operand's 256-row tile.
  // Lane l writes LDS byte c*1024 + l*16 = row 8c + (l>>3), slot l&7, which holds logical
  // 16-B chunk (l&7) ^ ((row>>1)&7). (row>>1)&7 is the same for all i (rows differ by 64).
  int srow, schunk;
  // Fragment reads: lane l reads row frow = l&15 of a 16-row block at logical chunk l>>4 of the
  // first 64 bytes (foff0; the second 64: ^ 64); a_off / b_off: that in this wave's rows of the
  // A / Bt half of a stage, 16-row block i a further i * 2048.
  int frow, foff0, a_off, b_off;
};
__device__ __forceinline__ TileLane tile_lane() {
  using namespace tile256;
  TileLane c;
  const int tid = threadIdx.x;
  c.lane = tid & 63;
  c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  c.wm = c.wave >> 2, c.wn = c.wave & 3;
  c.srow = 8 * c.wave + (c.lane >> 3);
  c.schunk = (c.lane & 7) ^ ((c.srow >> 1) & 7);
  c.frow = c.lane & 15;
  c.foff0 = c.frow * 128 + (((c.lane >> 4) ^ (c.frow >> 1)) << 4);
  c.a_off = c.wm * 128 * 128 + c.foff0;
  c.b_off = kTileBytes + c.wn * 64 * 128 + c.foff0;
  return c;
}

// This thread's 16 staged bytes of K-tile 0, in row row0 + srow of an operand whose rows are
// `row` elements of T apart.
template <class T>
__device__ __forceinline__ const T* tile_src(const TileLane& c, const T* op, int row0, size_t row) {
  return op + (size_t)(row0 + c.srow) * row + c.schunk * (16 / (int)sizeof(T));
}

// The operand stage: HBM→LDS with global_load_lds_dwordx4 (no VGPR round trip), 2 × 4 of them
// per thread, into the stage at `stage`. a_src / b_src from tile_src; row64, the stride of 64
// rows, and k0, the K-tile's offset, in elements of T.
template <class T, class K0>
__device__ __forceinline__ void tile_stage(const TileLane& c, char* stage, const T* a_src,
                                           const T* b_src, size_t row64, K0 k0) {
  using namespace tile256;
  char* base = stage + c.wave * 1024;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    __builtin_amdgcn_global_load_lds((gbl_void*)(a_src + i * row64 + k0),
                                     (lds_void*)(base + i * 8192), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void*)(b_src + i * row64 + k0),
                                     (lds_void*)(base + kTileBytes + i * 8192), 16, 0, 0);
  }
}

__device__ __forceinline__ void tile_zero(f32x4 (&acc)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The block's output tile: the XCD-aware map (gm_gemm_tile_map, gm_burnin_attr.h), in the plain
// kernels at rotation 0, a constant that folds away. kTraced, the attributed burn-in's form: at
// the iteration's rotation tr.r, and the block books itself (trace_block). Returns the flip the
// epilogue takes.
template <bool kTraced>
__device__ __forceinline__ uint32_t tile_pick(int M, int N, const GemmTrace& tr, int& tm, int& tn) {
  using namespace tile256;
  gm_gemm_tile_map<TM, TN, kGroupM>((int)blockIdx.x, (int)gridDim.x, M, N, kTraced ? tr.r : 0, tm,
                                    tn);
  if constexpr (kTraced) return trace_block(tr, tm * (N / TN) + tn);
  return 0;
}

// Epilogue: the C/D map of the 16x16 MFMA shapes: col = l&15, row = 4(l>>4) + reg. kTraced:
// element (0, 0) of the tile leaves with `flip` XORed into its bits.
template <bool kTraced>
__device__ __forceinline__ void tile_store(const TileLane& c, __bf16* __restrict__ C, int N, int tm,
                                           int tn, const f32x4 (&acc)[8][4], uint32_t flip) {
  using namespace tile256;
  const int crow = tm * TM + c.wm * 128 + 4 * (c.lane >> 4);
  const int ccol = tn * TN + c.wn * 64 + (c.lane & 15);
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        C[(size_t)(crow + i * 16 + r) * N + ccol + j * 16] =
            kTraced && i == 0 && j == 0 && r == 0 ? bf16_flipped(acc[0][0][0], flip)
                                                  : (__bf16)acc[i][j][r];
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

// numRegs and localSizeBytes of a kernel from hipFuncGetAttributes on the current device.
inline int kernel_regs(const void* kernel, int* num_regs, int* scratch_bytes) {
  if (!num_regs || !scratch_bytes) return (int)hipErrorInvalidValue;
  hipFuncAttributes attr;
  GM_CHECK(hipFuncGetAttributes(&attr, kernel));
  *num_regs = attr.numRegs;
  *scratch_bytes = (int)attr.localSizeBytes;
  return 0;
}

// ------------------------------------------------------------------ the burn-in driver
// A format's side of a burn-in is one small operand object, made from the format's code:
//   static bool shape_ok(int fmt, int n)  the format takes n × n × n
//   int fill(int n)                      allocates the operands and fills them (seeds 0x5151 and
//                                         0xa3a3) on the current device
//   int gemm(void* c, int n) const        launches one n³ GEMM into the n × n bf16 buffer c on
//   int gemm_traced(void* c, int n, const GemmTrace&) const      the null stream, plain / traced
// all but the first returning a HIP error code. BurnInBf16 (gm_gemm.hip) and BurnInMx
// (gm_mxgemm.hip) are the two.

// The negative control: corrupt the finished reference, through the host like the memtest's flip.
// The blocking copies on the null stream wait for the GEMM before them.
inline int burn_in_flip_reference(void* ref, int n_flips, const uint64_t* flip_elems,
                                  const uint16_t* flip_masks) {
  for (int i = 0; i < n_flips; ++i) {
    uint16_t* at = (uint16_t*)ref + flip_elems[i];
    uint16_t v = 0;
    GM_CHECK(hipMemcpy(&v, at, sizeof(v), hipMemcpyDeviceToHost));
    v ^= flip_masks[i];
    GM_CHECK(hipMemcpy(at, &v, sizeof(v), hipMemcpyHostToDevice));
  }
  return 0;
}

// The timed part of a burn-in: step(i), i = 1, 2, ..., launches iteration i's GEMM and compare on
// the null stream, in order, so the next GEMM overwrites a result only after the compare has
// read it. Batches of 8 steps with a synchronisation after each, until `seconds` have passed.
// *done: the steps launched; *ms: their time between two events.
template <class Step>
int burn_in_timed(double seconds, Step step, int* done, float* ms) {
  Events ev;
  GM_CHECK(ev.create());
  GM_CHECK(hipEventRecord(ev.e0, nullptr));
  const double t0 = now_s();
  int e = 0;
  while (!e) {
    for (int i = 0; i < 8 && !e; ++i) e = step(++*done);
    if (!e) e = (int)hipDeviceSynchronize();
    if (now_s() - t0 >= seconds) break;
  }
  if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
  if (!e) e = (int)hipEventSynchronize(ev.e1);
  if (!e) e = elapsed_ms(ev.e0, ev.e1, ms);
  return e;
}

// 2 n³ per GEMM over the wall time. The compare kernels are included; they move 2 × n² × 2 B per
// GEMM (about 2 % of a bf16 GEMM's time at 8192³, more of the shorter MX ones: profiles/mxgemm/).
inline double burn_in_tflops(int n, int done, float ms) {
  return ms > 0 ? 2.0 * n * (double)n * n * done / (ms * 1e-3) / 1e12 : 0;
}

// The plain burn-in, on the current device with the operands filled. The first result is the
// reference; the flips are applied to it; every later result is compared with it bit for bit: the
// kernel is deterministic (fixed reduction order, no atomics), so any difference is a hardware
// fault.
template <class Operands>
int burn_in_loop(const Operands& ops, int n, double seconds, int n_flips,
                 const uint64_t* flip_elems, const uint16_t* flip_masks, double* tflops,
                 uint64_t* mismatches, int* iters) {
  const size_t elems = (size_t)n * n;
  DevBuf dref, dc, dcount;
  GM_CHECK(dref.alloc(elems * 2));
  GM_CHECK(dc.alloc(elems * 2));
  GM_CHECK(dcount.alloc(sizeof(unsigned long long)));
  GM_CHECK(hipMemset(dcount.p, 0, sizeof(unsigned long long)));
  if (int e = ops.gemm(dref.p, n)) return e;  // the reference result
  if (int e = burn_in_flip_reference(dref.p, n_flips, flip_elems, flip_masks)) return e;
  int done = 0;
  float ms = 0;
  const auto step = [&](int) {
    const int rc = ops.gemm(dc.p, n);
    return rc ? rc : launch_count_diff(dc.p, dref.p, elems / 8, dcount.p, nullptr);  // 16-B words
  };
  if (int e = burn_in_timed(seconds, step, &done, &ms)) return e;
  unsigned long long bad = 0;
  GM_CHECK(hipMemcpy(&bad, dcount.p, sizeof(bad), hipMemcpyDeviceToHost));
  *iters = done;
  *mismatches = bad;
  *tflops = burn_in_tflops(n, done, ms);
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

// What an attributed burn-in takes and gives besides a plain one's arguments.
struct BurnInAttr {
  const gm_burnin_inject_t* inject;
  gm_burnin_attr_t* attr;
  gm_burnin_blamed_t* blamed;
  int blamed_cap;
};

// burn_in_loop's sibling, on the traced GEMM: the tiles rotate from one iteration to the next.
template <class Operands>
int burn_in_attr_loop(const Operands& ops, int n, double seconds, int n_flips,
                      const uint64_t* flip_elems, const uint16_t* flip_masks, const BurnInAttr& at,
                      double* tflops, uint64_t* mismatches, int* iters) {
  const gm_burnin_inject_t* inject = at.inject;
  gm_burnin_attr_t* attr = at.attr;
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
  int e = ops.gemm_traced(dref.p, n, tr);
  if (!e) e = compare(dref.p, dwarm.p, dwarm.p, 0);
  if (e) return e;
  if (inject) {
    if (inject->first) tr.inj_id_at = (const uint32_t*)dwarm.p;
    tr.inj_id = inject->id;
    tr.inj_mask = inject->mask;
  }
  // The reference result and its CU map, then the same compare: it books the reference's CUs.
  tr.cu_of_tile = (uint32_t*)dref_cu.p;
  e = ops.gemm_traced(dref.p, n, tr);
  if (!e) e = compare(dref.p, dref_cu.p, dref_cu.p, 0);
  if (e) return e;
  if ((e = burn_in_flip_reference(dref.p, n_flips, flip_elems, flip_masks))) return e;
  tr.cu_of_tile = (uint32_t*)dcu.p;
  int done = 0;
  float ms = 0;
  const auto iteration = [&](int i) {
    tr.r = gm_burnin_rotation(grid, step, i);
    const int rc = ops.gemm_traced(dc.p, n, tr);
    return rc ? rc : compare(dc.p, dcu.p, dref_cu.p, (uint32_t)i);
  };
  if ((e = burn_in_timed(seconds, iteration, &done, &ms))) return e;

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
  gm_burnin_store_blame(blame, st->log, attr, at.blamed, at.blamed_cap);
  *iters = done;
  *mismatches = st->total;
  *tflops = burn_in_tflops(n, done, ms);
  return 0;
}

// The front of the four burn-in entry points: the plain burn-in, or with `at` the attributed one.
// The outputs are zeroed before any refusal, and every refusal comes before the device is chosen.
template <class Operands>
int burn_in_run(int fmt, int dev, int n, double seconds, int n_flips,
                const uint64_t* flip_elems, const uint16_t* flip_masks, double* tflops,
                uint64_t* mismatches, int* iters, const BurnInAttr* at = nullptr) {
  *tflops = 0;
  *mismatches = 0;
  *iters = 0;
  if (at) {
    if (!at->attr || at->blamed_cap < 0 || (at->blamed_cap > 0 && !at->blamed))
      return (int)hipErrorInvalidValue;
    *at->attr = gm_burnin_attr_t{};
  }
  if (!Operands::shape_ok(fmt, n) || seconds <= 0 || (at && !burn_in_inject_ok(at->inject)) ||
      !burn_in_flips_ok((size_t)n * n, n_flips, flip_elems, flip_masks))
    return (int)hipErrorInvalidValue;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  Operands ops(fmt);  // after the guard: its buffers go before the device is restored
  if (int e = ops.fill(n)) return e;
  if (at)
    return burn_in_attr_loop(ops, n, seconds, n_flips, flip_elems, flip_masks, *at, tflops,
                             mismatches, iters);
  return burn_in_loop(ops, n, seconds, n_flips, flip_elems, flip_masks, tflops, mismatches, iters);
}

}  // namespace
