// gm_gemm.hip — the 256²-tile bf16 burn-in GEMM (schedule V5, with V1 as its reference point)
// and the bit-exact burn-in loop. Part of libgm_probe.so (built with gm_probe.hip).
// Measurements: profiles/history/r1_gemm/ (round 1 also timed eight other schedules, V0 V2-V4 V6-V9;
// none beat V5, and they were removed: the GEMM is a burn-in load, not a product kernel).

#include "gm_probe.h"
#include "gm_gemm_shared.h"

namespace {

// ------------------------------------------------------------------ MFMA bf16 GEMM, 256² tile
// Throughput form of the burn-in GEMM: C[M,N] (bf16) = A[M,K] · Bt[N,K]ᵀ, both operands K-major
// (the layout global_load_lds can stage without a transpose). Design (cdna_hip_programming.md §5):
//   * 256×256 output tile, BK=64, 512 threads = 8 waves as 2(M)×4(N); each wave owns 128×64 as
//     8×4 v_mfma_f32_16x16x32_bf16 accumulators (128 VGPRs), ~1 block per CU;
//   * operands go HBM→LDS with global_load_lds_dwordx4 (no VGPR round trip), two LDS stages of
//     64 KiB, the next stage's DMA issued before the current stage's MFMAs;
//   * LDS image lane-linear (one 1 KiB wave instruction = 8 rows × 128 B); bank conflicts of the
//     16-row ds_read_b128 fragment reads are removed by an XOR swizzle of the 16-B chunk index
//     with (row>>1)&7, applied to the per-lane GLOBAL source address and to the LDS read address
//     (TileLane, gm_gemm_shared.h, which holds everything here but the schedules);
//   * blockIdx remapped bijectively so each XCD runs a contiguous range of tiles, grouped 8 tile
//     rows deep, so concurrently running blocks of one XCD share A/B panels in that XCD's L2.
namespace g256 {
using namespace tile256;                      // the geometry itself: gm_gemm_shared.h
constexpr int TK = kRowBytes / 2;             // 64 bf16
constexpr int kLdsBytes = 2 * kStageBytes;    // two stages: 128 KiB of the 160 KiB LDS
}  // namespace g256
constexpr int kGemmNtDefault = 5;  // profiles/history/r1_gemm: V5 +2.9 % over V1 at 4096³, +0.9 % at 8192³

// V1 — the plain schedule, kept as the reference point for V5: all 24 fragment reads of the
// 64-deep K-tile are issued up front, so the second k-step's reads overlap the first step's
// MFMAs, then one vmcnt(0) + barrier per K-tile.
__global__ __launch_bounds__(512) void k_gemm_nt256(const __bf16* __restrict__ A,
                                                    const __bf16* __restrict__ Bt,
                                                    __bf16* __restrict__ C, int M, int N, int K) {
  using namespace g256;
  __shared__ __attribute__((aligned(1024))) char lds[kLdsBytes];
  const TileLane c = tile_lane();
  int tm, tn;
  tile_pick<false>(M, N, GemmTrace{}, tm, tn);
  const __bf16* a_src = tile_src(c, A, tm * TM, K);
  const __bf16* b_src = tile_src(c, Bt, tn * TN, K);
  const size_t row64 = (size_t)64 * K;
  auto stage = [&](int buf, int k0) {
    tile_stage(c, lds + buf * kStageBytes, a_src, b_src, row64, k0);
  };
  f32x4 acc[8][4];
  tile_zero(acc);

  const int nt = K / TK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) stage(cur ^ 1, (t + 1) * TK);
    const char* sb = lds + cur * kStageBytes;
    {
      bf16x8 af[2][8], bfr[2][4];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          bfr[kk][j] =
              *reinterpret_cast<const bf16x8*>(sb + ((c.b_off + j * 16 * 128) ^ (kk << 6)));
#pragma unroll
        for (int i = 0; i < 8; ++i)
          af[kk][i] =
              *reinterpret_cast<const bf16x8*>(sb + ((c.a_off + i * 16 * 128) ^ (kk << 6)));
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[kk][i], bfr[kk][j],
                                                                acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  tile_store<false>(c, C, N, tm, tn, acc, 0);
}

// V5 — V1's geometry with a local-read prefetch across the barrier. The second k-step's MFMAs
// of tile t are deferred past the barrier, so they run while the first k-step fragments of
// tile t+1 are read. Every fragment-read batch then overlaps 32 MFMAs of the same wave, and
// register use stays at two fragment sets (like V1). The barrier sits mid-tile, so the next
// tile's DMA is issued right after it.
//
// kTraced: the attributed burn-in's form of the same schedule. The tile comes from the map
// rotated by tr.r, thread 0 stores the block's CU id under the tile, and a block on the injected
// CU flips element (0, 0) of its tile on the way out (tile_pick, gm_gemm_shared.h). Nothing
// else differs: operands, order of summation and epilogue are the plain form's.
//
// This body, the one the burn-in and gemm_tflops time, spells the tile frame's coordinates,
// stage, zeroing and epilogue out (the same text as TileLane, tile_stage, tile_zero and
// tile_store; change them together). Written on those pieces it computes the same bits, but the
// compiler orders its address arithmetic and epilogue stores differently, and it measured 0.3 %
// (8192³) to 1.2 % (4096³) slower: profiles/burnin_attr/README.md.
template <bool kTraced>
__device__ __forceinline__ void gemm_nt256p_block(const __bf16* __restrict__ A,
                                                  const __bf16* __restrict__ Bt,
                                                  __bf16* __restrict__ C, int M, int N, int K,
                                                  const GemmTrace& tr) {
  using namespace g256;
  __shared__ __attribute__((aligned(1024))) char lds[kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  int tm, tn;
  const uint32_t flip = tile_pick<kTraced>(M, N, tr, tm, tn);
  const int srow = 8 * wave + (lane >> 3);
  const int schunk = (lane & 7) ^ ((srow >> 1) & 7);
  const __bf16* a_src = A + (size_t)(tm * TM + srow) * K + schunk * 8;
  const __bf16* b_src = Bt + (size_t)(tn * TN + srow) * K + schunk * 8;
  const size_t row64 = (size_t)64 * K;
  auto stage = [&](int buf, int k0) {
    char* base = lds + buf * kStageBytes + wave * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((gbl_void*)(a_src + i * row64 + k0),
                                       (lds_void*)(base + i * 8192), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void*)(b_src + i * row64 + k0),
                                       (lds_void*)(base + kTileBytes + i * 8192), 16, 0, 0);
    }
  };
  const int frow = lane & 15;
  const int foff0 = frow * 128 + (((lane >> 4) ^ (frow >> 1)) << 4);
  const int a_off = wm * 128 * 128 + foff0;
  const int b_off = kTileBytes + wn * 64 * 128 + foff0;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 a0[8], b0[4], a1[8], b1[4];
  auto read = [&](const char* sb, int kk, bf16x8 (&af)[8], bf16x8 (&bf)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bf[j] = *reinterpret_cast<const bf16x8*>(sb + ((b_off + j * 2048) ^ (kk << 6)));
#pragma unroll
    for (int i = 0; i < 8; ++i)
      af[i] = *reinterpret_cast<const bf16x8*>(sb + ((a_off + i * 2048) ^ (kk << 6)));
  };
  auto mma = [&](bf16x8 (&af)[8], bf16x8 (&bf)[4]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  const int nt = K / TK;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // Waits go through __builtin_amdgcn_s_waitcnt (gfx9 simm16: vmcnt[3:0]|expcnt[6:4]|
  // lgkmcnt[11:8]|vmcnt[5:4]<<14), not inline asm, so the compiler's own wait insertion knows
  // the counters are clear and adds no lgkmcnt(0) in front of the MFMAs.
  constexpr int kWaitLgkm0 = 0xC07F, kWaitVm0Lgkm0 = 0x0070;
  // Tile t+1's DMA is issued right after the barrier that frees its buffer (mid-tile t-1), so
  // it has a whole tile of MFMAs (64 per wave) to land before the vmcnt(0) that retires it.
  if (nt > 1) stage(1, TK);
  read(lds, 0, a0, b0);
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    const char* sb = lds + cur * kStageBytes;
    __builtin_amdgcn_s_waitcnt(kWaitLgkm0);  // a0/b0 (read behind the last 32 MFMAs) are in
    read(sb, 1, a1, b1);
    mma(a0, b0);
    __builtin_amdgcn_s_waitcnt(kWaitVm0Lgkm0);  // tile t+1 landed; our reads of `cur` done
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 2 < nt) stage(cur, (t + 2) * TK);   // every wave is past its reads of `cur`
    if (t + 1 < nt) read(lds + (cur ^ 1) * kStageBytes, 0, a0, b0);
    mma(a1, b1);
  }

  const int crow = tm * TM + wm * 128 + 4 * (lane >> 4);
  const int ccol = tn * TN + wn * 64 + (lane & 15);
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

__global__ __launch_bounds__(512) void k_gemm_nt256p(const __bf16* __restrict__ A,
                                                     const __bf16* __restrict__ Bt,
                                                     __bf16* __restrict__ C, int M, int N,
                                                     int K) {
  gemm_nt256p_block<false>(A, Bt, C, M, N, K, GemmTrace{});
}

__global__ __launch_bounds__(512) void k_gemm_nt256p_traced(const __bf16* __restrict__ A,
                                                            const __bf16* __restrict__ Bt,
                                                            __bf16* __restrict__ C, int M, int N,
                                                            int K, GemmTrace tr) {
  gemm_nt256p_block<true>(A, Bt, C, M, N, K, tr);
}

// Deterministic uniform [-1, 1] bf16 fill (random operands: zero-filled ones overstate a GEMM).
// The fp32 value lies in [-1, 1); the ones within half a bf16 step of 1 round up to exactly 1.0.
// The element index is hashed as 32 bits, so the sequence repeats after 2^32 elements.
__global__ __launch_bounds__(256) void k_fill_bf16(__bf16* dst, size_t n, uint32_t seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ seed;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    dst[i] = (__bf16)((float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f);
  }
}

// The one launch of the fill kernel (the compare kernel's is in gm_gemm_shared.h): the drivers
// below and the caller-owned-buffer entry points share them, so a test of the latter runs the
// grids the former use.
int launch_fill_bf16(void* dst, size_t n, uint32_t seed, hipStream_t s) {
  hipLaunchKernelGGL(k_fill_bf16, dim3(4096), dim3(256), 0, s, (__bf16*)dst, n, seed);
  return (int)hipGetLastError();
}

// The one launch of the traced kernel; the arguments were checked.
int launch_gemm_nt_traced(const void* A, const void* Bt, void* C, int M, int N, int K,
                          const GemmTrace& tr, hipStream_t stream) {
  using namespace g256;
  hipLaunchKernelGGL(k_gemm_nt256p_traced, dim3((M / TM) * (N / TN)), dim3(kThreads), 0, stream,
                     (const __bf16*)A, (const __bf16*)Bt, (__bf16*)C, M, N, K, tr);
  return (int)hipGetLastError();
}

// The bf16 burn-in's operands (gm_gemm_shared.h, "the burn-in driver"); bf16 has no format code.
struct BurnInBf16 {
  DevBuf da, db;
  explicit BurnInBf16(int) {}
  static bool shape_ok(int, int n) { return n > 0 && n % g256::TM == 0; }
  int fill(int n) {
    const size_t elems = (size_t)n * n;
    GM_CHECK(da.alloc(elems * 2));
    GM_CHECK(db.alloc(elems * 2));
    const int e = launch_fill_bf16(da.p, elems, 0x5151u, nullptr);
    return e ? e : launch_fill_bf16(db.p, elems, 0xa3a3u, nullptr);
  }
  int gemm(void* c, int n) const { return gm_probe_gemm_nt(da.p, db.p, c, n, n, n, nullptr); }
  int gemm_traced(void* c, int n, const GemmTrace& tr) const {
    return launch_gemm_nt_traced(da.p, db.p, c, n, n, n, tr, nullptr);
  }
};

}  // namespace

extern "C" {

int gm_probe_gemm_nt_variant(int variant, const void* A, const void* Bt, void* C, int M, int N,
                             int K, void* stream) {
  using namespace g256;
  if (M <= 0 || N <= 0 || K <= 0 || M % TM || N % TN || K % TK) return (int)hipErrorInvalidValue;
  const dim3 grid((M / TM) * (N / TN)), block(kThreads);
  switch (variant) {
    case 1:
      hipLaunchKernelGGL(k_gemm_nt256, grid, block, 0, (hipStream_t)stream,
                         (const __bf16*)A, (const __bf16*)Bt, (__bf16*)C, M, N, K);
      break;
    case 5:
      hipLaunchKernelGGL(k_gemm_nt256p, grid, block, 0, (hipStream_t)stream,
                         (const __bf16*)A, (const __bf16*)Bt, (__bf16*)C, M, N, K);
      break;
    default:
      return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

int gm_probe_gemm_nt(const void* A, const void* Bt, void* C, int M, int N, int K,
                     void* stream) {
  return gm_probe_gemm_nt_variant(kGemmNtDefault, A, Bt, C, M, N, K, stream);
}

int gm_probe_gemm_nt_tflops(int dev, int M, int N, int K, int iters, double* tflops) {
  using namespace g256;
  *tflops = 0;
  if (iters <= 0 || M <= 0 || N <= 0 || K <= 0 || M % TM || N % TN || K % TK)
    return (int)hipErrorInvalidValue;
  DeviceGuard g(dev);
  if (!g.ok) return (int)hipErrorInvalidDevice;
  DevBuf da, db, dc;
  GM_CHECK(da.alloc((size_t)M * K * 2));
  GM_CHECK(db.alloc((size_t)N * K * 2));
  GM_CHECK(dc.alloc((size_t)M * N * 2));
  int e = launch_fill_bf16(da.p, (size_t)M * K, 0x1234u, nullptr);
  if (!e) e = launch_fill_bf16(db.p, (size_t)N * K, 0x9876u, nullptr);
  if (e) return e;
  Events ev;
  GM_CHECK(ev.create());
  e = gm_probe_gemm_nt(da.p, db.p, dc.p, M, N, K, nullptr);  // warm-up
  if (!e) e = (int)hipEventRecord(ev.e0, nullptr);
  for (int i = 0; i < iters && !e; ++i) e = gm_probe_gemm_nt(da.p, db.p, dc.p, M, N, K, nullptr);
  if (!e) e = (int)hipEventRecord(ev.e1, nullptr);
  if (!e) e = (int)hipEventSynchronize(ev.e1);
  float ms = 0;
  if (!e) e = elapsed_ms(ev.e0, ev.e1, &ms);
  if (!e && ms > 0) *tflops = 2.0 * M * N * (double)K * iters / (ms * 1e-3) / 1e12;
  return e;
}

int gm_probe_count_diff(const void* a, const void* b, uint64_t bytes, void* stream,
                        uint64_t* count) {
  if (!count) return (int)hipErrorInvalidValue;
  *count = 0;
  if (!a || !b || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || bytes == 0 || (bytes & 15))
    return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  DevBuf dcount;
  GM_CHECK(dcount.alloc(sizeof(unsigned long long)));
  GM_CHECK(hipMemsetAsync(dcount.p, 0, sizeof(unsigned long long), s));
  if (int e = launch_count_diff(a, b, bytes / 16, dcount.p, s)) return e;
  unsigned long long h = 0;
  GM_CHECK(hipMemcpyAsync(&h, dcount.p, sizeof(h), hipMemcpyDeviceToHost, s));
  GM_CHECK(hipStreamSynchronize(s));
  *count = h;
  return 0;
}

int gm_probe_fill_bf16(void* dst, uint64_t n_elems, uint32_t seed, void* stream) {
  if (!dst || ((uintptr_t)dst & 1) || n_elems == 0) return (int)hipErrorInvalidValue;
  return launch_fill_bf16(dst, n_elems, seed, (hipStream_t)stream);
}

int gm_probe_burn_in(int dev, int n, double seconds, double* tflops, uint64_t* mismatches,
                     int* iters) {
  return gm_probe_burn_in_flip(dev, n, seconds, 0, nullptr, nullptr, tflops, mismatches, iters);
}

int gm_probe_burn_in_flip(int dev, int n, double seconds, int n_flips,
                          const uint64_t* flip_elems, const uint16_t* flip_masks,
                          double* tflops, uint64_t* mismatches, int* iters) {
  return burn_in_run<BurnInBf16>(0, dev, n, seconds, n_flips, flip_elems, flip_masks, tflops,
                                 mismatches, iters);
}

// ------------------------------------------------------------------ attributed burn-in

int gm_probe_burn_in_blame(const gm_burnin_event_t* events, int64_t n_events,
                           const uint8_t* exonerated, int tiles, gm_burnin_attr_t* out,
                           gm_burnin_blamed_t* blamed, int blamed_cap) {
  if (!out || tiles <= 0 || !exonerated || n_events < 0 || (n_events > 0 && !events) ||
      blamed_cap < 0 || (blamed_cap > 0 && !blamed))
    return (int)hipErrorInvalidValue;
  *out = gm_burnin_attr_t{};
  const GmBurninBlame b = gm_burnin_blame(events, n_events, exonerated, tiles);
  if (b.bad_event) return (int)hipErrorInvalidValue;
  gm_burnin_store_blame(b, events, out, blamed, blamed_cap);
  return 0;
}

int gm_probe_burn_in_tile_map(int M, int N, int block, int r, int* tm, int* tn, int* step) {
  using namespace g256;
  if (!tm || !tn || !step || M <= 0 || N <= 0 || M % TM || N % TN)
    return (int)hipErrorInvalidValue;
  const int64_t grid = (int64_t)(M / TM) * (N / TN);
  if (grid > INT32_MAX || block < 0 || block >= grid || r < 0 || r >= grid)
    return (int)hipErrorInvalidValue;
  gm_gemm_tile_map<TM, TN, kGroupM>(block, (int)grid, M, N, r, *tm, *tn);
  *step = gm_burnin_step((int)grid);
  return 0;
}

int gm_probe_gemm_nt_traced(const void* A, const void* Bt, void* C, int M, int N, int K, int r,
                            uint32_t* cu_of_tile, const gm_burnin_inject_t* inject,
                            void* stream) {
  using namespace g256;
  if (M <= 0 || N <= 0 || K <= 0 || M % TM || N % TN || K % TK || !A || !Bt || !C)
    return (int)hipErrorInvalidValue;
  const int grid = (M / TM) * (N / TN);
  if (r < 0 || r >= grid || !cu_of_tile || ((uintptr_t)cu_of_tile & 3) ||
      !burn_in_inject_ok(inject) || (inject && inject->first))
    return (int)hipErrorInvalidValue;
  return launch_gemm_nt_traced(
      A, Bt, C, M, N, K,
      GemmTrace{r, cu_of_tile, nullptr, inject ? inject->id : 0, inject ? inject->mask : 0},
      (hipStream_t)stream);
}

int gm_probe_gemm_nt_traced_info(int* num_regs, int* scratch_bytes) {
  return kernel_regs((const void*)k_gemm_nt256p_traced, num_regs, scratch_bytes);
}

int gm_probe_count_diff_tiles(const void* a, const void* b, int n, const uint32_t* cu,
                              const uint32_t* ref_cu, uint32_t iteration, void* state,
                              uint32_t* exonerated, uint32_t* moved, uint32_t* seen,
                              void* stream) {
  if (n <= 0 || n % kBurninTile || (int64_t)(n / kBurninTile) * (n / kBurninTile) > INT32_MAX)
    return (int)hipErrorInvalidValue;
  if (!a || !b || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || !state || ((uintptr_t)state & 7))
    return (int)hipErrorInvalidValue;
  for (const void* p : {(const void*)cu, (const void*)ref_cu, (const void*)exonerated,
                        (const void*)moved, (const void*)seen})
    if (!p || ((uintptr_t)p & 3)) return (int)hipErrorInvalidValue;
  return launch_count_diff_tiles(a, b, n, iteration, AttrMaps{cu, ref_cu, exonerated, moved, seen},
                                 state, (hipStream_t)stream);
}

uint64_t gm_probe_burn_in_state_bytes(void) { return sizeof(gm_burnin_state_t); }

int gm_probe_burn_in_attr(int dev, int n, double seconds, int n_flips,
                          const uint64_t* flip_elems, const uint16_t* flip_masks,
                          const gm_burnin_inject_t* inject, double* tflops,
                          uint64_t* mismatches, int* iters, gm_burnin_attr_t* attr,
                          gm_burnin_blamed_t* blamed, int blamed_cap) {
  const BurnInAttr at{inject, attr, blamed, blamed_cap};
  return burn_in_run<BurnInBf16>(0, dev, n, seconds, n_flips, flip_elems, flip_masks, tflops,
                                 mismatches, iters, &at);
}

}  // extern "C"
