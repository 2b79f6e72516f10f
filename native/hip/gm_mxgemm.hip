// gm_mxgemm.hip — the block-scaled (MX) burn-in GEMM for gfx950: C[M,N] (bf16) = A[M,K] · Bt[N,K]ᵀ
// with fp8 (e4m3) or fp4 (e2m1) operands and one E8M0 scale per 32 elements of K, on
// v_mfma_scale_f32_16x16x128_f8f6f4; its operand fills, its host expected values and its burn-in
// (the loop of gm_gemm_shared.h, shared with the bf16 GEMM). Part of libgm_probe.so.
// Value model: gm_mxgemm_ref.h, formulas in gm_probe.h. Measurements: profiles/mxgemm/.

#include "gm_probe.h"
#include "gm_gemm_shared.h"
#include "gm_mxgemm_ref.h"

namespace {

// ------------------------------------------------------------------ MX GEMM, 256² tile
// On the tile frame of gm_gemm_shared.h, like the bf16 kernels (gm_gemm.hip): 256×256 output
// tile, 512 threads = 8 waves as 2(M)×4(N), each wave 128×64 as 8×4 16x16 accumulators; operands
// HBM→LDS with global_load_lds_dwordx4, two stages, the XOR swizzle of the 16-B chunk index with
// (row>>1)&7; the block → tile map. A K-tile is 128 bytes of every row, so the byte layout is
// the bf16 kernels': 128 elements of fp8 (one MFMA per accumulator), 256 of fp4 (two). Here are
// the schedule, the fragments and the scales.
//
// Lane maps of v_mfma_scale_f32_16x16x128_f8f6f4 (lane l holds row / column l & 15, g = l >> 4):
//   fp8: bytes 0-15 are k = 16 g + j, bytes 16-31 are k = 64 + 16 g + (j - 16): logical chunks g
//        and 4 + g of the row's 128 bytes, the two reads of the bf16 kernel's two k-steps;
//   fp4: the 16 bytes are k = 32 g + 2 j, 2 j + 1 (low nibble first): chunk g of the 64 bytes of
//        one 128-element step, again the bf16 kernel's read, once per step;
//   the scale of row r, block s (k in [32 s, 32 s + 32)) is read from lane r + 16 s, byte 0.
// (profiles/r3_mx/README.md for fp8; profiles/mxgemm/lanemap.json for fp4.)
//
// Scales: one dword (fp8) or two (fp4) per row and K-tile, staged by one global_load_lds_dword
// per thread and step (thread t: operand t >> 8, row t & 255) into 4 KiB per stage behind the
// operand stages; a lane reads its byte with ds_read_u8 right before the MFMA that uses it.
namespace mx256 {
using namespace tile256;                       // the geometry itself: gm_gemm_shared.h
constexpr int kScaleStep = (TM + TN) * 4;      // 2 KiB: every row's 4 scale bytes of one step
constexpr int kScaleStage = 2 * kScaleStep;    // fp4 has two steps per K-tile
constexpr int kScaleBase = 2 * kStageBytes;    // 128 KiB of operands first
constexpr int kLdsBytes = kScaleBase + 2 * kScaleStage;  // 136 KiB of the 160 KiB LDS
}  // namespace mx256

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// The operand registers of one MFMA from the LDS stage `sb`: fp8 the two chunks of the lane's
// row, fp4 the one chunk of step kk (the upper four registers are not read by the instruction).
template <int FMT>
__device__ __forceinline__ i32x8 mx_fragment(const char* sb, int off, int kk) {
  if constexpr (FMT == GM_MX_FP8) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(sb + off);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(sb + (off ^ 64));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
    const i32x4 v = *reinterpret_cast<const i32x4*>(sb + (off ^ (kk << 6)));
    return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1);
  }
}

// kTraced: the attributed burn-in's form, as in gm_gemm.hip: the tile from the map rotated by
// tr.r, the block's CU id stored under it, element (0, 0) flipped on the injected CU; operands,
// order of summation and epilogue are the plain form's.
template <int FMT, bool kTraced>
__device__ __forceinline__ void mxgemm_nt_block(const uint8_t* __restrict__ A,
                                                const uint8_t* __restrict__ sA,
                                                const uint8_t* __restrict__ Bt,
                                                const uint8_t* __restrict__ sB,
                                                __bf16* __restrict__ C, int M, int N, int K,
                                                const GemmTrace& tr) {
  using namespace mx256;
  constexpr int kSteps = FMT == GM_MX_FP4 ? 2 : 1;  // MFMAs of K = 128 per accumulator and K-tile
  __shared__ __attribute__((aligned(1024))) char lds[kLdsBytes];
  const int tid = threadIdx.x;
  int tm, tn;
  const uint32_t flip = tile_pick<kTraced>(M, N, tr, tm, tn);
  const TileLane c = tile_lane();

  const size_t row_bytes = gm_mx_row_bytes(FMT, (size_t)K), srow_bytes = (size_t)K / GM_MX_BLOCK;
  const uint8_t* a_src = tile_src(c, A, tm * TM, row_bytes);
  const uint8_t* b_src = tile_src(c, Bt, tn * TN, row_bytes);
  // Scale staging: waves 0-3 move A's rows 64 w + l, waves 4-7 Bt's, 4 bytes per step.
  const uint8_t* s_src = c.wave < 4 ? sA + (size_t)(tm * TM + tid) * srow_bytes
                                    : sB + (size_t)(tn * TN + tid - TM) * srow_bytes;

  auto stage = [&](int buf, int t) {
    tile_stage(c, lds + buf * kStageBytes, a_src, b_src, 64 * row_bytes, (size_t)t * kRowBytes);
    char* sbase = lds + kScaleBase + buf * kScaleStage + c.wave * 256;
#pragma unroll
    for (int kk = 0; kk < kSteps; ++kk)
      __builtin_amdgcn_global_load_lds((gbl_void*)(s_src + ((size_t)t * kSteps + kk) * 4),
                                       (lds_void*)(sbase + kk * kScaleStep), 4, 0, 0);
  };

  // Scale reads: byte l>>4 (the block whose scale this lane supplies) of the dword of the lane's
  // row, wm * 128 + frow of A's 256 dwords and wn * 64 + frow of Bt's behind them.
  const int sa_off = c.wm * 512 + c.frow * 4 + (c.lane >> 4);
  const int sb_off = TM * 4 + c.wn * 256 + c.frow * 4 + (c.lane >> 4);

  f32x4 acc[8][4];
  tile_zero(acc);

  const int nt = K / gm_mx_tile_k(FMT);
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) stage(cur ^ 1, t + 1);
    const char* sb = lds + cur * kStageBytes;
    const uint8_t* ss = reinterpret_cast<const uint8_t*>(lds) + kScaleBase + cur * kScaleStage;
#pragma unroll
    for (int kk = 0; kk < kSteps; ++kk) {
      i32x8 bfr[4];
      int bsc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bfr[j] = mx_fragment<FMT>(sb, c.b_off + j * 2048, kk);
        bsc[j] = ss[kk * kScaleStep + sb_off + j * 64];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const i32x8 af = mx_fragment<FMT>(sb, c.a_off + i * 2048, kk);
        const int asc = ss[kk * kScaleStep + sa_off + i * 64];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bfr[j], acc[i][j], FMT,
                                                                       FMT, 0, asc, 0, bsc[j]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  tile_store<kTraced>(c, C, N, tm, tn, acc, flip);
}

template <int FMT>
__global__ __launch_bounds__(512) void k_mxgemm_nt(const uint8_t* __restrict__ A,
                                                   const uint8_t* __restrict__ sA,
                                                   const uint8_t* __restrict__ Bt,
                                                   const uint8_t* __restrict__ sB,
                                                   __bf16* __restrict__ C, int M, int N, int K) {
  mxgemm_nt_block<FMT, false>(A, sA, Bt, sB, C, M, N, K, GemmTrace{});
}

template <int FMT>
__global__ __launch_bounds__(512) void k_mxgemm_nt_traced(const uint8_t* __restrict__ A,
                                                          const uint8_t* __restrict__ sA,
                                                          const uint8_t* __restrict__ Bt,
                                                          const uint8_t* __restrict__ sB,
                                                          __bf16* __restrict__ C, int M, int N,
                                                          int K, GemmTrace tr) {
  mxgemm_nt_block<FMT, true>(A, sA, Bt, sB, C, M, N, K, tr);
}

// The packed element bytes of an operand, then its scale bytes: one grid-stride loop each.
__global__ __launch_bounds__(256) void k_mx_fill(int fmt, int cls, uint32_t seed, uint8_t* elems,
                                                 size_t elem_bytes, uint8_t* scales,
                                                 size_t scale_bytes, uint32_t kblocks) {
  const size_t first = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = first; i < elem_bytes; i += stride)
    elems[i] = (uint8_t)gm_mx_packed_byte(fmt, cls, seed, i);
  for (size_t i = first; i < scale_bytes; i += stride)
    scales[i] = (uint8_t)gm_mx_scale(cls, seed, (uint32_t)(i / kblocks), (uint32_t)(i % kblocks),
                                     kblocks);
}

// The one launch of the traced kernels; the arguments were checked.
int launch_mxgemm_traced(int fmt, const void* A, const void* sA, const void* Bt, const void* sB,
                         void* C, int M, int N, int K, const GemmTrace& tr, hipStream_t stream) {
  using namespace mx256;
  const dim3 grid((M / TM) * (N / TN)), block(kThreads);
  if (fmt == GM_MX_FP4)
    hipLaunchKernelGGL(k_mxgemm_nt_traced<GM_MX_FP4>, grid, block, 0, stream, (const uint8_t*)A,
                       (const uint8_t*)sA, (const uint8_t*)Bt, (const uint8_t*)sB, (__bf16*)C, M,
                       N, K, tr);
  else
    hipLaunchKernelGGL(k_mxgemm_nt_traced<GM_MX_FP8>, grid, block, 0, stream, (const uint8_t*)A,
                       (const uint8_t*)sA, (const uint8_t*)Bt, (const uint8_t*)sB, (__bf16*)C, M,
                       N, K, tr);
  return (int)hipGetLastError();
}

bool shape_ok(int fmt, int M, int N, int K) {
  return gm_mx_format_ok(fmt) && M > 0 && N > 0 && K > 0 && M % mx256::TM == 0 &&
         N % mx256::TN == 0 && K % gm_mx_tile_k(fmt) == 0;
}

// What both GEMM entry points take: a shape of the format's, and pointers as the kernels'
// 16-byte operand loads, 4-byte scale loads and 2-byte stores need them.
bool gemm_args_ok(int fmt, const void* A, const void* sA, const void* Bt, const void* sB,
                  const void* C, int M, int N, int K) {
  return shape_ok(fmt, M, N, K) && A && sA && Bt && sB && C && !((uintptr_t)A & 15) &&
         !((uintptr_t)Bt & 15) && !((uintptr_t)sA & 3) && !((uintptr_t)sB & 3) &&
         !((uintptr_t)C & 1);
}

template <int FMT>
const void* kernel_of(bool traced) {
  return traced ? (const void*)k_mxgemm_nt_traced<FMT> : (const void*)k_mxgemm_nt<FMT>;
}
int mx_kernel_regs(int fmt, bool traced, int* num_regs, int* scratch_bytes) {
  if (!gm_mx_format_ok(fmt)) return (int)hipErrorInvalidValue;
  return kernel_regs(fmt == GM_MX_FP4 ? kernel_of<GM_MX_FP4>(traced) : kernel_of<GM_MX_FP8>(traced),
                     num_regs, scratch_bytes);
}

// The MX burn-ins' operands (gm_gemm_shared.h, "the burn-in driver"): random-class fills.
struct BurnInMx {
  int fmt;
  DevBuf da, db, dsa, dsb;
  explicit BurnInMx(int fmt) : fmt(fmt) {}
  static bool shape_ok(int fmt, int n) { return ::shape_ok(fmt, n, n, n); }
  int fill(int n) {
    const size_t eb = (size_t)n * gm_mx_row_bytes(fmt, (size_t)n), sb = (size_t)n * n / GM_MX_BLOCK;
    GM_CHECK(da.alloc(eb));
    GM_CHECK(db.alloc(eb));
    GM_CHECK(dsa.alloc(sb));
    GM_CHECK(dsb.alloc(sb));
    const int e = gm_probe_mx_fill(fmt, GM_MX_RANDOM, 0x5151u, n, n, da.p, dsa.p, nullptr);
    return e ? e : gm_probe_mx_fill(fmt, GM_MX_RANDOM, 0xa3a3u, n, n, db.p, dsb.p, nullptr);
  }
  int gemm(void* c, int n) const {
    return gm_probe_mxgemm_nt(fmt, da.p, dsa.p, db.p, dsb.p, c, n, n, n, nullptr);
  }
  int gemm_traced(void* c, int n, const GemmTrace& tr) const {
    return launch_mxgemm_traced(fmt, da.p, dsa.p, db.p, dsb.p, c, n, n, n, tr, nullptr);
  }
};

}  // namespace

extern "C" {

int gm_probe_mx_fill(int fmt, int cls, uint32_t seed, int rows, int K, void* elems, void* scales,
                     void* stream) {
  if (!gm_mx_format_ok(fmt) || !gm_mx_class_ok(cls) || rows <= 0 || K <= 0 || K % GM_MX_BLOCK ||
      !elems || !scales)
    return (int)hipErrorInvalidValue;
  const size_t eb = (size_t)rows * gm_mx_row_bytes(fmt, (size_t)K);
  const uint32_t kblocks = (uint32_t)K / GM_MX_BLOCK;
  hipLaunchKernelGGL(k_mx_fill, dim3(4096), dim3(256), 0, (hipStream_t)stream, fmt, cls, seed,
                     (uint8_t*)elems, eb, (uint8_t*)scales, (size_t)rows * kblocks, kblocks);
  return (int)hipGetLastError();
}

int gm_probe_mxgemm_nt(int fmt, const void* A, const void* sA, const void* Bt, const void* sB,
                       void* C, int M, int N, int K, void* stream) {
  using namespace mx256;
  if (!gemm_args_ok(fmt, A, sA, Bt, sB, C, M, N, K)) return (int)hipErrorInvalidValue;
  const dim3 grid((M / TM) * (N / TN)), block(kThreads);
  if (fmt == GM_MX_FP4)
    hipLaunchKernelGGL(k_mxgemm_nt<GM_MX_FP4>, grid, block, 0, (hipStream_t)stream,
                       (const uint8_t*)A, (const uint8_t*)sA, (const uint8_t*)Bt,
                       (const uint8_t*)sB, (__bf16*)C, M, N, K);
  else
    hipLaunchKernelGGL(k_mxgemm_nt<GM_MX_FP8>, grid, block, 0, (hipStream_t)stream,
                       (const uint8_t*)A, (const uint8_t*)sA, (const uint8_t*)Bt,
                       (const uint8_t*)sB, (__bf16*)C, M, N, K);
  return (int)hipGetLastError();
}

int gm_probe_mxgemm_expected(int fmt, int cls, uint32_t seed_a, uint32_t seed_b, int M, int N,
                             int K, uint16_t* c, double* ref, double* abs_sum) {
  if (!gm_mx_format_ok(fmt) || !gm_mx_class_ok(cls) || M <= 0 || N <= 0 || K <= 0 ||
      K % GM_MX_BLOCK || (cls == GM_MX_RANDOM ? !ref || !abs_sum : !c))
    return (int)hipErrorInvalidValue;
  gm_mxgemm_expected_host(fmt, cls, seed_a, seed_b, M, N, K, c, ref, abs_sum);
  return 0;
}

int gm_probe_mxgemm_kernel_info(int fmt, int* num_regs, int* scratch_bytes) {
  return mx_kernel_regs(fmt, false, num_regs, scratch_bytes);
}

int gm_probe_mx_burn_in_flip(int dev, int fmt, int n, double seconds, int n_flips,
                             const uint64_t* flip_elems, const uint16_t* flip_masks,
                             double* tflops, uint64_t* mismatches, int* iters) {
  return burn_in_run<BurnInMx>(fmt, dev, n, seconds, n_flips, flip_elems, flip_masks, tflops,
                               mismatches, iters);
}

// ------------------------------------------------------------------ attributed burn-in

int gm_probe_mxgemm_nt_traced(int fmt, const void* A, const void* sA, const void* Bt,
                              const void* sB, void* C, int M, int N, int K, int r,
                              uint32_t* cu_of_tile, const gm_burnin_inject_t* inject,
                              void* stream) {
  using namespace mx256;
  if (!gemm_args_ok(fmt, A, sA, Bt, sB, C, M, N, K)) return (int)hipErrorInvalidValue;
  if (r < 0 || r >= (M / TM) * (N / TN) || !cu_of_tile || ((uintptr_t)cu_of_tile & 3) ||
      !burn_in_inject_ok(inject) || (inject && inject->first))
    return (int)hipErrorInvalidValue;
  return launch_mxgemm_traced(
      fmt, A, sA, Bt, sB, C, M, N, K,
      GemmTrace{r, cu_of_tile, nullptr, inject ? inject->id : 0, inject ? inject->mask : 0},
      (hipStream_t)stream);
}

int gm_probe_mxgemm_nt_traced_info(int fmt, int* num_regs, int* scratch_bytes) {
  return mx_kernel_regs(fmt, true, num_regs, scratch_bytes);
}

int gm_probe_mx_burn_in_attr(int dev, int fmt, int n, double seconds, int n_flips,
                             const uint64_t* flip_elems, const uint16_t* flip_masks,
                             const gm_burnin_inject_t* inject, double* tflops,
                             uint64_t* mismatches, int* iters, gm_burnin_attr_t* attr,
                             gm_burnin_blamed_t* blamed, int blamed_cap) {
  const BurnInAttr at{inject, attr, blamed, blamed_cap};
  return burn_in_run<BurnInMx>(fmt, dev, n, seconds, n_flips, flip_elems, flip_masks, tflops,
                               mismatches, iters, &at);
}

}  // extern "C"
