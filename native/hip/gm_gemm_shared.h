// gm_gemm_shared.h — what the two burn-in GEMMs (gm_gemm.hip: bf16, gm_mxgemm.hip: block-scaled
// fp8 / fp4) share: the XCD-aware block → tile map, the compare kernel and the bit-exact burn-in
// loop with its flip control. In an anonymous namespace, like gm_probe_common.h: each translation
// unit gets its own copy.
#pragma once

#include "gm_probe_common.h"

namespace {

// XCD-aware block → output tile: bijective for any grid size (the dispatcher deals block ids
// round-robin over the 8 XCDs, so ids ≡ x mod 8 share XCD x's L2 and get a contiguous range of
// tiles), then a GROUP_M-deep raster so co-resident tiles share A rows and B columns.
template <int TM, int TN, int kGroupM>
__device__ __forceinline__ void gemm_tile_of(int M, int N, int& tm, int& tn) {
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int q = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
  const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
  const int ntm = M / TM, ntn = N / TN;
  const int per_group = kGroupM * ntn;
  const int first_m = (wgid / per_group) * kGroupM;
  const int gsize = min(ntm - first_m, kGroupM);
  tm = first_m + (wgid % per_group) % gsize;
  tn = (wgid % per_group) / gsize;
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

}  // namespace
