// gm_where.h — where a wave runs, read from the hardware registers: the one reader behind the
// per-CU scans (gm_cuscan_frame.h) and the attributed burn-in (gm_gemm_shared.h).
// In an anonymous namespace: each translation unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// s_getreg immediate: (size - 1) << 11 | offset << 6 | register
constexpr int kRegHwId = 4, kRegXccId = 20;
constexpr int getreg(int size, int offset, int reg) {
  return ((size - 1) << 11) | (offset << 6) | reg;
}

// id: XCC_ID[3:0] << 8 | HW_ID[15:8] (SE 15:13, SH 12, CU 11:8), 12 bits; simd: HW_ID[5:4].
struct Where {
  uint32_t id, simd;
};

__device__ __forceinline__ Where where_am_i() {
  Where at;
  at.id = (__builtin_amdgcn_s_getreg(getreg(4, 0, kRegXccId)) << 8) |
          __builtin_amdgcn_s_getreg(getreg(8, 8, kRegHwId));
  at.simd = __builtin_amdgcn_s_getreg(getreg(2, 4, kRegHwId));
  return at;
}

}  // namespace
