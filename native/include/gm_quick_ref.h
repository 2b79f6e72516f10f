// gm_quick_ref.h — the liveness probe's expected words and its verdict, one definition for the
// gfx950 kernel (k_quick in native/hip/gm_probe.hip, which takes its lane value from here) and
// for the host (gm_probe_quick and the gm_probe_quick_* entry points). The formulas are written
// out in gm_probe.h; this is their only implementation.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GM_QUICK_HD __host__ __device__ inline
#else
#define GM_QUICK_HD inline
#endif

#define GM_QUICK_LANES 64
#define GM_QUICK_SUM_WORD 64     /* the 64-lane shuffle reduction of the lane words, mod 2^32 */
#define GM_QUICK_BALLOT_WORD 65  /* popcount of the wave's ballot: 64 on a wave64 machine */
#define GM_QUICK_WORDS 66

// which checks of gm_quick_verdict failed
enum {
  GM_QUICK_BAD_LANES = 1,   // one of words 0..63 is not its lane's value
  GM_QUICK_BAD_SUM = 2,     // word 64 is not the sum of the 64 lane values
  GM_QUICK_BAD_BALLOT = 4,  // word 65 is not 64
};

GM_QUICK_HD uint32_t gm_quick_salt(int dev) { return 0x9e3779b9u ^ (uint32_t)dev; }

GM_QUICK_HD uint32_t gm_quick_lane_value(uint32_t lane, uint32_t salt) {
  return lane * 2654435761u ^ salt;
}

inline void gm_quick_expected(uint32_t salt, uint32_t out[GM_QUICK_WORDS]) {
  uint32_t sum = 0;
  for (uint32_t l = 0; l < GM_QUICK_LANES; ++l) {
    out[l] = gm_quick_lane_value(l, salt);
    sum += out[l];
  }
  out[GM_QUICK_SUM_WORD] = sum;
  out[GM_QUICK_BALLOT_WORD] = GM_QUICK_LANES;
}

// 0 when all 66 words are the expected ones for `salt`, else the GM_QUICK_BAD_* bits of the
// checks that failed. The three checks are independent: each is made against the expected
// table, never against another received word.
inline uint32_t gm_quick_verdict(const uint32_t got[GM_QUICK_WORDS], uint32_t salt) {
  uint32_t want[GM_QUICK_WORDS];
  gm_quick_expected(salt, want);
  uint32_t failed = 0;
  for (uint32_t l = 0; l < GM_QUICK_LANES; ++l)
    if (got[l] != want[l]) failed |= GM_QUICK_BAD_LANES;
  if (got[GM_QUICK_SUM_WORD] != want[GM_QUICK_SUM_WORD]) failed |= GM_QUICK_BAD_SUM;
  if (got[GM_QUICK_BALLOT_WORD] != want[GM_QUICK_BALLOT_WORD]) failed |= GM_QUICK_BAD_BALLOT;
  return failed;
}
