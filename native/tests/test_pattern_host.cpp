// The pattern-stream kernels' chunking (include/gm_pattern_chunks.h) under ASan/UBSan: every n in
// 1…4096 and n around 2^32 and 2^36 elements, for the block counts and steps the tests that use
// it launch with. The kernel of gm_pattern_stream.h gives block b the elements
// [b * per_block, min(n, (b + 1) * per_block)), so these properties are what keeps every
// element covered once and no block outside the buffer.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <stdint.h>
#include <stdio.h>

#include "gm_pattern_chunks.h"

static int failures = 0;
#define EXPECT(cond)                                                                        \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      if (++failures <= 20)                                                                 \
        printf("FAIL %s:%d: %s (n %llu blocks %llu step %llu)\n", __FILE__, __LINE__, #cond, \
               (unsigned long long)n, (unsigned long long)blocks, (unsigned long long)step); \
    }                                                                                       \
  } while (0)

static void check(uint64_t n, uint64_t blocks, uint64_t step) {
  const gm_pattern_chunks_t c = gm_pattern_chunks(n, blocks, step);
  EXPECT(c.per_block >= step && c.per_block % step == 0);
  EXPECT(c.grid >= 1 && c.grid <= blocks);
  // in 128 bits, so that a product that would wrap 64 shows as a failure and not as a pass
  const unsigned __int128 per = c.per_block, covered = per * c.grid;
  EXPECT(per * (c.grid - 1) < n && n <= covered);
  EXPECT(covered <= UINT64_MAX);
  // the kernel's own arithmetic for the last block: begin + per_block, in 64 bits
  EXPECT((uint64_t)(c.grid - 1) * c.per_block <= UINT64_MAX - c.per_block);
}

int main() {
  const uint64_t blocks_of[5] = {1, 2, 16, 512, 1024};
  const uint64_t steps[2] = {1024, 2048};
  const uint64_t bigs[2] = {1ull << 32, 1ull << 36};
  for (uint64_t blocks : blocks_of)
    for (uint64_t step : steps) {
      for (uint64_t n = 1; n <= 4096; ++n) check(n, blocks, step);
      for (uint64_t big : bigs)
        for (uint64_t n = big - 2 * step - 1; n <= big + 2 * step + 1; ++n) check(n, blocks, step);
    }

  // what the shapes of the GPU tests rely on: 1 MiB + 4112 B on 512 blocks of 32 KiB steps is 32
  // one-step blocks and one with 257 elements; 0 blocks count as one
  const gm_pattern_chunks_t m = gm_pattern_chunks(((1u << 20) + 4112) / 16, 512, 2048);
  const gm_pattern_chunks_t z = gm_pattern_chunks(5000, 0, 1024);
  const uint64_t n = 0, blocks = 0, step = 0;  // EXPECT prints them
  EXPECT(m.per_block == 2048 && m.grid == 33);
  EXPECT(z.per_block == 5120 && z.grid == 1);

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("test_pattern_host: ok\n");
  return 0;
}
