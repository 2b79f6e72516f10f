// gm_pattern_chunks.h — how the pattern-streaming kernels (native/hip/gm_pattern_stream.h) split
// a buffer among their blocks. Plain C++ with no HIP: tests/test_pattern_host.cpp checks it alone.
#pragma once
#include <stdint.h>

struct gm_pattern_chunks_t {
  uint64_t per_block;  // elements per block: a whole number of steps
  uint32_t grid;       // blocks to launch; block b owns [b * per_block, min(n, (b + 1) * per_block))
};

// A contiguous chunk for each of at most `blocks` blocks (0 counts as 1) over n >= 1 elements,
// each chunk a whole number of `step` >= 1 elements. Blocks whose chunk would start past the end
// are not launched: (grid - 1) * per_block < n <= grid * per_block.
inline gm_pattern_chunks_t gm_pattern_chunks(uint64_t n, uint64_t blocks, uint64_t step) {
  if (blocks == 0) blocks = 1;
  const uint64_t share = n / blocks + (n % blocks != 0);  // ceil without n + blocks - 1 wrapping
  uint64_t steps = share / step + (share % step != 0);
  if (steps == 0) steps = 1;
  const uint64_t per_block = steps * step;
  return {per_block, (uint32_t)(n / per_block + (n % per_block != 0))};
}
