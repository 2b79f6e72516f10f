// gm_burnin_attr.h — what the attributed burn-in (gm_probe.h, "attributed burn-in") evaluates on
// both sides or on the host alone: the rotated block → tile map (host and device), the step of
// the rotation and the blame rule (host only). Plain C++, no HIP: native/tests/
// test_burnin_attr_host.cpp builds it on its own.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "gm_probe.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GM_BURNIN_HD __host__ __device__ inline
#else
#define GM_BURNIN_HD inline
#endif

// Block → output tile of a grid of (M / TM) · (N / TN) blocks at rotation r, 0 <= r < grid.
// The block id is rotated first: block b takes the place of block (b + r) mod grid. Then the
// XCD-aware remap, bijective for any grid size (the dispatcher deals block ids round-robin over
// the 8 XCDs, so ids ≡ x mod 8 share XCD x's L2 and get a contiguous range of tiles), then a
// kGroupM-deep raster so co-resident tiles share A rows and B columns. A rotation and two
// bijections: bijective for every grid and r. With r % 8 != 0 a tile lands on another XCD.
// A constant r = 0 folds away: the plain kernels' map.
template <int TM, int TN, int kGroupM>
GM_BURNIN_HD void gm_gemm_tile_map(int block, int grid, int M, int N, int r, int& tm, int& tn) {
  const int nwg = grid;
  const int orig = r == 0 ? block : (block + r >= nwg ? block + r - nwg : block + r);
  const int q = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
  const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
  const int ntm = M / TM, ntn = N / TN;
  const int per_group = kGroupM * ntn;
  const int first_m = (wgid / per_group) * kGroupM;
  const int gsize = ntm - first_m < kGroupM ? ntm - first_m : kGroupM;
  tm = first_m + (wgid % per_group) % gsize;
  tn = (wgid % per_group) / gsize;
}

// The geometry of the two burn-in GEMMs (tile256 in hip/gm_gemm_shared.h).
constexpr int kBurninTile = 256, kBurninGroupM = 8;

inline int gm_burnin_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The rotation's step for a grid: the smallest s above grid / 3 that is coprime to the grid
// (iteration i runs at r = i · s mod grid, so every r comes up within grid iterations) and,
// where the grid has more than 8 blocks, no multiple of 8 (so r % 8 changes, and with it the
// XCD of every tile, from one iteration to the next). About a third of the grid, not 1: the
// tile then also leaves the neighbourhood of blocks that were dispatched together. One of
// grid + 1 and 2 · grid + 1 always qualifies, so the search ends.
inline int gm_burnin_step(int grid) {
  for (int s = grid / 3 + 1;; ++s)
    if (gm_burnin_gcd(s, grid) == 1 && (grid <= 8 || s % 8 != 0)) return s;
}

inline int gm_burnin_rotation(int grid, int step, int64_t iteration) {
  return (int)((iteration * (int64_t)step) % grid);
}

struct GmBurninBlame {
  uint64_t events = 0;  // as counted: the logged ones and those past the log's capacity
  uint32_t logged = 0, tiles_exonerated = 0;
  bool log_overflow = false, bad_event = false;
  std::vector<gm_burnin_blamed_t> blamed;  // most events first, ties by id
};

// The blame rule. An event at tile t with worker W and reference R blames W if t is exonerated
// (another CU reproduced the reference's bits there, so the reference stands) or W == R (one
// unit disagreeing with itself), else R: no other CU ever reproduced the reference's tile, so
// the reference is the odd one out, whether its fault was transient or consistent. The role
// follows the same reasoning: W is blamed as the worker, R as the reference, and a unit that
// disagrees with itself (W == R) as the worker unless t is not exonerated and another unit
// disagreed with that reference in a logged event too. Then the reference is the odd one out
// for its own CU as for every other, and the event counts as_reference. Only the
// first min(n_events, GM_BURNIN_LOG_CAP) events exist; the others were counted, not logged.
inline GmBurninBlame gm_burnin_blame(const gm_burnin_event_t* events, int64_t n_events,
                                     const uint8_t* exonerated, int tiles) {
  GmBurninBlame out;
  out.events = (uint64_t)n_events;
  out.logged = (uint32_t)std::min<int64_t>(n_events, GM_BURNIN_LOG_CAP);
  out.log_overflow = out.events > out.logged;
  for (int t = 0; t < tiles; ++t) out.tiles_exonerated += exonerated[t] != 0;
  const auto bad = [&](const gm_burnin_event_t& e) {
    return e.tile >= (uint32_t)tiles || e.worker >= GM_CUSCAN_IDS || e.reference >= GM_CUSCAN_IDS;
  };
  std::vector<uint8_t> others(tiles > 0 ? tiles : 0, 0);  // another unit disagreed with the tile
  for (uint32_t i = 0; i < out.logged; ++i)
    if (!bad(events[i]) && events[i].worker != events[i].reference) others[events[i].tile] = 1;
  std::vector<int> slot(GM_CUSCAN_IDS, -1);
  for (uint32_t i = 0; i < out.logged; ++i) {
    const gm_burnin_event_t& e = events[i];
    if (bad(e)) {
      out.bad_event = true;
      continue;
    }
    const bool worker =
        exonerated[e.tile] != 0 || (e.worker == e.reference && others[e.tile] == 0);
    const uint32_t id = worker ? e.worker : e.reference;
    if (slot[id] < 0) {
      slot[id] = (int)out.blamed.size();
      out.blamed.push_back(gm_burnin_blamed_t{id, 0, 0, 0, 0});
    }
    gm_burnin_blamed_t& b = out.blamed[slot[id]];
    ++b.events;
    ++(worker ? b.as_worker : b.as_reference);
    b.words += e.words;
  }
  std::sort(out.blamed.begin(), out.blamed.end(),
            [](const gm_burnin_blamed_t& a, const gm_burnin_blamed_t& b) {
              return a.events != b.events ? a.events > b.events : a.id < b.id;
            });
  return out;
}

// The summary fields of *attr, its first records and the caller's array from a blame over
// `events` (the log the blame was made from).
inline void gm_burnin_store_blame(const GmBurninBlame& b, const gm_burnin_event_t* events,
                                  gm_burnin_attr_t* attr, gm_burnin_blamed_t* blamed,
                                  int blamed_cap) {
  attr->records_filled = std::min<uint32_t>(b.logged, GM_BURNIN_MAX_RECORDS);
  for (uint32_t i = 0; i < attr->records_filled; ++i) attr->records[i] = events[i];
  attr->events = b.events;
  attr->logged = b.logged;
  attr->log_overflow = b.log_overflow;
  attr->tiles_exonerated = b.tiles_exonerated;
  attr->n_blamed = (uint32_t)b.blamed.size();
  for (size_t i = 0; i < b.blamed.size() && (int)i < blamed_cap; ++i) blamed[i] = b.blamed[i];
}
