// Host side of the attributed burn-in (include/gm_burnin_attr.h) under ASan/UBSan: the rotated
// block → tile map as a bijection at every grid and rotation the GPU tests and the default size
// use, r = 0 against a second, plain copy of the map the GEMMs have always used, the step's two
// conditions, and the blame rule on synthetic logs.
// No GPU, no HIP, nothing loaded into an interpreter; part of `make -C native check`.
#include <stdint.h>
#include <stdio.h>

#include <set>
#include <vector>

#include "gm_burnin_attr.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// The map before it had a rotation, written out again: 256² tiles, groups of 8 tile rows.
static void plain_map(int block, int grid, int M, int N, int& tm, int& tn) {
  const int q = grid / 8, rem = grid % 8, xcd = block % 8;
  int wgid = block / 8;
  for (int x = 0; x < xcd; ++x) wgid += x < rem ? q + 1 : q;  // the XCDs before this one
  const int ntm = M / 256, ntn = N / 256;
  const int group = wgid / (8 * ntn), in_group = wgid % (8 * ntn);
  const int rows = ntm - group * 8 < 8 ? ntm - group * 8 : 8;
  tm = group * 8 + in_group % rows;
  tn = in_group / rows;
}

static void map(int block, int grid, int M, int N, int r, int& tm, int& tn) {
  gm_gemm_tile_map<kBurninTile, kBurninTile, kBurninGroupM>(block, grid, M, N, r, tm, tn);
}

static void test_map() {
  const int sizes[] = {256, 768, 1536, 2048, 8192};
  const int tiles[] = {1, 9, 36, 64, 1024};
  for (int s = 0; s < 5; ++s) {
    const int n = sizes[s], grid = (n / 256) * (n / 256);
    EXPECT(grid == tiles[s]);
    const int rs[] = {0, 1, 7, 8, grid - 1};
    for (int r : rs) {
      if (r >= grid) continue;  // the 1-tile grid has r = 0 alone
      std::set<int> seen;
      for (int b = 0; b < grid; ++b) {
        int tm = -1, tn = -1;
        map(b, grid, n, n, r, tm, tn);
        EXPECT(tm >= 0 && tm < n / 256 && tn >= 0 && tn < n / 256);
        seen.insert(tm * (n / 256) + tn);
        int pm, pn;  // block b at rotation r stands in for block (b + r) mod grid
        plain_map((b + r) % grid, grid, n, n, pm, pn);
        EXPECT(pm == tm && pn == tn);
      }
      EXPECT((int)seen.size() == grid);
    }
    const int step = gm_burnin_step(grid);
    EXPECT(step >= 1 && gm_burnin_gcd(step, grid) == 1);
    EXPECT(grid <= 8 || step % 8 != 0);
    std::set<int> rot;  // coprime: every rotation within grid iterations
    for (int i = 1; i <= grid; ++i) rot.insert(gm_burnin_rotation(grid, step, i));
    EXPECT((int)rot.size() == grid);
    EXPECT(gm_burnin_rotation(grid, step, 1) == step % grid);
    EXPECT(gm_burnin_rotation(grid, step, (int64_t)1 << 40) < grid);  // no 32-bit product
  }
  // rectangular grids and every grid size up to 70: still a bijection at every r
  for (int ntm = 1; ntm <= 10; ++ntm)
    for (int ntn = 1; ntn <= 7; ++ntn) {
      const int grid = ntm * ntn;
      for (int r = 0; r < grid; ++r) {
        std::set<int> seen;
        for (int b = 0; b < grid; ++b) {
          int tm, tn;
          map(b, grid, ntm * 256, ntn * 256, r, tm, tn);
          EXPECT(tm >= 0 && tm < ntm && tn >= 0 && tn < ntn);
          seen.insert(tm * ntn + tn);
        }
        EXPECT((int)seen.size() == grid);
      }
      const int step = gm_burnin_step(grid);
      EXPECT(gm_burnin_gcd(step, grid) == 1 && (grid <= 8 || step % 8 != 0));
    }
}

static const gm_burnin_blamed_t* find(const GmBurninBlame& b, uint32_t id) {
  for (const auto& u : b.blamed)
    if (u.id == id) return &u;
  return nullptr;
}

static void test_blame() {
  const int tiles = 64;
  {  // a transient worker fault on a tile another CU reproduced: the worker
    std::vector<uint8_t> ex(tiles, 1);
    const gm_burnin_event_t ev[] = {{5, 3, 0x123, 0x045, 2}};
    const GmBurninBlame b = gm_burnin_blame(ev, 1, ex.data(), tiles);
    EXPECT(b.blamed.size() == 1 && b.blamed[0].id == 0x123 && b.blamed[0].as_worker == 1);
    EXPECT(b.blamed[0].as_reference == 0 && b.blamed[0].words == 2 && b.blamed[0].events == 1);
    EXPECT(b.events == 1 && b.logged == 1 && !b.log_overflow && b.tiles_exonerated == 64);
  }
  {  // a corrupted reference tile that never matches: the reference, whoever worked
    std::vector<uint8_t> ex(tiles, 1);
    ex[7] = 0;
    std::vector<gm_burnin_event_t> ev;
    for (uint32_t i = 1; i <= 40; ++i) ev.push_back({i, 7, 0x200 + i, 0x045, 1});
    const GmBurninBlame b = gm_burnin_blame(ev.data(), (int64_t)ev.size(), ex.data(), tiles);
    EXPECT(b.blamed.size() == 1 && b.blamed[0].id == 0x045 && b.blamed[0].as_reference == 40);
    EXPECT(b.blamed[0].as_worker == 0 && b.blamed[0].words == 40 && b.tiles_exonerated == 63);
  }
  {  // a consistent CU X: wrong as the reference of tile 9 and as a worker elsewhere: only X
    const uint32_t X = 0x311;
    std::vector<uint8_t> ex(tiles, 1);
    ex[9] = 0;  // X computed the reference there; nobody reproduces it
    std::vector<gm_burnin_event_t> ev;
    for (uint32_t i = 1; i <= 20; ++i) {
      if (i % 5) ev.push_back({i, 9, 0x400 + i, X, 1});  // others against X's reference
      ev.push_back({i, i % 8 + 20, X, 0x500 + i, 1});    // X against the others' references
    }
    const GmBurninBlame b = gm_burnin_blame(ev.data(), (int64_t)ev.size(), ex.data(), tiles);
    EXPECT(b.blamed.size() == 1 && b.blamed[0].id == X);
    EXPECT(b.blamed[0].as_reference == 16 && b.blamed[0].as_worker == 20);
    EXPECT(b.blamed[0].events == 36);
  }
  {  // W == R blames W, exonerated or not
    std::vector<uint8_t> ex(tiles, 0);
    const gm_burnin_event_t ev[] = {{1, 0, 0x077, 0x077, 3}};
    const GmBurninBlame b = gm_burnin_blame(ev, 1, ex.data(), tiles);
    EXPECT(b.blamed.size() == 1 && b.blamed[0].id == 0x077 && b.blamed[0].as_worker == 1);
  }
  {  // W == R at a tile other units disagree with too: the reference's role, unless exonerated
    for (int exonerated = 0; exonerated < 2; ++exonerated) {
      std::vector<uint8_t> ex(tiles, (uint8_t)exonerated);
      const gm_burnin_event_t ev[] = {{9, 7, 0x045, 0x045, 1}, {1, 7, 0x201, 0x045, 1},
                                      {2, 7, 0x202, 0x045, 1}, {9, 8, 0x046, 0x046, 1},
                                      {3, 6, 0x203, 0x046, 1}};
      const GmBurninBlame b = gm_burnin_blame(ev, 5, ex.data(), tiles);
      const gm_burnin_blamed_t *u = find(b, 0x045), *v = find(b, 0x046);
      EXPECT(u && v);
      if (!u || !v) continue;
      // tile 8 has no witness but the unit itself; the event at tile 6 is another tile's
      EXPECT(v->as_worker == 1u && v->events == (exonerated ? 1u : 2u));
      EXPECT(u->as_reference == (exonerated ? 0u : 3u) && u->as_worker == (exonerated ? 1u : 0u));
      EXPECT(u->events == (exonerated ? 1u : 3u));
    }
  }
  {  // the order: most events first, ties by id
    std::vector<uint8_t> ex(tiles, 1);
    const gm_burnin_event_t ev[] = {{1, 0, 9, 1, 1}, {1, 1, 4, 1, 1}, {2, 2, 7, 1, 1},
                                    {2, 3, 7, 1, 1}};
    const GmBurninBlame b = gm_burnin_blame(ev, 4, ex.data(), tiles);
    EXPECT(b.blamed.size() == 3 && b.blamed[0].id == 7 && b.blamed[1].id == 4);
    EXPECT(b.blamed[2].id == 9);
  }
  {  // overflow: reported, and what was not logged is not read, so it blames nobody
    std::vector<uint8_t> ex(tiles, 1);
    std::vector<gm_burnin_event_t> ev(GM_BURNIN_LOG_CAP, gm_burnin_event_t{1, 2, 0x123, 0x045, 1});
    ev.push_back({9, 2, 0xFFFFFFFFu, 0x7777777u, 1});  // past the capacity: never looked at
    const GmBurninBlame b = gm_burnin_blame(ev.data(), 5000, ex.data(), tiles);
    EXPECT(b.log_overflow && b.events == 5000 && b.logged == GM_BURNIN_LOG_CAP && !b.bad_event);
    EXPECT(b.blamed.size() == 1 && find(b, 0x123) && find(b, 0x123)->events == GM_BURNIN_LOG_CAP);
    gm_burnin_attr_t attr{};
    gm_burnin_blamed_t out[2] = {};
    gm_burnin_store_blame(b, ev.data(), &attr, out, 2);
    EXPECT(attr.records_filled == GM_BURNIN_MAX_RECORDS && attr.records[15].worker == 0x123);
    EXPECT(attr.log_overflow == 1 && attr.events == 5000 && attr.logged == GM_BURNIN_LOG_CAP);
    EXPECT(attr.n_blamed == 1 && out[0].id == 0x123 && out[1].id == 0);
  }
  {  // an event outside the tables is refused, not indexed
    std::vector<uint8_t> ex(tiles, 1);
    const gm_burnin_event_t ev[] = {{1, 64, 1, 2, 1}, {1, 0, 4096, 2, 1}, {1, 0, 1, 4096, 1}};
    const GmBurninBlame b = gm_burnin_blame(ev, 3, ex.data(), tiles);
    EXPECT(b.bad_event && b.blamed.empty());
  }
}

int main() {
  test_map();
  test_blame();
  if (failures) {
    printf("test_burnin_attr_host: %d failure(s)\n", failures);
    return 1;
  }
  printf("test_burnin_attr_host: ok\n");
  return 0;
}
