// Stand-alone driver of fibergen_amd/csrc/fg_tile_frame.h (tests/test_tile_frame.py builds and runs it, plain and sanitized):
// for every grid, tile shape and CU count it walks every workgroup of the plan and every thread, as the six tiled marching
// sweeps of fg_kernels_fast.hip construct their frame, and checks
//   ownership  every pair (x, j, kp) of the grid is owned, for 0 <= step < nsteps, by exactly one thread;
//   offsets    j, kp and plane(q), q = x0 - 2 .. x0 + nsteps + 1, lie inside the field -- under both wraps, on a whole grid
//              and on an x-slab with its four spare planes (xw_lo = nx + 4, xw_hi = 0, as SlabGroup sets them);
//   rows       rm / rp of an owning row are r - 1 / r + 1;
//   surplus    padding workgroups make no step under either convention (nsteps -2 or 0);
//   remap      the XCD remap is a permutation of 0 .. nb - 1 (every tile is some workgroup's, the others are surplus).
// It prints one PLAN line per case (the test compares them with the parent's figures) and exits 1 on the first failed check.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../../fibergen_amd/csrc/fg_tile_frame.h"

using namespace fg;

static int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      std::printf("FAIL %s: ", #cond);       \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
      if (++failures > 20) std::exit(1);     \
    }                                        \
  } while (0)

// every workgroup and thread of plan p on grid g (gi: 0 whole, 1 x-slab; field: its elements) under one wrap and one convention
template <int TYR, int ZS, XWrap WRAP>
static void walk_frames(const Grid& g, int gi, long field, const TilePlan& p, int surplus_nsteps) {
  using S = TileShape<TYR, ZS>;
  const int nx = g.nx, ny = g.ny, nzh = g.nz / 2;
  std::vector<int> owners((size_t)nx * ny * nzh, 0);
  for (int b = 0; b < p.nb; ++b) {
    for (int th = 0; th < S::THREADS; ++th) {
      const TileFrame t = tile_frame<TYR, ZS, WRAP>(g, p.nty, p.ntz, p.LX, b, p.nb, (unsigned)th, surplus_nsteps);
      CHECK(t.r >= 0 && t.r < TYR && t.zs >= 0 && t.zs < S::NZS && t.l >= 0 && t.l < 64 && t.li >= 0 && t.li < S::RW,
            "place of thread %d", th);
      CHECK(t.zprev >= 0 && t.zprev < S::NZS && t.znext >= 0 && t.znext < S::NZS, "segments of thread %d", th);
      CHECK(t.rm >= 0 && t.rm < TYR && t.rp >= 0 && t.rp < TYR, "rows of thread %d", th);
      CHECK(t.j >= 0 && t.j < ny && t.kp >= 0 && t.kp < nzh, "block %d thread %d: j %d kp %d", b, th, t.j, t.kp);
      CHECK(t.rowoff == (long)t.j * g.nzp + 2 * t.kp, "rowoff of block %d thread %d", b, th);
      if (t.surplus) {
        CHECK(t.nsteps == surplus_nsteps && t.nsteps <= 0, "surplus block %d makes %d steps", b, t.nsteps);
      } else {
        CHECK(t.nsteps >= 1 && t.nsteps <= p.LX && t.x0 >= 0 && t.x0 + t.nsteps <= nx, "block %d: x0 %d nsteps %d", b, t.x0, t.nsteps);
      }
      for (int q = t.x0 - 2; q <= t.x0 + t.nsteps + 1; ++q) {
        const long o = t.plane[q - (t.x0 - 2)];
        CHECK(o >= 0 && o + 1 < field, "block %d thread %d plane %d: offset %ld of %ld", b, th, q, o, field);
        if (q >= 0 && q < nx) CHECK(o == (long)q * g.nyzp + t.rowoff, "plane %d is not itself", q);
      }
      if (t.own) {
        CHECK(t.rm == t.r - 1 && t.rp == t.r + 1, "block %d thread %d: row %d has %d / %d", b, th, t.r, t.rm, t.rp);
        for (int st = 0; st < t.nsteps; ++st) ++owners[((size_t)(t.x0 + st) * ny + t.j) * nzh + t.kp];
      }
    }
  }
  for (int x = 0; x < nx; ++x)
    for (int j = 0; j < ny; ++j)
      for (int k = 0; k < nzh; ++k) {
        const int c = owners[((size_t)x * ny + j) * nzh + k];
        CHECK(c == 1, "pair (%d, %d, %d) owned %d times (grid %d, wrap %d, surplus nsteps %d)", x, j, k, c, gi, (int)WRAP, surplus_nsteps);
      }
}

template <int TYR, int ZS>
static void walk(const Grid& whole, int cus, MarchRule rule) {
  const TilePlan p = tile_plan(whole, TYR, ZS, cus, rule);
  std::printf("PLAN %dx%dx%d <%d,%d> cus=%d %s: %d %d %d %d %d\n", whole.nx, whole.ny, whole.nz, TYR, ZS, cus,
              rule == MarchRule::fixed ? "fixed" : "balanced", p.nty, p.ntz, p.LX, p.ntx, p.nb);
  const int nx = whole.nx;
  CHECK(p.nb >= p.nty * p.ntz * p.ntx && (p.nb < 8 || p.nb % 8 == 0), "nb %d", p.nb);
  CHECK(p.LX >= 1 && p.LX <= nx && p.ntx * p.LX >= nx, "LX %d", p.LX);
  {   // the remap is a permutation: the workgroups' tiles -- told apart by (x0, j, kp) of the first owning thread's place -- are
      // all distinct, nty * ntz * ntx of them, and the rest of the nb workgroups is surplus
    using S = TileShape<TYR, ZS>;
    std::set<std::tuple<int, int, int>> tiles;
    int surplus = 0;
    for (int b = 0; b < p.nb; ++b) {
      const TileFrame t = tile_frame<TYR, ZS, XWrap::slab>(whole, p.nty, p.ntz, p.LX, b, p.nb, (unsigned)(S::NZS * 64 + 1), 0);
      if (t.surplus) ++surplus;
      else tiles.insert(std::make_tuple(t.x0, t.j, t.kp));
    }
    CHECK((int)tiles.size() == p.nty * p.ntz * p.ntx && surplus == p.nb - p.nty * p.ntz * p.ntx, "%d tiles, %d surplus of %d",
          (int)tiles.size(), surplus, p.nb);
  }
  Grid slab = whole;
  slab.xw_lo = nx + 4;
  slab.xw_hi = 0;
  for (int gi = 0; gi < 2; ++gi) {
    const Grid& g = gi ? slab : whole;
    const long field = (long)(gi ? nx + 4 : nx) * g.nyzp;
    for (int surplus_nsteps : {-2, 0}) {
      walk_frames<TYR, ZS, XWrap::slab>(g, gi, field, p, surplus_nsteps);
      walk_frames<TYR, ZS, XWrap::periodic>(g, gi, field, p, surplus_nsteps);
    }
  }
}

int main() {
  const int grids[][3] = {{4, 14, 80}, {8, 14, 124}, {4, 14, 200}, {6, 20, 130}, {6, 14, 128},
                          {16, 16, 128}, {4, 14, 256}, {5, 20, 256}, {9, 14, 80}};
  const int cus[] = {256, 512, 2};
  for (const auto& n : grids) {
    const Grid g = make_grid(n[0], n[1], n[2], 1.0, 1.0, 1.0);
    for (int c : cus) {
      tile_shape_dispatch(g.nz / 2, [&](auto R, auto Z) { walk<decltype(R)::value, decltype(Z)::value>(g, c, MarchRule::balanced); });
      if (g.nz / 2 == 128)   // the callers without a <6, 2> form
        tile_shape_dispatch<false>(g.nz / 2, [&](auto R, auto Z) { walk<decltype(R)::value, decltype(Z)::value>(g, c, MarchRule::balanced); });
    }
    tile_shape_dispatch(g.nz / 2, [&](auto R, auto Z) { walk<decltype(R)::value, decltype(Z)::value>(g, 256, MarchRule::fixed); });
  }
  if (failures) return 1;
  std::printf("OK\n");
  return 0;
}
