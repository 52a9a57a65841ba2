// The frame of the six tiled marching sweeps of fg_kernels_fast.hip (k_u_tile, k_cgu_tile, k_eps_tile, k_sc_tile,
// k_sc_tile_aniso, k_sc_cgu_tile), written once: the shape of a tile, the plan of a launch and the place of one thread in it --
// the index arithmetic, including the rule that every voxel is owned by exactly one thread of one tile.  What a kernel does with
// its place is the kernel's; where the six differ on purpose it is a named parameter here (DESIGN.md 3.1 has the table).  Plain
// C++ without any HIP in it, like fg_cg_loop.h and fg_g0_chain.h, and driven on its own by tests/test_tile_frame.py.
#pragma once

#include <type_traits>

#include "fg_common.h"

namespace fg {

// A workgroup of TYR rows (one wave each, or ZS waves), lanes = consecutive z pairs, marching along x.  Rows 0 and TYR - 1 are
// halo.  ZS >= 1: nz/2 == 64 ZS, a z row is ZS whole waves (no halo lanes).  ZS == 0: general nz, lanes 0 and 63 are halo.
template <int TYR, int ZS>
struct TileShape {
  static constexpr bool FULLROW = ZS > 0;
  static constexpr int NZS = ZS ? ZS : 1;              // waves per row
  static constexpr int TYU = TYR - 2;                  // rows with output
  static constexpr int TZU = FULLROW ? 64 * NZS : 62;  // pairs with output per tile row
  static constexpr int RW = NZS * 64;                  // LDS entries per row
  static constexpr int THREADS = TYR * NZS * 64;
};

// The tile shape of a grid: f(integral_constant TYR, integral_constant ZS).  WIDE = false for callers without a <6, 2> form,
// whose rows of 128 pairs take the general tiles of 62 pairs.
template <bool WIDE = true, class F>
void tile_shape_dispatch(int nzh, F&& f) {
  using std::integral_constant;
  if (nzh == 64) return f(integral_constant<int, 8>{}, integral_constant<int, 1>{});   // a z row is one wave
  if constexpr (WIDE) {
    // a z row is two waves: 6 rows x 2 segments (256^3: 0.268 ms against 0.325 ms with halo lanes; 8 x 2 = 16 waves in
    // lock-step 0.38 ms, 4 x 2 0.31 ms)
    if (nzh == 128) return f(integral_constant<int, 6>{}, integral_constant<int, 2>{});
  }
  // general: tiles of 62 pairs with halo lanes (12- and 16-row tiles move fewer halo bytes -- 512^3: 8.95 -> 8.5 GB -- in the
  // same time: rounds 1 and 5)
  f(integral_constant<int, 8>{}, integral_constant<int, 0>{});
}

// Planes per march of the tiled sweep.  A march of LX planes costs LX + 3 steps (pipeline fill), the workgroups are dealt
// to the CUs in rounds, and a CU with two workgroups runs each at half speed, so the sweep takes about
// ceil(tiles * ceil(nx / LX) / CUs) * (LX + 3) steps: the LX with the smallest product wins, the longer march on a tie.
// Measured against the fixed 32 / 16 of round 1: 128^3 16 -> 12 planes (242 workgroups on 256 CUs) 0.0366 -> 0.0347 ms,
// 11 planes (264: a second round) 0.049 ms; 256^3 32 -> 64 (exactly 256 workgroups) 0.210 -> 0.203 ms, 48 (384) 0.265 ms;
// 512^3 32 -> 64: -1 %; thin x-slabs 32 x 256 x 256 -> 8, 64 x 512 x 512 -> 16 as measured before (44.7 -> 39.9 us,
// 281 -> 240 us).
inline int march_length(int nx, long tiles, int cus) {
  int best = nx < 4 ? nx : 4;
  long best_cost = -1;
  for (int lx = 4; lx <= nx && lx <= 64; ++lx) {   // (128-plane marches: 384^3 0.727 -> 0.766 ms, 512^3 no gain: neighbouring tiles drift apart)
    const long groups = tiles * ((nx + lx - 1) / lx);
    const long cost = ((groups + cus - 1) / cus) * (lx + 3);
    if (best_cost < 0 || cost <= best_cost) best = lx, best_cost = cost;
  }
  return best;
}

// The fixed rule of round 1, which the strain sweep (k_eps_tile) kept: 32 planes, 16 where that leaves CUs idle.
inline int march_length_fixed(int nx, long tiles, int cus) {
  return tiles * ((nx + 31) / 32) < cus ? 16 : 32;
}

enum class MarchRule { balanced, fixed };

// One launch: nty x ntz tiles per plane, ntx marches of LX planes, nb workgroups.  From 8 on nb is rounded up to a multiple
// of 8 so that the XCD remap applies; the surplus workgroups make no step.
struct TilePlan {
  int nty, ntz, LX, ntx, nb;
};

// cus: the CUs the march is sized for (the device's, or twice that for a sweep light enough to run two workgroups per CU at
// full speed)
inline TilePlan tile_plan(const Grid& g, int TYR, int ZS, int cus, MarchRule rule = MarchRule::balanced) {
  const int TYU = TYR - 2, TZU = ZS ? 64 * ZS : 62;
  const int nzh = g.nz / 2;
  TilePlan p;
  p.nty = (g.ny + TYU - 1) / TYU;
  p.ntz = (nzh + TZU - 1) / TZU;
  const long tiles = (long)p.nty * p.ntz;
  p.LX = rule == MarchRule::fixed ? march_length_fixed(g.nx, tiles, cus) : march_length(g.nx, tiles, cus);
  if (p.LX > g.nx) p.LX = g.nx;
  p.ntx = (g.nx + p.LX - 1) / p.LX;
  p.nb = p.nty * p.ntz * p.ntx;
  if (p.nb >= 8) p.nb = ((p.nb + 7) / 8) * 8;
  return p;
}

FG_HD int tile_min(int a, int b) { return (a < b) ? a : b; }

// How a plane index outside [0, nx) is wrapped.  slab: through Grid::xw_lo / xw_hi -- periodic in a whole grid, the spare
// planes of the component in an x-slab.  periodic: with nx, for a sweep that runs on whole grids only.
enum class XWrap { slab, periodic };

// The place of one thread, as locals of the function that states FG_TILE_FRAME: row r (wave wv / NZS) and z segment zs of the
// tile, lane l, entry li of an LDS row; zprev / znext, the z segments before / after this one in the row (periodic); rm / rp,
// the rows before / after this one in the LDS image (clamped: a halo row's is never used); the voxel pair (j, kp) it holds in
// every plane at element offset rowoff, and whether it owns it (own: this thread writes the output of its pair); surplus
// (padding workgroup: the grid is rounded up to a multiple of 8), the first plane x0 and the planes nsteps of the march; hx, hy,
// hz; and plane(q), the element offset of the pair in x plane q, q in [-nx, 2 nx) (slab: [-1, nx + 3), whole grids down to -2).
//
// A macro and not a function: the six kernels must compile to the code they compiled to when each spelled these lines out
// (profiles/tile_frame_resources.md) -- handed over through a returned struct the same values came out with another schedule
// and other register counts.  tile_frame() below is the same text as a function, for the CPU test.
//
// workgroups of one XCD (block % 8) take a contiguous run of tiles: z- and y-adjacent tiles, which share halo
// rows and 128-byte segments, then meet in that XCD's L2 (FETCH_SIZE 2.1x -> see profiles/ for the effect).
// The last tile of a row / column is moved back to end at the boundary: it overlaps its neighbour, which keeps the voxels
// (jr may be -1 or ny).
// SURPLUS_NSTEPS: nsteps of a padding workgroup, whatever makes the kernel's loop take no step -- -2 for a loop
// `st = -1 .. nsteps` (k_u_tile, k_eps_tile; k_cgu_tile asks nsteps > 0 and could take either), 0 for `st = 0 .. nsteps - 1`
// (the scalar kernels; the drain step k_sc_tile_aniso still takes at 0 completes no plane).
// THREAD is unsigned and the rest int, as the kernels had it: the compiler's knowledge of the ranges decides its code.
#define FG_TILE_FRAME(TYR, ZS, WRAP, SURPLUS_NSTEPS, g, nty, ntz, LX, BLOCK, NBLOCKS, THREAD)                                   \
  [[maybe_unused]] const int wv = (THREAD) >> 6, l = (THREAD) & 63;                                                            \
  [[maybe_unused]] const int r = wv / TileShape<TYR, ZS>::NZS, zs = wv % TileShape<TYR, ZS>::NZS;                               \
  [[maybe_unused]] const int li = zs * 64 + l;                                                                                  \
  [[maybe_unused]] const int zprev = (zs + TileShape<TYR, ZS>::NZS - 1) % TileShape<TYR, ZS>::NZS,                              \
                             znext = (zs + 1) % TileShape<TYR, ZS>::NZS;                                                       \
  const int nzh = g.nz / 2;                                                                                                     \
  int tile_b = BLOCK;                                                                                                           \
  {                                                                                                                             \
    const int nb = NBLOCKS;                                                                                                     \
    if (nb % 8 == 0) tile_b = (tile_b % 8) * (nb / 8) + tile_b / 8;                                                             \
  }                                                                                                                             \
  const int tz = tile_b % ntz;                                                                                                  \
  tile_b /= ntz;                                                                                                                \
  const int ty = tile_b % nty;                                                                                                  \
  const int tx = tile_b / nty;                                                                                                  \
  [[maybe_unused]] const bool surplus = tx * LX >= g.nx;                                                                        \
  const int j0 = tile_min(ty * TileShape<TYR, ZS>::TYU, g.ny - TileShape<TYR, ZS>::TYU),                                        \
            kp0 = tile_min(tz * TileShape<TYR, ZS>::TZU, nzh - TileShape<TYR, ZS>::TZU), x0 = surplus ? 0 : tx * LX;            \
  const int jr = j0 - 1 + r;                                                                                                    \
  [[maybe_unused]] const int j = jr < 0 ? jr + g.ny : (jr >= g.ny ? jr - g.ny : jr);                                            \
  const int kr = TileShape<TYR, ZS>::FULLROW ? li : kp0 - 1 + l;                                                                \
  [[maybe_unused]] const int kp = kr < 0 ? kr + nzh : (kr >= nzh ? kr - nzh : kr);                                              \
  [[maybe_unused]] const bool own = r >= 1 && r <= TileShape<TYR, ZS>::TYU && jr >= ty * TileShape<TYR, ZS>::TYU &&             \
                                    (TileShape<TYR, ZS>::FULLROW ||                                                             \
                                     (l >= 1 && l <= TileShape<TYR, ZS>::TZU && kr >= tz * TileShape<TYR, ZS>::TZU));           \
  const long rowoff = (long)j * g.nzp + 2 * kp;                                                                                 \
  [[maybe_unused]] const int rm = r > 0 ? r - 1 : 0, rp = r + 1 < TYR ? r + 1 : TYR - 1;                                        \
  [[maybe_unused]] const double hx = g.hx, hy = g.hy, hz = g.hz;                                                                \
  [[maybe_unused]] const int nsteps = surplus ? (SURPLUS_NSTEPS) : (x0 + LX <= g.nx ? LX : g.nx - x0);                          \
  [[maybe_unused]] auto plane = [&](int q) {                                                                                    \
    constexpr XWrap tile_wrap = WRAP;                                                                                           \
    const int x = tile_wrap == XWrap::slab ? (q < 0 ? q + g.xw_lo : (q >= g.nx ? q - g.xw_hi : q))                                 \
                                        : (q < 0 ? q + g.nx : (q >= g.nx ? q - g.nx : q));                                      \
    return (long)x * g.nyzp + rowoff;                                                                                           \
  }

// FG_TILE_FRAME as a function that returns its locals and the offsets of planes x0 - 2 .. x0 + nsteps + 1 (tests)
struct TileFrame {
  int r, zs, l, li, zprev, znext, rm, rp, j, kp;
  bool own, surplus;
  long rowoff;
  int x0, nsteps;
  long plane[64 + 4];   // plane[i] = plane(x0 - 2 + i)
};

template <int TYR, int ZS, XWrap WRAP>
inline TileFrame tile_frame(const Grid& g, int nty, int ntz, int LX, int block, int nblocks, unsigned thread, int surplus_nsteps) {
  FG_TILE_FRAME(TYR, ZS, WRAP, surplus_nsteps, g, nty, ntz, LX, block, nblocks, thread);
  TileFrame t{r, zs, l, li, zprev, znext, rm, rp, j, kp, own, surplus, rowoff, x0, nsteps, {}};
  for (int q = x0 - 2; q <= x0 + nsteps + 1; ++q) t.plane[q - (x0 - 2)] = plane(q);
  return t;
}

}  // namespace fg
