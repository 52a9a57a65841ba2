// Which transform family runs an axis of Fft3, decided once.  Six families grew over six rounds -- power of two, the one-kernel
// p * 2^k passes, sub-lines plus a combine sweep, the Stockham tile plans, Bluestein, the O(n^2) sums -- and the constructor, the
// entry points, can_fuse() and path() each used to re-derive the choice from a handful of members.  Here it is one function per
// question: route_axis() for a z / y / x pass, route_fused_x() for the fused Green-operator pass, and the resource limits of the
// one-kernel sub-line launchers as constexpr predicates that the launchers (`if constexpr`) and the routes share.  DESIGN.md
// has the table of lengths, families and the measurements behind the thresholds.  Host code without any HIP in it, like
// fg_g0_chain.h, and walked over every length 1 ... 2048 by tests/test_fft_route.py.
#pragma once

#include "fg_fft_bluestein.h"

namespace fg {
namespace fft {

enum class Family {
  Len1,        // nothing to transform (the z pass still copies the row through the O(n^2) sweep)
  Pow2,        // 8 ... 1024 points: the register / LDS kernels of fg_fft_kernels.h
  SubOne,      // p * 2^k, one kernel for the whole pass (k_strided_mixed, k_z_mixed)
  SubLds,      // p * 2^k, power-of-two kernels on the p sub-lines + a combine sweep in place through LDS
  SubScratch,  // the same with the combine sweep through the scratch component (lines above 1152 points; x and y only)
  Tile,        // 13-smooth: the Stockham tile kernels of fg_fft_smooth.h
  Bluestein,   // a prime factor above 13, from kBluesteinMin points on (set_bluestein(false): Quadratic)
  Quadratic    // O(n^2) sums through the scratch component
};

constexpr int kMaxOddFactor = 25;              // 25: the decimal sizes 200, 400, 800
constexpr size_t kSubLdsMax = 144 * 1024;      // LDS a sub-line kernel may ask for
constexpr int kSubTileMin[3] = {100, 100, 72}; // per axis: from this line length on a tile plan beats the one-kernel sub-line pass

constexpr bool fast_len(int n) { return is_pow2(n) && n >= 8 && n <= 1024; }
constexpr int mixed_factor(int n) {   // p if n = p * 2^k with 2^k a fast length, else 0
  for (int p = 3; p <= kMaxOddFactor; p += 2)
    if (n % p == 0 && fast_len(n / p)) return p;
  return 0;
}

// ---- the one-kernel sub-line launchers: p in {3, 5, 7, 9} ({3, 5} fused), sub-lines of m in {8 ... 256} points
constexpr bool sub_one_p(int p) { return p == 3 || p == 5 || p == 7 || p == 9; }
constexpr bool sub_one_m(int m) { return is_pow2(m) && m >= 8 && m <= 256; }
// strided and fused pass: m * p threads, two exchange planes of p * 8 padded sub-lines
constexpr size_t sub_tile_lds(int m, int p) { return (size_t)2 * (m + m / 8) * p * 8 * sizeof(double); }
constexpr bool sub_one_strided_fits(int m, int p) { return m * p <= 1024 && sub_tile_lds(m, p) <= kSubLdsMax; }
// (N <= 512 like the power-of-two fused pass: 640 and 768 need 0.9-1.3 KB of scratch per lane)
constexpr bool sub_one_fused_fits(int m, int p) { return m * p <= 512 && sub_tile_lds(m, p) <= kSubLdsMax; }
// z pass: LINES packed rows per workgroup
constexpr int sub_z_lines(int mp, int p) { return 2048 / (mp * p) > 1 ? 2048 / (mp * p) : 1; }
constexpr int sub_z_threads(int mp, int p) { return (mp / 8) * p * sub_z_lines(mp, p); }
constexpr size_t sub_z_lds(int mp, int p) {
  const size_t ex = (size_t)2 * (mp + mp / 8) * p * sub_z_lines(mp, p) * sizeof(double);
  const size_t im = (size_t)sub_z_lines(mp, p) * p * mp * sizeof(cplx);
  return ex > im ? ex : im;
}
constexpr bool sub_one_z_fits(int mp, int p) { return sub_z_threads(mp, p) <= 1024 && sub_z_lds(mp, p) <= kSubLdsMax; }

constexpr bool sub_one_strided(int p, int m) { return sub_one_p(p) && sub_one_m(m) && sub_one_strided_fits(m, p); }
constexpr bool sub_one_z(int p, int mp) { return sub_one_p(p) && sub_one_m(mp) && sub_one_z_fits(mp, p); }
constexpr bool sub_one_fused(int p, int m) { return (p == 3 || p == 5) && sub_one_m(m) && sub_one_fused_fits(m, p); }

// An x length whose three components have no joint image plan (384 = 3 * 2^7: 9 216 points of a tile against 512 threads x 20
// values) keeps the sub-line kernels' fused x pass where there is one: 384^3 fused x 1 114 us against 1 732 us in the R <= 32
// class kernel (238 -> 263 it/s).  The x axis' own passes then stay on the sub-line kernels too.  (Asked with joint_x on, its
// default: set_joint_x() does not move an axis between families.)
inline bool x_keeps_subline_fused(int nx, int p) {
  if (!p || !sub_one_fused(p, nx / p)) return false;
  SmoothPlan three;
  smooth_plan_xfused(nx, 3, &three);
  return three.joint != 3;
}

struct AxisRoute {
  Family family = Family::Quadratic;   // with Bluestein on; see resolved()
  int line = 0;          // complex points of a line: the length, z: nz / 2, odd nz: nz
  int p = 0, m = 0;      // line = p * m, p odd <= 25, m a fast length (0: no such p).  Set whichever family runs the axis:
                         // the fused sub-line pass of a y-slab uses it beside a tile plan
  SmoothPlan plan;       // Tile
  BluesteinPlan blue;    // Bluestein: kept when set_bluestein(false) turns the family into Quadratic
  bool zodd = false;     // odd nz on a tile plan: the rows as nz complex points
  // tables and scratch the constructor uploads / allocates
  int pass_twiddles = 0; // != 0: pass twiddles of this power-of-two length
  bool half_roots = false, z_roots = false;   // e^{-i pi j / n} (fused pass of a power-of-two x / y); e^{-2 pi i k / nz}, k <= nz / 2
  bool unit_roots = false, scratch = false;   // e^{-2 pi i k / n}, k < n; one scratch component
  Family resolved(bool bluestein_on) const { return family == Family::Bluestein && !bluestein_on ? Family::Quadratic : family; }
};

// axis 0, 1: lines of len points (x, y); axis 2: rows of len reals (z)
inline AxisRoute route_axis(int axis, int len) {
  AxisRoute r;
  const bool z = axis == 2;
  r.line = z ? (len % 2 ? len : len / 2) : len;
  if (z ? (len % 2 == 0 && fast_len(len / 2)) : fast_len(len)) {
    r.family = Family::Pow2;
    r.pass_twiddles = r.line;
    r.half_roots = !z;
    r.z_roots = z;
    return r;
  }
  r.unit_roots = r.scratch = true;
  const int m = z && len % 2 ? 0 : r.line;   // what the packed-real trick / the strided kernels would transform
  if (z && len % 2 == 1 && len > 1 && smooth_plan_z(len, &r.plan)) r.zodd = true;
  r.p = m ? mixed_factor(m) : 0;
  r.m = r.p ? m / r.p : 0;
  r.pass_twiddles = r.m;
  // Where a one-kernel p * 2^k pass exists it stays below kSubTileMin points; everything else with a tile plan takes the plan
  const bool keep_sub_one = sub_one_p(r.p) && m <= 1024 && m < kSubTileMin[axis];
  if (m > 1 && !keep_sub_one) z ? smooth_plan_z(m, &r.plan) : smooth_plan_strided(m, &r.plan);
  if (axis == 0 && r.plan.n && x_keeps_subline_fused(len, r.p)) r.plan = SmoothPlan();
  if (len == 1) r.family = Family::Len1;
  else if (r.plan.n) r.family = Family::Tile;
  else if (r.p) {
    if (z ? sub_one_z(r.p, r.m) : sub_one_strided(r.p, r.m)) r.family = Family::SubOne;
    else r.family = z || (size_t)len * 8 * sizeof(cplx) <= kSubLdsMax ? Family::SubLds : Family::SubScratch;
  } else if (z ? bluestein_plan_z(r.line, &r.blue) : bluestein_plan_strided(r.line, &r.blue)) r.family = Family::Bluestein;
  return r;
}

// Fft3::path(): the six-valued summary the fft_path_* counters report
constexpr int path_of(Family f) {
  return f == Family::Len1 ? 0 : f == Family::Pow2 ? 1 : f == Family::Tile ? 3 : f == Family::Bluestein ? 4 : f == Family::Quadratic ? 5 : 2;
}

// ---- the fused pass: transform, 1/N, Green operator, inverse transform in one kernel (x of the field; y of a y-slab: axis 1)
enum class Fused { None, Pow2, Tile, Sub };
struct FusedXRoute {
  Fused kind = Fused::None;
  int p = 0, m = 0;   // Sub
  SmoothPlan plan;    // Tile
};

inline FusedXRoute route_fused_x(int n, int ncomp, bool joint, int axis = 0) {
  FusedXRoute f;
  const AxisRoute r = route_axis(axis, n);
  if (r.family == Family::Pow2) {
    f.kind = Fused::Pow2;
  } else if (axis == 0 && r.family == Family::Tile && (ncomp == 1 || ncomp == 3)) {
    if (smooth_plan_xfused(n, ncomp, &f.plan, joint)) f.kind = Fused::Tile;
  } else if (ncomp == 3 && sub_one_fused(r.p, r.m)) {   // p * 2^k with p = 3, 5: the three-component form only
    f.kind = Fused::Sub;
    f.p = r.p, f.m = r.m;
  }
  return f;
}

}  // namespace fft
}  // namespace fg
