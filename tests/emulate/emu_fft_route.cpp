// Stand-alone driver of fibergen_amd/csrc/fg_fft_route.h (tests/test_fft_route.py): prints the route of every length 1 ... 2048
// on each axis in the format of tests/golden/fft_routes.txt.gz, and checks the routes against the resource predicates of the
// one-kernel sub-line launchers.  A FAIL line per broken property, OK as the last line.
#include <cstdio>

#include "../../fibergen_amd/csrc/fg_fft_route.h"

using namespace fg::fft;

// the limits, spelled out once more as figures: 1024 threads (512 fused), 144 KB
static_assert(sub_one_strided_fits(128, 7) && !sub_one_strided_fits(128, 9) && !sub_one_strided_fits(256, 5), "m p <= 1024");
static_assert(sub_one_fused_fits(128, 3) && !sub_one_fused_fits(128, 5) && !sub_one_fused_fits(256, 3), "fused: m p <= 512");
static_assert(sub_tile_lds(128, 7) == 129024 && sub_tile_lds(256, 5) == 184320, "two planes of p * 8 padded sub-lines");
static_assert(sub_z_lines(8, 3) == 85 && sub_z_threads(8, 3) == 255 && sub_z_lines(256, 9) == 1 && sub_z_threads(256, 9) == 288, "z");
static_assert(sub_z_lds(8, 3) == 85 * 3 * 9 * 16 && sub_z_lds(256, 9) == 288 * 9 * 16 && sub_one_z_fits(256, 9), "z: about 256 threads whatever the row");
static_assert(sub_one_m(8) && sub_one_m(256) && !sub_one_m(4) && !sub_one_m(512) && !sub_one_m(48), "m in 8 ... 256");

static const char* kName[] = {"len1", "pow2", "sub_one", "sub_lds", "sub_scratch", "tile", "bluestein", "quadratic"};

static void plan(const fg::fft::SmoothPlan& s) {
  printf(" %d/%d/%d.%d.%d.%d/%d/%d/%d/%d", s.n, s.npass, s.fac[0], s.fac[1], s.fac[2], s.fac[3], s.lines, s.threads, s.cap, s.joint);
}

int main() {
  int fails = 0;
  auto check = [&](bool ok, const char* what, int axis, int n) {
    if (!ok) printf("FAIL %s: axis %d, length %d\n", what, axis, n), ++fails;
  };
  printf("# axis len family path p m plan(n/npass/fac/lines/threads/cap/joint) bluestein_m zodd [x, y: fused kind for (ncomp, joint_x) = (1,on) (3,on) (1,off) (3,off), x: each with its plan]\n");
  for (int axis = 0; axis < 3; ++axis)
    for (int n = 1; n <= 2048; ++n) {
      const AxisRoute r = route_axis(axis, n);
      printf("%d %d %s %d %d %d", axis, n, kName[(int)r.family], path_of(r.family), r.p, r.m);
      plan(r.plan);
      printf(" %d %d", r.blue.m(), r.zodd ? 1 : 0);
      if (axis < 2)
        for (int joint = 1; joint >= 0; --joint)
          for (int nc : {1, 3}) {
            const FusedXRoute f = route_fused_x(n, nc, joint != 0, axis);
            printf(" %d", (int)f.kind);
            if (axis == 0) plan(f.plan);
            // the fused sub-line launcher: named exactly where its predicate holds
            check((f.kind != Fused::Sub) || (sub_one_fused(f.p, f.m) && f.p * f.m == n), "fused sub-line route outside its launcher", axis, n);
            check(f.kind != Fused::None || nc != 3 || !sub_one_fused(r.p, r.m) || (axis == 0 && r.family == Family::Tile),
                  "fused sub-line launcher left unused", axis, n);
            check((f.kind == Fused::Tile) == (f.plan.n != 0), "fused tile route without its plan", axis, n);
          }
      printf("\n");
      const bool launcher = axis == 2 ? sub_one_z(r.p, r.m) : sub_one_strided(r.p, r.m);
      if (r.family == Family::SubOne) check(launcher, "one-kernel route outside its launcher's limits", axis, n);
      if (r.family == Family::SubLds || r.family == Family::SubScratch) check(!launcher, "combine sweep where the one-kernel launcher fits", axis, n);
      if (r.p) check(r.p * r.m == r.line && fast_len(r.m) && r.pass_twiddles == r.m, "p m != line", axis, n);
      check((r.family == Family::Tile) == (r.plan.n != 0), "tile route and plan disagree", axis, n);
      check((r.family == Family::Bluestein) == (r.blue.n != 0), "Bluestein route and plan disagree", axis, n);
      if (r.family == Family::Bluestein) check(path_of(r.resolved(false)) == 5 && path_of(r.resolved(true)) == 4, "Bluestein off", axis, n);
      else check(r.resolved(false) == r.family, "Bluestein switch moved another family", axis, n);
      check((r.family == Family::Pow2) == (r.half_roots || r.z_roots) && (r.family == Family::Pow2) != (r.unit_roots && r.scratch), "tables", axis, n);
    }
  printf(fails ? "FAILED\n" : "OK\n");
  return fails ? 1 : 0;
}
