// Host emulation of the Bluestein tile kernels' thread bodies (fg_fft_bluestein.h; test infrastructure): the phases of
// k_bluestein_strided / k_bluestein_z for every thread of every workgroup, in the device's order
//   load | barrier | (c2r, even nz: merge | barrier) | passes | filter | barrier | passes | store
// with the plans and the tables the library makes.  Build with g++ -DFG_HOST_EMULATION.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../fibergen_amd/csrc/fg_fft_kernels.h"
#include "../../fibergen_amd/csrc/fg_fft_plane.h"
#include "../../fibergen_amd/csrc/fg_fft_smooth.h"
#include "../../fibergen_amd/csrc/fg_fft_smooth_plans.h"
#include "../../fibergen_amd/csrc/fg_fft_tables.h"
#include "../../fibergen_amd/csrc/fg_fft_bluestein.h"

using namespace fg;
using namespace fg::fft;

// one forward pass set of the tile in the image: per pass every (virtual) thread reads and transforms its butterfly, then --
// behind the barrier -- every thread writes it
static void emu_bluestein_passes(cplx* img, const SmoothPlan& plan, const SmoothMap& L, const cplx* w) {
  constexpr int QMAX = 8;   // a thread owns up to smooth_rounds(R) butterflies: virtual threads tid + q * threads
  std::vector<cplx> regs((size_t)plan.threads * QMAX * kSmoothMaxRadix);
  std::vector<char> active((size_t)plan.threads * QMAX);
  int Ns = 1;
  for (int f = 0; f < plan.npass; ++f) {
    const int R = plan.fac[f];
    const int nvirt = plan.threads * (plan.cap ? smooth_rounds(R, plan.cap) : 1);
    for (int half = 0; half < 2; ++half)
      for (int tid = 0; tid < nvirt; ++tid) {
        cplx* v = &regs[(size_t)tid * kSmoothMaxRadix];
        switch (R) {
#define FG_R(r)                                                                                   \
  case r:                                                                                         \
    if (half == 0) active[tid] = smooth_pass_read<r, -1, true>(img, plan.n, Ns, L, w, 1, tid, v); \
    else if (active[tid]) smooth_pass_write<r, true>(img, plan.n, Ns, L, tid, v);                 \
    break;
          FG_R(2) FG_R(3) FG_R(4) FG_R(5) FG_R(6) FG_R(7) FG_R(8) FG_R(9) FG_R(10) FG_R(11) FG_R(12) FG_R(13) FG_R(14) FG_R(15)
          FG_R(16) FG_R(18) FG_R(20) FG_R(21) FG_R(22) FG_R(24) FG_R(25) FG_R(26) FG_R(27) FG_R(28) FG_R(30) FG_R(32)
#undef FG_R
          default: std::abort();
        }
      }
    Ns *= R;
  }
}

static void emu_bluestein_middle(cplx* img, const SmoothPlan& plan, const BluesteinGeom& G, const BluesteinTables& t) {
  const SmoothMap L = G.map();
  emu_bluestein_passes(img, plan, L, t.w);
  for (int tid = 0; tid < plan.threads; ++tid) bluestein_filter(G, t.filter, tid, plan.threads, img);
  emu_bluestein_passes(img, plan, L, t.w);
}

extern "C" {

// the planner: kind 0 strided, 1 z.  out = {M, lines, threads, passes, image bytes}; returns 1 when the length has no plan
int emu_bluestein_plan(int kind, int n, long* out) {
  BluesteinPlan p;
  if (!(kind == 0 ? bluestein_plan_strided(n, &p) : bluestein_plan_z(n, &p))) return 1;
  const BluesteinGeom G = kind == 0 ? bluestein_geom_strided(p.pass) : bluestein_geom_z(p.pass);
  out[0] = p.m(), out[1] = p.pass.lines, out[2] = p.pass.threads, out[3] = p.pass.npass, out[4] = (long)G.lds_bytes();
  return 0;
}

long emu_bluestein_lds_max() { return (long)kSmoothLdsMax; }
int emu_bluestein_min() { return kBluesteinMin; }

// c2c along the strided axis of data[nouter][n][ncols] (ls = ncols, os = n * ncols)
int emu_bluestein_strided(int n, int dir, double* data, int ncols, int nouter, double scale) {
  BluesteinPlan bp;
  if (!bluestein_plan_strided(n, &bp)) return 1;
  const std::vector<cplx> chirp = make_bluestein_chirp(n), filter = make_bluestein_filter(n, bp.m()), w = make_unit_roots(bp.m(), bp.m());
  BluesteinArgs a;
  a.data = reinterpret_cast<cplx*>(data);
  a.ls = ncols;
  a.os = (long)n * ncols;
  a.ncols = ncols;
  a.plan = bp.pass;
  const int C = a.plan.lines, T = a.plan.threads;
  a.tiles_per_outer = (ncols + C - 1) / C;
  a.scale = scale;
  a.nt = 0;
  a.dir = dir;
  a.n = n;
  a.t = BluesteinTables{chirp.data(), filter.data(), w.data()};
  const BluesteinGeom G = bluestein_geom_strided(a.plan);
  std::vector<cplx> img(G.lds_bytes() / sizeof(cplx));
  for (int b = 0; b < a.tiles_per_outer * nouter; ++b) {
    for (auto& x : img) x = cmake(NAN, NAN);
    for (int tid = 0; tid < T; ++tid) bluestein_strided_load<8>(a, G, b, tid, T, img.data());
    emu_bluestein_middle(img.data(), a.plan, G, a.t);
    for (int tid = 0; tid < T; ++tid) bluestein_strided_store(a, G, b, tid, T, img.data());
  }
  return 0;
}

// r2c (fwd = 1) / c2r (fwd = 0) of the rows data[nrows][2 (nz / 2 + 1)], even and odd nz
int emu_bluestein_z(int nz, int fwd, double* data, long nrows) {
  const int odd = nz % 2, n = odd ? nz : nz / 2;
  BluesteinPlan bp;
  if (!bluestein_plan_z(n, &bp)) return 1;
  const std::vector<cplx> chirp = make_bluestein_chirp(n), filter = make_bluestein_filter(n, bp.m()), w = make_unit_roots(bp.m(), bp.m());
  const std::vector<cplx> wz = make_unit_roots(nz, nz);
  BluesteinZArgs a;
  a.data = data;
  a.nrows = nrows;
  a.nzp = 2 * (nz / 2 + 1);
  a.nt = 0;
  a.fwd = fwd;
  a.odd = odd;
  a.n = n;
  a.t = BluesteinTables{chirp.data(), filter.data(), w.data()};
  a.wz = wz.data();
  a.plan = bp.pass;
  const BluesteinGeom G = bluestein_geom_z(a.plan);
  const int lines = a.plan.lines, T = a.plan.threads;
  std::vector<cplx> img(G.lds_bytes() / sizeof(cplx));
  for (long b = 0; b * lines < nrows; ++b) {
    for (auto& x : img) x = cmake(NAN, NAN);
    const long row0 = b * lines;
    for (int tid = 0; tid < T; ++tid) bluestein_z_load<8>(a, G, row0, tid, T, img.data());
    if (!odd && !fwd)
      for (int tid = 0; tid < T; ++tid) bluestein_z_merge(a, G, tid, T, img.data());
    emu_bluestein_middle(img.data(), a.plan, G, a.t);
    for (int tid = 0; tid < T; ++tid) bluestein_z_store(a, G, row0, tid, T, img.data());
  }
  return 0;
}
}
