// The transform chain of one operator pass -- forward transform, Green operator in Fourier space, inverse transform on one or
// three components (fftVector F:18481-18510, G0OperatorFourierStaggered F:19749-19755 / G0OperatorStaggeredHeat F:20118-20135) --
// as Solver::fft_g0_chain runs it for every solver loop, written once: the skeleton owns the order of the calls and the timing
// slot each one is charged to; the decisions come in as a plain struct the caller fills once, and what a call does is the
// site's (DESIGN.md has the table).  Host code without any HIP in it, like fg_cg_loop.h, and driven on its own by
// tests/test_g0_chain.py.
#pragma once

namespace fg {

// Filled once per chain (Solver::fft_g0_chain); nothing here is decided a second time.  The order of the decisions is the
// caller's: x layout before plane, plane before pair chunk (at most one of xlayout / plane is set, pair_chunk is 0 with plane).
struct G0ChainPlan {
  int ncomp;        // 1 (heat / porous: the potential) or 3 (displacement)
  int nx;           // x planes of the field: what the windows of pair_chunk run over
  bool has_x, has_y;   // nx > 1, ny > 1: where the 1/N rides depends on which passes exist
  bool xlayout;     // the spectrum passes through the scratch in the x-contiguous layout (implies fuse_x)
  bool plane;       // z and y transforms of a z-y plane in one kernel
  int pair_chunk;   // > 0: z and y passes in runs of this many x planes, r2c(w) -> y(w) and y^-1(w) -> c2r(w)
  bool fuse_x;      // x transform + 1/N + Green operator + inverse x transform in one kernel
  double scale;     // 1/N
  double c10, c20;  // the Green operator's two constants
};

// Site (Solver) supplies the passes -- a window is (x0, np) with np < 0 for the whole field -- and the timing slots:
//   chain_r2c_z(buf, ncomp, x0, np)                    chain_c2r_z(buf, ncomp, x0, np)
//   chain_c2c_y(buf, ncomp, dir, scale, x0, np)        chain_c2c_y_xlayout(in, out, ncomp, dir, x0, np)
//   chain_c2c_x(buf, ncomp, dir, scale)                chain_zy_plane(buf, ncomp, dir)
//   chain_scale(buf, ncomp, scale)
//   chain_fused_x(data, ncomp, scale, c10, c20, xlayout)     the fused x pass, in place on data
//   chain_green(buf, ncomp, c10, c20)                         the Green operator as its own kernel
//   time_begin(slot), time_end(slot)
// Slots (StageTimes): 2 r2c_z  3 y forward  4 x forward  5 Green operator (or the fused pass)  6 x inverse  7 y inverse  8 c2r_z;
// a fused pair (plane kernel, chunked pairs) is charged to the slot of its outer pass.
template <class Site>
void g0_chain(Site& site, const G0ChainPlan& p, double* buf, double* xscratch) {
  const int nc = p.ncomp;
  // the 1/N of F:18501-18506 rides on the last forward pass there is: x, else y; with neither it is a sweep of its own
  const double y_scale = (p.has_x || !p.has_y) ? 1.0 : p.scale;
  auto y_forward = [&](int x0, int np) {
    if (p.xlayout) site.chain_c2c_y_xlayout(buf, xscratch, nc, -1, x0, np);
    else site.chain_c2c_y(buf, nc, -1, y_scale, x0, np);
  };
  auto y_inverse = [&](int x0, int np) {
    if (p.xlayout) site.chain_c2c_y_xlayout(xscratch, buf, nc, +1, x0, np);
    else site.chain_c2c_y(buf, nc, +1, 1.0, x0, np);
  };
  // first(w) then second(w) for every run w of pair_chunk x planes
  auto pairs = [&](auto first, auto second) {
    for (int x0 = 0; x0 < p.nx; x0 += p.pair_chunk) {
      const int np = p.nx - x0 < p.pair_chunk ? p.nx - x0 : p.pair_chunk;
      first(x0, np);
      second(x0, np);
    }
  };
  auto r2c = [&](int x0, int np) { site.chain_r2c_z(buf, nc, x0, np); };
  auto c2r = [&](int x0, int np) { site.chain_c2r_z(buf, nc, x0, np); };

  if (p.plane) {
    site.time_begin(2);
    site.chain_zy_plane(buf, nc, -1);
    site.time_end(2);
  } else if (p.pair_chunk) {
    site.time_begin(2);
    pairs(r2c, y_forward);
    site.time_end(2);
  } else {
    site.time_begin(2);
    r2c(0, -1);
    site.time_end(2);
    site.time_begin(3);
    y_forward(0, -1);
    site.time_end(3);
  }

  if (p.fuse_x) {
    site.time_begin(5);
    site.chain_fused_x(p.xlayout ? xscratch : buf, nc, p.scale, p.c10, p.c20, p.xlayout);
    site.time_end(5);
  } else {
    site.time_begin(4);
    site.chain_c2c_x(buf, nc, -1, p.has_x ? p.scale : 1.0);
    site.time_end(4);
    if (!p.has_x && !p.has_y) site.chain_scale(buf, nc, p.scale);
    site.time_begin(5);
    site.chain_green(buf, nc, p.c10, p.c20);
    site.time_end(5);
    site.time_begin(6);
    site.chain_c2c_x(buf, nc, +1, 1.0);
    site.time_end(6);
  }

  if (p.plane) {
    site.time_begin(8);
    site.chain_zy_plane(buf, nc, +1);
    site.time_end(8);
  } else if (p.pair_chunk) {
    site.time_begin(7);
    pairs(y_inverse, c2r);
    site.time_end(7);
  } else {
    site.time_begin(7);
    y_inverse(0, -1);
    site.time_end(7);
    site.time_begin(8);
    c2r(0, -1);
    site.time_end(8);
  }
}

}  // namespace fg
