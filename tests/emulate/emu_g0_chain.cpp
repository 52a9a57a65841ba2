// C shim around fibergen_amd/csrc/fg_g0_chain.h and hostmath::bc_correction (fg_hostmath.h) for tests/test_g0_chain.py: both
// are host code, so the very schedule Solver::fft_g0_chain runs is driven here by a site that only records.  One text line
// per pass the chain calls:
//   <slot open at the time, -1 = none> <pass> <ncomp> <dir, 0 = none> <scale, - = none> <window: all | x0+np> <buffer> [...]
// buffer: buf | scratch, the y passes of the x layout buf>scratch | scratch>buf; fused_x and green append their constants.
// A time_end that does not close the open slot, or a slot left open, is a line of its own ("bad ...").
#include <cstdio>
#include <string>

#include "../../fibergen_amd/csrc/fg_g0_chain.h"
#include "../../fibergen_amd/csrc/fg_hostmath.h"

using namespace fg;

namespace {

struct Recorder {
  double *buf, *scratch;
  std::string out;
  int open = -1;
  const char* name(const double* p) const { return p == buf ? "buf" : (p == scratch ? "scratch" : "?"); }
  std::string win(int x0, int np) const { return np < 0 ? "all" : std::to_string(x0) + "+" + std::to_string(np); }
  void line(const char* pass, int ncomp, int dir, const double* scale, const std::string& w, const std::string& where,
            const std::string& tail = "") {
    char s[64] = "-";
    if (scale) std::snprintf(s, sizeof s, "%g", *scale);
    out += std::to_string(open) + " " + pass + " " + std::to_string(ncomp) + " " + std::to_string(dir) + " " + s + " " + w + " " +
           where + tail + "\n";
  }
  static std::string consts(double c10, double c20) {
    char s[96];
    std::snprintf(s, sizeof s, " c10=%g c20=%g", c10, c20);
    return s;
  }
  void time_begin(int slot) {
    if (open != -1) out += "bad time_begin " + std::to_string(slot) + " inside " + std::to_string(open) + "\n";
    open = slot;
  }
  void time_end(int slot) {
    if (open != slot) out += "bad time_end " + std::to_string(slot) + " with " + std::to_string(open) + " open\n";
    open = -1;
  }
  void chain_r2c_z(double* b, int nc, int x0, int np) { line("r2c_z", nc, -1, nullptr, win(x0, np), name(b)); }
  void chain_c2r_z(double* b, int nc, int x0, int np) { line("c2r_z", nc, +1, nullptr, win(x0, np), name(b)); }
  void chain_c2c_y(double* b, int nc, int dir, double scale, int x0, int np) { line("c2c_y", nc, dir, &scale, win(x0, np), name(b)); }
  void chain_c2c_y_xlayout(double* in, double* o, int nc, int dir, int x0, int np) {
    line("c2c_y_xlayout", nc, dir, nullptr, win(x0, np), std::string(name(in)) + ">" + name(o));
  }
  void chain_c2c_x(double* b, int nc, int dir, double scale) { line("c2c_x", nc, dir, &scale, "all", name(b)); }
  void chain_zy_plane(double* b, int nc, int dir) { line("zy_plane", nc, dir, nullptr, "all", name(b)); }
  void chain_scale(double* b, int nc, double scale) { line("scale", nc, 0, &scale, "all", name(b)); }
  void chain_fused_x(double* d, int nc, double scale, double c10, double c20, bool xlayout) {
    line("fused_x", nc, 0, &scale, "all", name(d), std::string(xlayout ? " xl=1" : " xl=0") + consts(c10, c20));
  }
  void chain_green(double* b, int nc, double c10, double c20) { line("green", nc, 0, nullptr, "all", name(b), consts(c10, c20)); }
};

hostmath::Mat6 mat6(const double* a36) {
  hostmath::Mat6 m;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) m.a[i][j] = a36[6 * i + j];
  return m;
}

}  // namespace

extern "C" {

// Returns the length of the trace (the first cap - 1 characters of it are in out, zero-terminated).
int emu_g0_chain(int ncomp, int nx, int has_x, int has_y, int xlayout, int plane, int pair_chunk, int fuse_x, double scale,
                 double c10, double c20, char* out, int cap) {
  double buf[1], scratch[1];
  Recorder r{buf, scratch};
  G0ChainPlan p;
  p.ncomp = ncomp;
  p.nx = nx;
  p.has_x = has_x != 0;
  p.has_y = has_y != 0;
  p.xlayout = xlayout != 0;
  p.plane = plane != 0;
  p.pair_chunk = pair_chunk;
  p.fuse_x = fuse_x != 0;
  p.scale = scale;
  p.c10 = c10;
  p.c20 = c20;
  g0_chain(r, p, buf, scratch);
  if (r.open != -1) r.out += "bad end: slot " + std::to_string(r.open) + " left open\n";
  std::snprintf(out, cap, "%s", r.out.c_str());
  return (int)r.out.size();
}

// matrices row-major 6 x 6
void emu_bc_correction(const double* MQ, const double* M, const double* QC0, double bc_relax, double alpha, const double* F0,
                       const double* F00, double* R) {
  hostmath::bc_correction(mat6(MQ), mat6(M), mat6(QC0), bc_relax, alpha, F0, F00, R);
}

}  // extern "C"
