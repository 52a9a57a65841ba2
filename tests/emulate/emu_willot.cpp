// C shim around fibergen_amd/csrc/fg_willot_math.h for tests/test_willot_oracle.py: the per-frequency function the kernel
// k_gamma_willot calls and the table builder the solver calls run here on a whole half spectrum [6][nx][ny][nzc] (no padding).
#include "../../fibergen_amd/csrc/fg_willot_math.h"

using namespace fg;

extern "C" {

// th: six components of nx * ny * nzc interleaved complex doubles, in place; the zero frequency is set to E
void emu_willot_apply(int nx, int ny, int nz, double dx, double dy, double dz, double mu_0, double lambda_0, double alpha,
                      double beta, const double* E, double* th) {
  const int nzc = nz / 2 + 1;
  std::vector<double> t[3];
  std::vector<cplx> e[3];
  willot_axis_table(nx, dx, nx, &t[0], &e[0]);
  willot_axis_table(ny, dy, ny, &t[1], &e[1]);
  willot_axis_table(nz, dz, nzc, &t[2], &e[2]);
  const bool inf = std::isinf(lambda_0);
  const WillotCoef cf = willot_coef(mu_0, lambda_0, inf, alpha, beta);
  const long nfreq = (long)nx * ny * nzc;
  cplx* c = reinterpret_cast<cplx*>(th);
  for (int ii = 0; ii < nx; ++ii)
    for (int jj = 0; jj < ny; ++jj)
      for (int kk = 0; kk < nzc; ++kk) {
        const long idx = ((long)ii * ny + jj) * nzc + kk;
        cplx tv[6], ey[6];
        for (int q = 0; q < 6; ++q) tv[q] = c[q * nfreq + idx];
        if (ii == 0 && jj == 0 && kk == 0) {
          for (int q = 0; q < 6; ++q) ey[q] = cmake(E[q], 0.0);
        } else {
          const double ta[3] = {t[0][ii], t[1][jj], t[2][kk]};
          const cplx e012 = cmul(cmul(e[0][ii], e[1][jj]), e[2][kk]);
          if (inf) willot_point<true>(ta, e012, cf, tv, ey);
          else willot_point<false>(ta, e012, cf, tv, ey);
        }
        for (int q = 0; q < 6; ++q) c[q * nfreq + idx] = ey[q];
      }
}

}  // extern "C"
