// Host build of the general-phase arithmetic of fibergen_amd/csrc/fg_stage_math.h for tests/test_general_emulation.py:
// general6, pk1_voigt over mixed isotropic / general phases and the reference-material scan's tangent_eigs (Jacobi).
// One case = three phases: in[126] = law[3], mu[3], lambda[3], C[3][36], phi[3], F[6];
//                         out[14] = general6(F, C[0], 1) [6], pk1_voigt(F, phi, alpha = 1) [6], emin, emax of the Voigt tangent.
// Built as a shared library (ctypes) and, with -DEMU_GENERAL_MAIN, as a stand-alone program `emu_general in out` on files of
// raw doubles (the sanitizer run).
#include <cstdio>
#include <vector>

#include "../../fibergen_amd/csrc/fg_stage_math.h"

using namespace fg;

extern "C" {

void emu_general_case(const double* in, double* out) {
  PhaseTable pt;
  pt.n = 3;
  for (int p = 0; p < kMaxPhases; ++p) {
    pt.law[p] = kLawIso;
    pt.mu[p] = pt.lambda[p] = 0.0;
    for (int k = 0; k < 36; ++k) pt.C[p][k] = 0.0;
  }
  double phi[kMaxPhases] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = 0; p < 3; ++p) {
    pt.law[p] = in[p] != 0.0 ? kLawGeneral : kLawIso;
    pt.mu[p] = in[3 + p];
    pt.lambda[p] = in[6 + p];
    for (int k = 0; k < 36; ++k) pt.C[p][k] = in[9 + 36 * p + k];
    phi[p] = in[117 + p];
  }
  const double* F = in + 120;
  general6(F, pt.C[0], 1.0, false, out);
  pk1_voigt<kMaxPhases>(F, phi, pt, 1.0, false, out + 6);
  tangent_eigs<kMaxPhases, true>(phi, pt, kMixVoigt, out + 12, out + 13);
}

void emu_general_batch(long n, const double* in, double* out) {
  for (long i = 0; i < n; ++i) emu_general_case(in + 126 * i, out + 14 * i);
}

// eigenvalue extremes of one symmetric 6 x 6 matrix (row-major)
void emu_jacobi_minmax6(const double* A36, double* lo, double* hi) {
  double A[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) A[i][j] = A36[6 * i + j];
  jacobi_minmax6(A, lo, hi);
}

}  // extern "C"

#ifdef EMU_GENERAL_MAIN
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[126];
  while (std::fread(buf, sizeof(double), 126, f) == 126) in.insert(in.end(), buf, buf + 126);
  std::fclose(f);
  const long n = (long)(in.size() / 126);
  std::vector<double> out(14 * (size_t)n);
  emu_general_batch(n, in.data(), out.data());
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 4;
  const size_t w = std::fwrite(out.data(), sizeof(double), out.size(), g);
  std::fclose(g);
  return w == out.size() ? 0 : 5;
}
#endif
