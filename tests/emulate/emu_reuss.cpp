// Host build of the Reuss rule's arithmetic of fibergen_amd/csrc/fg_stage_math.h for tests/test_reuss_emulation.py:
// stress_voxel and tangent_eigs with kMixReuss (and with kMixVoigt, for the pure voxels' bits).
// One case = nph <= 4 phases: in[21] = nph, mu[4], lambda[4], phi[4], F[6], mu_0, lambda_0;
//                            out[20] = stress_voxel reuss [6], emin, emax of the Reuss tangent, stress_voxel voigt [6],
//                                      stress_voxel reuss with C0 = 0 [6].
// Built as a shared library (ctypes) and, with -DEMU_REUSS_MAIN, as a stand-alone program `emu_reuss in out` on files of raw
// doubles.
#include <cstdio>
#include <vector>

#include "../../fibergen_amd/csrc/fg_stage_math.h"

using namespace fg;

extern "C" {

void emu_reuss_case(const double* in, double* out) {
  StressParams sp;
  sp.pt.n = (int)in[0];
  for (int p = 0; p < kMaxPhases; ++p) {
    sp.pt.law[p] = kLawIso;
    sp.pt.mu[p] = sp.pt.lambda[p] = 0.0;
    for (int k = 0; k < 36; ++k) sp.pt.C[p][k] = 0.0;
  }
  double phi[kMaxPhases] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = 0; p < 4; ++p) {
    sp.pt.mu[p] = in[1 + p];
    sp.pt.lambda[p] = in[5 + p];
    phi[p] = in[9 + p];
  }
  const double* F = in + 13;
  const double normal[3] = {0, 0, 0};
  sp.mu_0 = in[19];
  sp.lambda_0 = in[20];
  sp.alpha = 1.0;
  sp.eps_g = sp.eps_a = 0.0;
  sp.mixing = kMixReuss;
  stress_voxel<kMaxPhases>(F, phi, normal, sp, out);
  tangent_eigs<kMaxPhases>(phi, sp.pt, kMixReuss, out + 6, out + 7);
  sp.mixing = kMixVoigt;
  stress_voxel<kMaxPhases>(F, phi, normal, sp, out + 8);
  sp.mixing = kMixReuss;
  sp.mu_0 = sp.lambda_0 = 0.0;
  if (sp.pt.n <= 2) stress_voxel<2>(F, phi, normal, sp, out + 14);   // the two-phase instantiation of the kernels
  else stress_voxel<kMaxPhases>(F, phi, normal, sp, out + 14);
}

void emu_reuss_batch(long n, const double* in, double* out) {
  for (long i = 0; i < n; ++i) emu_reuss_case(in + 21 * i, out + 20 * i);
}

}  // extern "C"

#ifdef EMU_REUSS_MAIN
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[21];
  while (std::fread(buf, sizeof(double), 21, f) == 21) in.insert(in.end(), buf, buf + 21);
  std::fclose(f);
  const long n = (long)(in.size() / 21);
  std::vector<double> out(20 * (size_t)n);
  emu_reuss_batch(n, in.data(), out.data());
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 4;
  const size_t w = std::fwrite(out.data(), sizeof(double), out.size(), g);
  std::fclose(g);
  return w == out.size() ? 0 : 5;
}
#endif
