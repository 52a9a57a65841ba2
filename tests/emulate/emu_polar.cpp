// Host build of the per-voxel arithmetic of method polarization (fibergen_amd/csrc/fg_stage_math.h: polarize_iso,
// polarize_generic, polarize_voxel) for tests/test_polarization_emulation.py.
// One case = three phases: in[127] = law[3], mu[3], lambda[3], C[3][36], phi[3], F[6], mu_0;
//                         out[25] = polarize_voxel forward [6], inverse [6], took the 6 x 6 solve [1],
//                                   polarize_generic forward [6], inverse [6]   (the NPH = kMaxPhases instantiation).
// emu_polar2_*: the NPH = 2 instantiation every two-phase run takes, on phases 0 and 1 of the same record with the fractions
// (phi_0, phi_1) as given: out[13] = polarize_voxel forward [6], inverse [6], took the 6 x 6 solve [1].
// Built as a shared library (ctypes).
#include "../../fibergen_amd/csrc/fg_stage_math.h"

using namespace fg;

extern "C" {

void emu_polar_case(const double* in, double* out) {
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
  const double mu_0 = in[126];
  const bool generic = polarize_voxel<kMaxPhases>(F, phi, pt, mu_0, false, out);
  polarize_voxel<kMaxPhases>(F, phi, pt, mu_0, true, out + 6);
  out[12] = generic ? 1.0 : 0.0;
  polarize_generic<kMaxPhases>(F, phi, pt, mu_0, false, out + 13);
  polarize_generic<kMaxPhases>(F, phi, pt, mu_0, true, out + 19);
}

void emu_polar_batch(long n, const double* in, double* out) {
  for (long i = 0; i < n; ++i) emu_polar_case(in + 127 * i, out + 25 * i);
}

void emu_polar2_case(const double* in, double* out) {
  PhaseTable pt;
  pt.n = 2;
  for (int p = 0; p < kMaxPhases; ++p) {
    pt.law[p] = kLawIso;
    pt.mu[p] = pt.lambda[p] = 0.0;
    for (int k = 0; k < 36; ++k) pt.C[p][k] = 0.0;
  }
  double phi[2];
  for (int p = 0; p < 2; ++p) {
    pt.law[p] = in[p] != 0.0 ? kLawGeneral : kLawIso;
    pt.mu[p] = in[3 + p];
    pt.lambda[p] = in[6 + p];
    for (int k = 0; k < 36; ++k) pt.C[p][k] = in[9 + 36 * p + k];
    phi[p] = in[117 + p];
  }
  const double* F = in + 120;
  const double mu_0 = in[126];
  const bool generic = polarize_voxel<2>(F, phi, pt, mu_0, false, out);
  polarize_voxel<2>(F, phi, pt, mu_0, true, out + 6);
  out[12] = generic ? 1.0 : 0.0;
}

void emu_polar2_batch(long n, const double* in, double* out) {
  for (long i = 0; i < n; ++i) emu_polar2_case(in + 127 * i, out + 13 * i);
}

}  // extern "C"

// emu_polarn_*: the NPH = 4 .. 7 instantiations (launch_polarize has one kernel per phase count) on nph phases:
// in[40 nph + 7] = law[nph], mu[nph], lambda[nph], C[nph][36], phi[nph], F[6], mu_0; out[13] as emu_polar2_case.
template <int NPH>
static void polarn_case(const double* in, double* out) {
  PhaseTable pt;
  pt.n = NPH;
  for (int p = 0; p < kMaxPhases; ++p) {
    pt.law[p] = kLawIso;
    pt.mu[p] = pt.lambda[p] = 0.0;
    for (int k = 0; k < 36; ++k) pt.C[p][k] = 0.0;
  }
  double phi[NPH];
  for (int p = 0; p < NPH; ++p) {
    pt.law[p] = in[p] != 0.0 ? kLawGeneral : kLawIso;
    pt.mu[p] = in[NPH + p];
    pt.lambda[p] = in[2 * NPH + p];
    for (int k = 0; k < 36; ++k) pt.C[p][k] = in[3 * NPH + 36 * p + k];
    phi[p] = in[39 * NPH + p];
  }
  const double* F = in + 40 * NPH;
  const double mu_0 = in[40 * NPH + 6];
  const bool generic = polarize_voxel<NPH>(F, phi, pt, mu_0, false, out);
  polarize_voxel<NPH>(F, phi, pt, mu_0, true, out + 6);
  out[12] = generic ? 1.0 : 0.0;
}

extern "C" int emu_polarn_batch(int nph, long n, const double* in, double* out) {
  const long stride = 40 * nph + 7;
  for (long i = 0; i < n; ++i) {
    switch (nph) {
      case 4: polarn_case<4>(in + stride * i, out + 13 * i); break;
      case 5: polarn_case<5>(in + stride * i, out + 13 * i); break;
      case 6: polarn_case<6>(in + stride * i, out + 13 * i); break;
      case 7: polarn_case<7>(in + stride * i, out + 13 * i); break;
      default: return 1;
    }
  }
  return 0;
}
