// C shim around the measurement pieces of fibergen_amd/csrc/fg_hostmath.h for tests/test_hostmath_measure.py
#include <cstring>

#include "../../fibergen_amd/csrc/fg_hostmath.h"

using namespace fg::hostmath;

namespace {
Mat6 mat(const double* m36) {
  Mat6 m;
  std::memcpy(m.a, m36, sizeof(m.a));
  return m;
}
}  // namespace

extern "C" {

double emu_bc_error_value(const double* P36, const double* Q36, double bc_tol, const double* Emean, const double* Smean,
                          const double* E_cur, const double* S_cur) {
  return bc_error_value(mat(P36), mat(Q36), bc_tol, Emean, Smean, E_cur, S_cur);
}

// 0: compatible, 1: the stress condition was refused, 2: the strain condition, -1: another text
int emu_check_bc_compatible(const double* P36, const double* Q36, const double* Emax, const double* Smax) {
  try {
    check_bc_compatible(mat(P36), mat(Q36), Emax, Smax);
  } catch (const std::runtime_error& e) {
    return !std::strcmp(e.what(), "Incompatible stress boundary condition specified")   ? 1
           : !std::strcmp(e.what(), "Incompatible strain boundary condition specified") ? 2
                                                                                        : -1;
  }
  return 0;
}

double emu_ref_mu0(double lambda_min, double lambda_max, int method, double ref_scale) {
  return ref_mu0(lambda_min, lambda_max, method, ref_scale);
}

int emu_extrapolation_weights(const double* t, int n, double t_new, double* w) { return extrapolation_weights(t, n, t_new, w); }

int emu_check_load_steps(const double* params, int nparams, int first) {
  try {
    check_load_steps(params, nparams, first);
  } catch (const std::runtime_error& e) {
    return !std::strcmp(e.what(), "invalid load steps") ? 1 : -1;
  }
  return 0;
}

void emu_load_step_values(double t, const double* Emax, const double* Smax, double* E, double* S) {
  load_step_values(t, Emax, Smax, E, S);
}

}  // extern "C"
