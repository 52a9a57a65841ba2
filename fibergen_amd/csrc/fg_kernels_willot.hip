// gamma_scheme willot: Willot's rotated Green operator in Fourier space (GammaOperatorFourierWillotR F:19083-19299), the
// per-frequency arithmetic of fg_willot_math.h on the six complex components in place.
#include "fg_kernels.h"

#include "fg_hip_util.h"
#include "fg_kernels_common.h"
#include "fg_willot_math.h"

namespace fg {

namespace {

// One thread per frequency of [nx][ny][nzc]; the padded columns of a row are skipped (never read, never written).  Reads the
// six tau_hat and writes the six eta_hat: 192 B per frequency, the traffic of k_gamma_collocated.  No trigonometry here: the
// three table entries per axis come from the host (willot_axis_table).  The zero frequency is set to E (F:19296-19298; the
// caller adds the BC-projector term), plus mcoef * mean6[c] where the caller keeps a mean on the device (Delta operator:
// adj = E - 2 alpha m <tau>, F:20405).
template <bool INF_LAMBDA>
__global__ __launch_bounds__(kBlock) void k_gamma_willot(Grid g, FieldPtrs<6> th, WillotTables wt, WillotCoef cf, Vec6 E,
                                                         const double* mean6, double mcoef) {
  const long nfreq = (long)g.nx * g.ny * g.nzc;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < nfreq; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / g.nzc;
    const int kk = (int)(idx - row * g.nzc);
    if (kk >= g.nzf) continue;  // row padding
    const int ii = (int)(row / g.ny);
    const int jj = (int)(row - (long)ii * g.ny);
    cplx ey[6];
    if (ii == 0 && jj == 0 && kk == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) ey[c] = cmake(mean6 ? E.v[c] + mcoef * mean6[c] : E.v[c], 0.0);
    } else {
      cplx t[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) t[c] = reinterpret_cast<const cplx*>(th.p[c])[idx];
      const double ta[3] = {wt.t[0][ii], wt.t[1][jj], wt.t[2][kk]};
      const cplx e012 = cmul(cmul(wt.e[0][ii], wt.e[1][jj]), wt.e[2][kk]);   // F:19149
      willot_point<INF_LAMBDA>(ta, e012, cf, t, ey);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) reinterpret_cast<cplx*>(th.p[c])[idx] = ey[c];
  }
}

}  // namespace

void launch_gamma_willot(const Grid& g, const FieldPtrs<6>& th, const WillotTables& wt, double mu_0, double lambda_0,
                         double alpha, double beta, const Vec6& E, const double* mean6, double mcoef, hipStream_t s) {
  const long nfreq = (long)g.nx * g.ny * g.nzc;
  const int nb = grid_for(nfreq, 1 << 20);   // as launch_gamma_collocated
  const bool inf = std::isinf(lambda_0);
  const WillotCoef cf = willot_coef(mu_0, lambda_0, inf, alpha, beta);
  if (inf)
    hipLaunchKernelGGL(k_gamma_willot<true>, dim3(nb), dim3(kBlock), 0, s, g, th, wt, cf, E, mean6, mcoef);
  else
    hipLaunchKernelGGL(k_gamma_willot<false>, dim3(nb), dim3(kBlock), 0, s, g, th, wt, cf, E, mean6, mcoef);
  FG_HIP_CHECK(hipGetLastError());
}

}  // namespace fg
