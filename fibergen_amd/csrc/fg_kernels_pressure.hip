// Kernels of the pressure accessor of mode = viscosity (get_raw_field("p")  F:15554-15573): the scalar divergence of a vector
// field with the reference's difference offsets (divVector  F:19983-20003) and the Fourier symbol of poisson_solve
// (F:23454-23500).  Operation order of the reference throughout (this translation unit is compiled without FMA contraction).
#include "fg_kernels.h"

#include "fg_hip_util.h"
#include "fg_kernels_common.h"

namespace fg {

namespace {

// divVector  F:19996-19998: b[k] = (t0[k] - t0[k + _ffd_x[ii]]) chx + (t1[k] - t1[k + _ffd_y[jj]]) chy + (t2[k] - t2[k + _ffd_z[kk]]) chz
// with ch_a = alpha n_a / d_a.  _ffd_a (F:14867-14891) is the offset to the NEXT voxel along a, periodic: the value itself minus
// its forward neighbour, i.e. MINUS the forward difference.  One thread per real of the padded rows; the padding columns
// (k >= nz) are neither read nor written.
__global__ __launch_bounds__(kBlock) void k_div_vector(Grid g, FieldPtrs<3> t, double chx, double chy, double chz, double* b) {
  const long n = g.n;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / g.nzp;
    const int kk = (int)(idx - row * g.nzp);
    if (kk >= g.nz) continue;
    const int ii = (int)(row / g.ny);
    const int jj = (int)(row - (long)ii * g.ny);
    const long fx = (ii == g.nx - 1 ? -(long)(g.nx - 1) : 1L) * g.nyzp;
    const long fy = (jj == g.ny - 1 ? -(long)(g.ny - 1) : 1L) * g.nzp;
    const long fz = kk == g.nz - 1 ? -(long)(g.nz - 1) : 1L;
    b[idx] = (t.p[0][idx] - t.p[0][idx + fx]) * chx + (t.p[1][idx] - t.p[1][idx + fy]) * chy +
             (t.p[2][idx] - t.p[2][idx + fz]) * chz;
  }
}

// poisson_solve  F:23484-23496 on the half spectrum [nx][ny][nzc] (nzf bins a row, the pitch's padding left alone):
//   uc[k] /= c (hax (cos xi0 - 1) + hay (cos xi1 - 1) + haz (cos xi2 - 1));   uc[0] = 0
// cs[a][m] = cos(2 pi m / n_a) from the host's libm.  The reference divides bin 0 by zero and overwrites the result; here the
// bin is set without the division, so no NaN exists at any time.  std::complex /= real divides both parts.
__global__ __launch_bounds__(kBlock) void k_poisson_symbol(Grid g, cplx* uc, PoissonTables tb, double c, double hax, double hay,
                                                           double haz) {
  const long nfreq = (long)g.nx * g.ny * g.nzc;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < nfreq; idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / g.nzc;
    const int kk = (int)(idx - row * g.nzc);
    if (kk >= g.nzf) continue;
    const int ii = (int)(row / g.ny);
    const int jj = (int)(row - (long)ii * g.ny);
    cplx e;
    if (ii == 0 && jj == 0 && kk == 0) {
      e = cmake(0.0, 0.0);
    } else {
      const double d = c * (hax * (tb.cs[0][ii] - 1.0) + hay * (tb.cs[1][jj] - 1.0) + haz * (tb.cs[2][kk] - 1.0));
      const cplx v = uc[idx];
      e = cmake(v.re / d, v.im / d);
    }
    uc[idx] = e;
  }
}

}  // namespace

void launch_div_vector(const Grid& g, const FieldPtrs<3>& t, double alpha, double* b, hipStream_t s) {
  const double chx = alpha * g.nx / g.dx, chy = alpha * g.ny / g.dy, chz = alpha * g.nz / g.dz;   // F:19987-19989
  hipLaunchKernelGGL(k_div_vector, dim3(grid_for(g.n, 1 << 20)), dim3(kBlock), 0, s, g, t, chx, chy, chz, b);
  FG_HIP_CHECK(hipGetLastError());
}

void launch_poisson_symbol(const Grid& g, double* uc, const PoissonTables& tb, hipStream_t s) {
  const double c = 2 * (double)g.nxyz;                                   // F:23463
  const double hax = (double)((long)g.nx * g.nx) / (g.dx * g.dx);        // F:23464-23466
  const double hay = (double)((long)g.ny * g.ny) / (g.dy * g.dy);
  const double haz = (double)((long)g.nz * g.nz) / (g.dz * g.dz);
  const long nfreq = (long)g.nx * g.ny * g.nzc;
  hipLaunchKernelGGL(k_poisson_symbol, dim3(grid_for(nfreq, 1 << 20)), dim3(kBlock), 0, s, g, reinterpret_cast<cplx*>(uc), tb, c,
                     hax, hay, haz);
  FG_HIP_CHECK(hipGetLastError());
}

}  // namespace fg
