// gamma_scheme full_staggered / half_staggered: the doubly fine grid ("dfg", use_dfg F:14894-14897) of the reference in
// coarse form (see fg_kernels.h).  The fine phase image exists only while a phase is uploaded: it is reduced here to the
// four staggered fractions of every coarse voxel, and the iteration reads five per-voxel moduli instead of two.
#include "fg_kernels.h"

#include "fg_hip_util.h"
#include "fg_kernels_common.h"

namespace fg {

namespace {

__device__ __forceinline__ long wrap(long a, long n) { return a < 0 ? a + n : (a >= n ? a - n : a); }

// restrict_from_dfg F:14273-14335 of one component group: 0.125 x the 8 fine cells (2i + si .. 2i + 1 + si, ...), periodic,
// summed in the reference's order
__device__ __forceinline__ double dfg_mean8(const double* f, long fx, long fy, long fz, int i, int j, int k, int si, int sj,
                                            int sk) {
  const long i0 = wrap(2L * i + si, fx) * fy * fz, i1 = wrap(2L * i + 1 + si, fx) * fy * fz;
  const long j0 = wrap(2L * j + sj, fy) * fz, j1 = wrap(2L * j + 1 + sj, fy) * fz;
  const long k0 = wrap(2L * k + sk, fz), k1 = wrap(2L * k + 1 + sk, fz);
  return 0.125 * (f[i0 + j0 + k0] + f[i1 + j0 + k0] + f[i0 + j1 + k0] + f[i1 + j1 + k0] + f[i0 + j0 + k1] + f[i1 + j0 + k1] +
                  f[i0 + j1 + k1] + f[i1 + j1 + k1]);
}

__global__ __launch_bounds__(kBlock) void k_dfg_fractions_fine(Grid g, const double* fine, double* phi_n, FieldPtrs<3> phi_s) {
  const long fx = 2L * g.nx, fy = 2L * g.ny, fz = 2L * g.nz;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < g.nxyz; v += (long)gridDim.x * blockDim.x) {
    const int k = (int)(v % g.nz);
    const long t = v / g.nz;
    const int j = (int)(t % g.ny), i = (int)(t / g.ny);
    const long o = (long)i * g.nyzp + (long)j * g.nzp + k;
    // shifts of restrict_from_dfg: normal (0,0,0), 23 (0,-1,-1), 13 (-1,0,-1), 12 (-1,-1,0)
    phi_n[o] = dfg_mean8(fine, fx, fy, fz, i, j, k, 0, 0, 0);
    phi_s.p[0][o] = dfg_mean8(fine, fx, fy, fz, i, j, k, 0, -1, -1);
    phi_s.p[1][o] = dfg_mean8(fine, fx, fy, fz, i, j, k, -1, 0, -1);
    phi_s.p[2][o] = dfg_mean8(fine, fx, fy, fz, i, j, k, -1, -1, 0);
  }
}

// prolongate (copy) then restrict: the shifted 8-cell block covers 2 coarse cells along each shifted axis
__global__ __launch_bounds__(kBlock) void k_dfg_fractions_replica(Grid g, const double* phi, FieldPtrs<3> phi_s) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < g.nxyz; v += (long)gridDim.x * blockDim.x) {
    const int k = (int)(v % g.nz);
    const long t = v / g.nz;
    const int j = (int)(t % g.ny), i = (int)(t / g.ny);
    const long xo = (long)i * g.nyzp, xb = (long)(i == 0 ? g.nx - 1 : i - 1) * g.nyzp;
    const long yo = (long)j * g.nzp, yb = (long)(j == 0 ? g.ny - 1 : j - 1) * g.nzp;
    const long ko = k, kb = k == 0 ? g.nz - 1 : k - 1;
    const long o = xo + yo + ko;
    phi_s.p[0][o] = 0.25 * (phi[xo + yb + kb] + phi[xo + yo + kb] + phi[xo + yb + ko] + phi[o]);
    phi_s.p[1][o] = 0.25 * (phi[xb + yo + kb] + phi[xo + yo + kb] + phi[xb + yo + ko] + phi[o]);
    phi_s.p[2][o] = 0.25 * (phi[xb + yb + ko] + phi[xo + yb + ko] + phi[xb + yo + ko] + phi[o]);
  }
}

// the Voigt rule's threshold (F:12736) applied to each group's fractions, as k_effective_moduli does to the coarse ones
__global__ __launch_bounds__(kBlock) void k_dfg_moduli(long n2, long n, PhaseTable pt, const double* phi, const double* phis,
                                                       FieldPtrs<5> mod) {
  const double threshold = 10 * 2.220446049250313e-16;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = make_double2(0.0, 0.0);
    for (int p = 0; p < pt.n; ++p) {
      const double2 f = ld2(phi + (long)p * n, 2 * i);
      if (f.x > threshold) { m[0].x += 2 * f.x * pt.mu[p]; m[1].x += f.x * pt.lambda[p]; }
      if (f.y > threshold) { m[0].y += 2 * f.y * pt.mu[p]; m[1].y += f.y * pt.lambda[p]; }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double2 h = ld2(phis + (3L * p + c) * n, 2 * i);
        if (h.x > threshold) m[2 + c].x += 2 * h.x * pt.mu[p];
        if (h.y > threshold) m[2 + c].y += 2 * h.y * pt.mu[p];
      }
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) st2(mod.p[q], 2 * i, m[q]);
  }
}

// MODE 0: tau written; 1: per-block sums of P; 2: per-block sums of 1/2 P:eps (component 0)
__device__ __forceinline__ void dfg_voxel(const double* e, const double* m, double alpha, double beta, double gamma, double* P) {
  const double tr = e[0] + e[1] + e[2];
  const double b = alpha * m[1] + gamma;
#pragma unroll
  for (int c = 0; c < 3; ++c) P[c] = e[c] * (alpha * m[0] + beta) + b * tr;
#pragma unroll
  for (int c = 3; c < 6; ++c) P[c] = e[c] * (alpha * m[c - 1] + beta);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_dfg_stress(Grid g, double alpha, double beta, double gamma, FieldPtrs<6> eps,
                                                       FieldPtrs<5> mod, FieldPtrs<6> tau, double* partial) {
  __shared__ double smem[4 * 6];
  const long npairs = (long)g.nx * g.ny * g.nzc;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (long pidx = (long)blockIdx.x * blockDim.x + threadIdx.x; pidx < npairs; pidx += (long)gridDim.x * blockDim.x) {
    const PairPos p = pair_pos(pidx, g);
    if (p.k >= g.nz) continue;  // padding pair
    const bool second = p.k + 1 < g.nz;
    double2 e2[6], m2[5];
#pragma unroll
    for (int c = 0; c < 6; ++c) e2[c] = ld2(eps.p[c], p.off);
#pragma unroll
    for (int q = 0; q < 5; ++q) m2[q] = ld2(mod.p[q], p.off);
    double e[6], m[5], P0[6], P1[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) e[c] = e2[c].x;
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] = m2[q].x;
    dfg_voxel(e, m, alpha, beta, gamma, P0);
    double w = 0.0;
    if (MODE == 2) w = 0.5 * (P0[0] * e[0] + P0[1] * e[1] + P0[2] * e[2] + 2 * (P0[3] * e[3] + P0[4] * e[4] + P0[5] * e[5]));
    if (second) {
#pragma unroll
      for (int c = 0; c < 6; ++c) e[c] = e2[c].y;
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] = m2[q].y;
      dfg_voxel(e, m, alpha, beta, gamma, P1);
      if (MODE == 2) w += 0.5 * (P1[0] * e[0] + P1[1] * e[1] + P1[2] * e[2] + 2 * (P1[3] * e[3] + P1[4] * e[4] + P1[5] * e[5]));
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) P1[c] = 0.0;
    }
    if (MODE == 2) {
      acc[0] += w;
    } else if (MODE == 1) {
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += P0[c] + P1[c];
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) st2(tau.p[c], p.off, make_double2(P0[c], P1[c]));
    }
  }
  if (MODE) {
    block_reduce<6>(acc, smem, OpSum());
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < 6; ++c) partial[(long)blockIdx.x * 6 + c] = acc[c];
    }
  }
}

unsigned blocks_for(long items) {
  long nb = (items + kBlock - 1) / kBlock;
  if (nb > 65536) nb = 65536;
  return (unsigned)(nb < 1 ? 1 : nb);
}

}  // namespace

void launch_dfg_fractions_fine(const Grid& g, const double* fine, double* phi_n, const FieldPtrs<3>& phi_s, hipStream_t s) {
  hipLaunchKernelGGL(k_dfg_fractions_fine, dim3(blocks_for(g.nxyz)), dim3(kBlock), 0, s, g, fine, phi_n, phi_s);
  FG_HIP_CHECK(hipGetLastError());
}

void launch_dfg_fractions_replica(const Grid& g, const double* phi, const FieldPtrs<3>& phi_s, hipStream_t s) {
  hipLaunchKernelGGL(k_dfg_fractions_replica, dim3(blocks_for(g.nxyz)), dim3(kBlock), 0, s, g, phi, phi_s);
  FG_HIP_CHECK(hipGetLastError());
}

void launch_dfg_moduli(const Grid& g, const PhaseTable& pt, const double* phi, const double* phis, const FieldPtrs<5>& mod,
                       hipStream_t s) {
  const long n2 = g.n / 2;
  hipLaunchKernelGGL(k_dfg_moduli, dim3(blocks_for(n2)), dim3(kBlock), 0, s, n2, g.n, pt, phi, phis, mod);
  FG_HIP_CHECK(hipGetLastError());
}

void launch_dfg_stress(int mode, const Grid& g, const StressParams& sp, const FieldPtrs<6>& eps, const FieldPtrs<5>& mod,
                       const FieldPtrs<6>& tau, double* partial, double* out6, hipStream_t s) {
  const double beta = -sp.alpha * 2 * sp.mu_0, gamma = -sp.alpha * sp.lambda_0;
  const long npairs = (long)g.nx * g.ny * g.nzc;
  if (mode == 0) {
    hipLaunchKernelGGL(k_dfg_stress<0>, dim3(blocks_for(npairs)), dim3(kBlock), 0, s, g, sp.alpha, beta, gamma, eps, mod, tau,
                       (double*)nullptr);
    FG_HIP_CHECK(hipGetLastError());
    return;
  }
  const int nb = reduce_blocks(g);
  if (mode == 1)
    hipLaunchKernelGGL(k_dfg_stress<1>, dim3(nb), dim3(kBlock), 0, s, g, sp.alpha, beta, gamma, eps, mod, tau, partial);
  else
    hipLaunchKernelGGL(k_dfg_stress<2>, dim3(nb), dim3(kBlock), 0, s, g, sp.alpha, beta, gamma, eps, mod, tau, partial);
  FG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_fold<OpSum>, dim3(1), dim3(kBlock), 0, s, partial, nb, 6, 0.0, out6);
  FG_HIP_CHECK(hipGetLastError());
}

}  // namespace fg
