// method "polarization" (Eyre & Milton 1999; runPolarization F:21808-21851, polarizationScheme F:20536-20554): the streaming
// kernels of one pass whose state is the polarisation field P (six components).  Per-voxel arithmetic: fg_stage_math.h
// (polarize_voxel), shared with the host emulation in tests.
#include "fg_kernels.h"

#include "fg_hip_util.h"
#include "fg_kernels_common.h"

namespace fg {

namespace {

// calcPolarization  F:18044-18131: out = Q(P) (INV = false) or the strain R = (C + C0)^-1 P (INV = true; out may be the
// input field: every thread reads its pair before it writes it).  One thread per z pair as k_stress; reads 6 + nph doubles
// per voxel and writes 6.  INV = false also leaves per block the six sums of Q (P00 = <Q>, F:20547) and the number of voxels
// that took the 6 x 6 solve (fg_get_counter "polarization_generic_voxels"): rows of 7 partials, folded in a fixed order.
template <int NPH, bool INV>
__global__ __launch_bounds__(kBlock) void k_polarize(Grid g, PhaseTable pt, double mu_0, FieldPtrs<6> in,
                                                     FieldPtrs<kMaxPhases> phi, FieldPtrs<6> out, double* partial) {
  __shared__ double smem[4 * 7];
  const long npairs = (long)g.nx * g.ny * g.nzc;
  double acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long pidx = (long)blockIdx.x * blockDim.x + threadIdx.x; pidx < npairs; pidx += (long)gridDim.x * blockDim.x) {
    const PairPos p = pair_pos(pidx, g);
    if (p.k >= g.nz) continue;  // padding pair
    const bool second = p.k + 1 < g.nz;
    double2 e[6], f[NPH];
#pragma unroll
    for (int c = 0; c < 6; ++c) e[c] = ld2(in.p[c], p.off);
#pragma unroll
    for (int q = 0; q < NPH; ++q) f[q] = q < pt.n ? ld2(phi.p[q], p.off) : make_double2(0.0, 0.0);
    double2 o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = make_double2(0.0, 0.0);
    double ngen = 0.0;
    // the two voxels of the pair one after the other through ONE copy of the per-voxel code (two inlined copies of the 6 x 7
    // elimination do not fit the register file)
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
      if (h == 1 && !second) break;
      double F[6], ph[NPH], Q[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) F[c] = h ? e[c].y : e[c].x;
#pragma unroll
      for (int q = 0; q < NPH; ++q) ph[q] = h ? f[q].y : f[q].x;
      ngen += polarize_voxel<NPH>(F, ph, pt, mu_0, INV, Q) ? 1.0 : 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        if (h) o[c].y = Q[c];
        else o[c].x = Q[c];
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) st2(out.p[c], p.off, o[c]);
    if (!INV) {
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += o[c].x + o[c].y;
      acc[6] += ngen;
    }
  }
  if (!INV) {
    block_reduce<7>(acc, smem, OpSum());
    if (threadIdx.x == 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) partial[(long)blockIdx.x * 7 + c] = acc[c];
    }
  }
}

// Staggered scheme, tail of a pass:  P = Q + (P0 + sym grad_h u)  with u = -4 mu_0 G0 div_h Q from the transform chain --
// epsOperatorStaggered F:18614-18692 as k_eps_norm evaluates it, plus the stored Q; sym grad_h of a periodic u has zero mean,
// so <P> = <Q> + P0 = P00 + P0 (F:20553).  Written over the old P, with the six sums of squares of the new one (component_norm
// F:10088-10138) for the stop rule.  Reads 3 (+ neighbours from L2) + 6 doubles per voxel, writes 6.
__global__ __launch_bounds__(kBlock) void k_polar_back(Grid g, FieldPtrs<3> u, FieldPtrs<6> Q, FieldPtrs<6> P, Vec6 P0,
                                                       double* partial, Sweep ry) {
  __shared__ double smem[4 * 6];
  const double hx = g.hx, hy = g.hy, hz = g.hz;
  const long npairs = (long)g.nx * g.ny * g.nzc;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  const BlockRun run = block_run((npairs + kBlock - 1) / kBlock);
  for (long it = 0; it < run.count; ++it) {
    const long pidx = (run.first + it * run.stride) * kBlock + threadIdx.x;
    if (pidx >= npairs) continue;
    const PairPos p = pair_pos_tiled(pidx, g, ry);
    if (p.k >= g.nz) continue;
    const bool second = p.k + 1 < g.nz;
    const long xf = (p.i + 1 == g.nx ? -(long)(g.nx - 1) : 1L) * g.nyzp;
    const long xb = (p.i == 0 ? (long)(g.nx - 1) : -1L) * g.nyzp;
    const long yf = (p.j + 1 == g.ny ? -(long)(g.ny - 1) : 1L) * g.nzp;
    const long yb = (p.j == 0 ? (long)(g.ny - 1) : -1L) * g.nzp;
    const long rowoff = p.off - p.k;
    const int kb = p.k == 0 ? g.nz - 1 : p.k - 1;
    const int kf2 = (p.k + 2 >= g.nz) ? p.k + 2 - g.nz : p.k + 2;

    const double2 u0 = ld2(u.p[0], p.off), u1 = ld2(u.p[1], p.off), u2 = ld2(u.p[2], p.off);
    const double2 u0xf = ld2(u.p[0], p.off + xf), u1xb = ld2(u.p[1], p.off + xb), u2xb = ld2(u.p[2], p.off + xb);
    const double2 u0yb = ld2(u.p[0], p.off + yb), u1yf = ld2(u.p[1], p.off + yf), u2yb = ld2(u.p[2], p.off + yb);
    const double u0zb = u.p[0][rowoff + kb], u1zb = u.p[1][rowoff + kb];
    const double u2zf2 = u.p[2][rowoff + kf2];
    const double u2zf1 = second ? u2.y : u.p[2][rowoff];

    double2 e[6];
    e[3].x = P0.v[3] + 0.5 * ((u2.x - u2yb.x) * hy + (u1.x - u1zb) * hz);
    e[4].x = P0.v[4] + 0.5 * ((u2.x - u2xb.x) * hx + (u0.x - u0zb) * hz);
    e[5].x = P0.v[5] + 0.5 * ((u1.x - u1xb.x) * hx + (u0.x - u0yb.x) * hy);
    e[0].x = P0.v[0] + (u0xf.x - u0.x) * hx;
    e[1].x = P0.v[1] + (u1yf.x - u1.x) * hy;
    e[2].x = P0.v[2] + (u2zf1 - u2.x) * hz;
    e[3].y = P0.v[3] + 0.5 * ((u2.y - u2yb.y) * hy + (u1.y - u1.x) * hz);
    e[4].y = P0.v[4] + 0.5 * ((u2.y - u2xb.y) * hx + (u0.y - u0.x) * hz);
    e[5].y = P0.v[5] + 0.5 * ((u1.y - u1xb.y) * hx + (u0.y - u0yb.y) * hy);
    e[0].y = P0.v[0] + (u0xf.y - u0.y) * hx;
    e[1].y = P0.v[1] + (u1yf.y - u1.y) * hy;
    e[2].y = P0.v[2] + (u2zf2 - u2.y) * hz;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double2 q = ld2(Q.p[c], p.off);
      e[c].x = q.x + e[c].x;
      e[c].y = second ? q.y + e[c].y : 0.0;
      acc[c] += e[c].x * e[c].x + e[c].y * e[c].y;
      st2(P.p[c], p.off, e[c]);
    }
  }
  block_reduce<6>(acc, smem, OpSum());
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) partial[(long)blockIdx.x * 6 + c] = acc[c];
  }
}

}  // namespace

void launch_polarize(const Grid& g, const PhaseTable& pt, double mu_0, bool inv, const FieldPtrs<6>& in,
                     const FieldPtrs<kMaxPhases>& phi, const FieldPtrs<6>& out, double* partial, double* out7, hipStream_t s) {
  const int nb = reduce_blocks(g);
  // one instantiation per phase count (as the reference-material scan has): the unrolled phase loop of an instantiation wider
  // than the problem costs registers the elimination needs
#define FG_LAUNCH(NPH, INV) \
  hipLaunchKernelGGL((k_polarize<NPH, INV>), dim3(nb), dim3(kBlock), 0, s, g, pt, mu_0, in, phi, out, partial)
#define FG_LAUNCH_N(NPH)          \
  do {                            \
    if (inv) FG_LAUNCH(NPH, true); \
    else FG_LAUNCH(NPH, false);   \
  } while (0)
  switch (pt.n <= 2 ? 2 : pt.n) {
    case 2: FG_LAUNCH_N(2); break;
    case 3: FG_LAUNCH_N(3); break;
    case 4: FG_LAUNCH_N(4); break;
    case 5: FG_LAUNCH_N(5); break;
    case 6: FG_LAUNCH_N(6); break;
    case 7: FG_LAUNCH_N(7); break;
    default: FG_LAUNCH_N(kMaxPhases); break;
  }
#undef FG_LAUNCH_N
#undef FG_LAUNCH
  FG_HIP_CHECK(hipGetLastError());
  if (!inv) {
    hipLaunchKernelGGL(k_fold<OpSum>, dim3(1), dim3(kBlock), 0, s, partial, nb, 7, 0.0, out7);
    FG_HIP_CHECK(hipGetLastError());
  }
}

void launch_polar_back(const Grid& g, const FieldPtrs<3>& u, const FieldPtrs<6>& Q, const FieldPtrs<6>& P, const Vec6& P0,
                       double* partial, double* sumsq6, hipStream_t s) {
  const int nb = sweep_blocks((long)g.nx * g.ny * g.nzc);
  hipLaunchKernelGGL(k_polar_back, dim3(nb), dim3(kBlock), 0, s, g, u, Q, P, P0, partial, chunk_rows(g));
  FG_HIP_CHECK(hipGetLastError());
  fold_sum(partial, nb, 6, sumsq6, s);
  FG_HIP_CHECK(hipGetLastError());
}

}  // namespace fg
