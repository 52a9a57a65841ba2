// Bluestein tile kernels for lengths with a prime factor above 13 (fg_fft_bluestein.h): the strided (x / y) pass and the z passes,
// on the run-time-plan class kernels' pass loop (smooth_dev_passes) for the padded length M.
#include "fg_fft_bluestein_dev.h"

namespace fg {
namespace fft {

namespace {

// the M-point forward passes twice, the filter between them (the loop stays rolled: one copy of the pass code per kernel)
template <int RMAX>
__device__ __forceinline__ void bluestein_dev_middle(cplx* img, const SmoothPlan& plan, const BluesteinGeom& G, const BluesteinTables& t) {
  const SmoothMap L = G.map();
#pragma nounroll
  for (int rep = 0; rep < 2; ++rep) {
    smooth_dev_passes<-1, RMAX>(img, plan, L, t.w, 1);   // (ends behind a barrier)
    if (rep == 0) {
      bluestein_filter(G, t.filter, threadIdx.x, blockDim.x, img);
      __syncthreads();
    }
  }
}

// THREADS / RMAX classes as for the tile kernels: (256, 16), (256, 32), (1024, 16)
template <int THREADS, int RMAX>
__global__ __launch_bounds__(THREADS) void k_bluestein_strided(BluesteinArgs a, long comp_stride) {
  extern __shared__ __align__(16) double lds[];
  cplx* img = reinterpret_cast<cplx*>(lds);
  a.data += (long)blockIdx.y * comp_stride;
  constexpr int B = THREADS == 256 ? 8 : 4;
  const BluesteinGeom G = bluestein_geom_strided(a.plan);
  bluestein_strided_load<B>(a, G, blockIdx.x, threadIdx.x, THREADS, img);
  __syncthreads();
  bluestein_dev_middle<RMAX>(img, a.plan, G, a.t);
  bluestein_strided_store(a, G, blockIdx.x, threadIdx.x, THREADS, img);
}

template <int THREADS, int RMAX>
__global__ __launch_bounds__(THREADS) void k_bluestein_z(BluesteinZArgs a, long comp_stride) {
  extern __shared__ __align__(16) double lds[];
  cplx* img = reinterpret_cast<cplx*>(lds);
  a.data += (long)blockIdx.y * comp_stride;
  constexpr int B = THREADS == 256 ? 8 : 4;
  const BluesteinGeom G = bluestein_geom_z(a.plan);
  const long row0 = (long)blockIdx.x * a.plan.lines;
  bluestein_z_load<B>(a, G, row0, threadIdx.x, THREADS, img);
  __syncthreads();
  if (!a.odd && !a.fwd) {
    bluestein_z_merge(a, G, threadIdx.x, THREADS, img);
    __syncthreads();
  }
  bluestein_dev_middle<RMAX>(img, a.plan, G, a.t);
  bluestein_z_store(a, G, row0, threadIdx.x, THREADS, img);
}

}  // namespace

void launch_bluestein_strided(const BluesteinArgs& a0, int nouter, int ncomp, long cs, hipStream_t s) {
  BluesteinArgs a = a0;
  const int C = a.plan.lines;
  if (C < 2 || (C & (C - 1)) || a.n < 1 || a.plan.n < 2 * a.n - 1) throw std::runtime_error("fft: bad Bluestein plan");
  a.tiles_per_outer = (a.ncols + C - 1) / C;
  const size_t lds = bluestein_geom_strided(a.plan).lds_bytes();
  if (lds > kSmoothLdsMax) throw std::runtime_error("fft: Bluestein image exceeds the LDS");
  static PerDeviceOnce configured;
  if (auto once = configured.first_use()) {
    smooth_configure(&k_bluestein_strided<256, 16>);
    smooth_configure(&k_bluestein_strided<256, 32>);
    smooth_configure(&k_bluestein_strided<1024, 16>);
  }
  const dim3 grid((unsigned)((long)a.tiles_per_outer * nouter), ncomp);
  switch (smooth_class(a.plan)) {
    case 0: hipLaunchKernelGGL((k_bluestein_strided<256, 16>), grid, dim3(256), lds, s, a, cs); break;
    case 1: hipLaunchKernelGGL((k_bluestein_strided<256, 32>), grid, dim3(256), lds, s, a, cs); break;
    default: hipLaunchKernelGGL((k_bluestein_strided<1024, 16>), grid, dim3(1024), lds, s, a, cs); break;
  }
  FG_HIP_CHECK(hipGetLastError());
}

void launch_bluestein_z(const BluesteinZArgs& a, int ncomp, long comp_stride, hipStream_t s) {
  const int lines = a.plan.lines;
  if (lines < 1 || a.n < 1 || a.plan.n < 2 * a.n - 1) throw std::runtime_error("fft: bad Bluestein plan");
  const size_t lds = bluestein_geom_z(a.plan).lds_bytes();
  if (lds > kSmoothLdsMax) throw std::runtime_error("fft: Bluestein image exceeds the LDS");
  static PerDeviceOnce configured;
  if (auto once = configured.first_use()) {
    smooth_configure(&k_bluestein_z<256, 16>);
    smooth_configure(&k_bluestein_z<256, 32>);
    smooth_configure(&k_bluestein_z<1024, 16>);
  }
  const dim3 grid((unsigned)((a.nrows + lines - 1) / lines), ncomp);
  switch (smooth_class(a.plan)) {
    case 0: hipLaunchKernelGGL((k_bluestein_z<256, 16>), grid, dim3(256), lds, s, a, comp_stride); break;
    case 1: hipLaunchKernelGGL((k_bluestein_z<256, 32>), grid, dim3(256), lds, s, a, comp_stride); break;
    default: hipLaunchKernelGGL((k_bluestein_z<1024, 16>), grid, dim3(1024), lds, s, a, comp_stride); break;
  }
  FG_HIP_CHECK(hipGetLastError());
}

}  // namespace fft
}  // namespace fg
