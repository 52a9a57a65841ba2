// Hand-written 3-D r2c/c2r FFT for gfx950 (no hipFFT/rocFFT).
//
// Three batched 1-D passes per transform, each in place:
//   z : rows of nz reals <-> nzc complex (packed-real trick, lanes along z => coalesced 16 B/lane)
//   y : lines nzc complex apart, tiles of C adjacent kz columns (C*16 B contiguous segments)
//   x : lines ny*nzc apart, tiles of C adjacent (ky,kz) columns
// Butterflies live in registers (8 points/thread), exchanges go through padded LDS.
// Which kernels run an axis -- power of two, p * 2^k sub-lines, tile plans, Bluestein, O(n^2) sums through a scratch
// component -- is the route of fg_fft_route.h, chosen once per axis; every entry point below is a switch on its family.
#include "fg_fft.h"

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "fg_fft_kernels.h"
#include "fg_fft_plane.h"
#include "fg_fft_bluestein_dev.h"
#include "fg_fft_smooth_dev.h"
#include "fg_fft_tables.h"
#include "fg_hip_util.h"

namespace fg {

using namespace fft;

namespace {

// Kernels whose lines never span two waves (z passes: T threads per line, T divides 64) exchange through LDS inside
// one wave only: the LDS queue of a wave is in order, so a compiler-level fence replaces the workgroup barrier and
// the waves of a workgroup drift freely (loads of one overlap the butterflies of another).
template <class K>
struct WaveLocal {
  static constexpr bool value = false;
};
template <int M, int LINES, bool MIRROR, int IMAGES>
struct WaveLocal<R2CKernel<M, LINES, MIRROR, IMAGES>> {
  static constexpr bool value = (M / 8) <= 64 && 64 % (M / 8) == 0;
};
template <int M, int LINES, bool MIRROR, int IMAGES>
struct WaveLocal<C2RKernel<M, LINES, MIRROR, IMAGES>> {
  static constexpr bool value = (M / 8) <= 64 && 64 % (M / 8) == 0;
};

template <class K, class Args, int PH>
struct DevicePhases {
  __device__ __forceinline__ static void run(typename K::Regs& r, int block, int tid, double* lds, const Args& a) {
    K::template phase<PH>(r, block, tid, lds, a);
    if constexpr (PH + 1 < K::NPHASE) {
      if constexpr (WaveLocal<K>::value) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      } else {
        __syncthreads();
      }
      DevicePhases<K, Args, PH + 1>::run(r, block, tid, lds, a);
    }
  }
};

template <class K>
__global__ __launch_bounds__(K::THREADS) void k_strided(StridedArgs a, long comp_stride) {
  extern __shared__ __align__(16) double lds[];
  a.data += (long)blockIdx.y * comp_stride;
  if (a.out) a.out += (long)blockIdx.y * a.out_cs;
  typename K::Regs r;
  int b = blockIdx.x;
  if (a.xcd_order && gridDim.x % 8 == 0) b = (b % 8) * (gridDim.x / 8) + b / 8;
  DevicePhases<K, StridedArgs, 0>::run(r, b, threadIdx.x, lds, a);
}

template <class K>
__global__ __launch_bounds__(K::THREADS) void k_zpass(ZArgs a, long comp_stride) {
  extern __shared__ __align__(16) double lds[];
  a.data += (long)blockIdx.y * comp_stride;
  typename K::Regs r;
  DevicePhases<K, ZArgs, 0>::run(r, blockIdx.x, threadIdx.x, lds, a);
}

// tools/xfused_probe.hip compiles this file with -DFG_PROBE: cycle stamps (s_memtime) of one wave per sampled
// workgroup at every phase boundary of the fused x pass, to see where a tile's time goes.  Empty in the library.
#ifdef FG_PROBE
#ifndef FG_PROBE_STRIDE
#define FG_PROBE_STRIDE 256
#endif
constexpr int kProbeBlocks = 64, kProbeSlots = 40, kProbeStride = FG_PROBE_STRIDE;
__device__ unsigned long long g_probe[kProbeBlocks][kProbeSlots];
#define FG_PROBE_MARK(ph)                                                                        \
  do {                                                                                           \
    if (tid == FG_PROBE_THREAD && block % kProbeStride == 0 && block / kProbeStride < kProbeBlocks) \
      g_probe[block / kProbeStride][(ph)] = __builtin_readcyclecounter();                        \
  } while (0)
#else
#define FG_PROBE_MARK(ph) do { } while (0)
#endif

// z + y transforms of one plane per workgroup (fg_fft_plane.h); blockIdx.y = component
template <class K, int PH>
struct DevicePhasesP {
  __device__ __forceinline__ static void run(typename K::Regs& r, int block, int tid, double* lds, const PlaneArgs& a) {
    FG_PROBE_MARK(PH);
    K::template phase<PH>(r, block, tid, lds, a);
    if constexpr (PH + 1 == K::NPHASE) FG_PROBE_MARK(PH + 1);
    if constexpr (PH + 1 < K::NPHASE) {
      if constexpr (K::barrier_after(PH) == 2 || K::THREADS <= 64) {
        __syncthreads();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      DevicePhasesP<K, PH + 1>::run(r, block, tid, lds, a);
    }
  }
};
template <class K>
__global__ __launch_bounds__(K::THREADS) void k_plane(PlaneArgs a, long comp_stride) {
  extern __shared__ __align__(16) double lds[];
  a.data += (long)blockIdx.y * comp_stride;
  typename K::Regs r;
  DevicePhasesP<K, 0>::run(r, blockIdx.x, threadIdx.x, lds, a);
}

template <class K, int PH>
struct DevicePhasesX {
  __device__ __forceinline__ static void run(typename K::Regs& r, int block, int tid, double* lds, const XFusedArgs& a) {
    FG_PROBE_MARK(PH);
    K::template phase<PH>(r, block, tid, lds, a);
    if constexpr (PH + 1 < K::NPHASE) {
      if constexpr (K::barrier_after(PH)) __syncthreads();
      DevicePhasesX<K, PH + 1>::run(r, block, tid, lds, a);
    } else {
      FG_PROBE_MARK(PH + 1);
    }
  }
};

template <class K>
__global__ __launch_bounds__(K::THREADS) void k_xfused(XFusedArgs a) {
  extern __shared__ __align__(16) double lds[];
  typename K::Regs r;
  // workgroups are dealt round-robin to the eight XCDs: give every XCD a contiguous run of tiles (512^3: 1.84 -> 1.80 ms,
  // 256^3: 0.200 -> 0.188 ms against neighbouring tiles on different XCDs)
  int b = blockIdx.x;
  if (a.xcd_order && gridDim.x % 8 == 0) b = (b % 8) * (gridDim.x / 8) + b / 8;
  DevicePhasesX<K, 0>::run(r, b, threadIdx.x, lds, a);
}

__global__ void k_dft_strided_generic(const cplx* src, cplx* dst, long ls, long os, int ncols, int nouter, int n,
                                      int dir, double scale, const cplx* w) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)nouter * n * ncols;
  if (idx >= total) return;
  int col = idx % ncols;
  long rest = idx / ncols;
  int k = rest % n;
  int o = rest / n;
  dft_strided_point(src, dst, (long)o * os + col, ls, n, k, dir, scale, w);
}

__global__ void k_r2c_generic(const double* src, double* dst, long nrows, int nz, int nzp, const cplx* w) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int nzc = nz / 2 + 1;
  if (idx >= nrows * nzc) return;
  long row = idx / nzc;
  int k = idx % nzc;
  r2c_point(src + row * nzp, reinterpret_cast<cplx*>(dst + row * nzp), nz, k, w);
}

__global__ void k_c2r_generic(const double* src, double* dst, long nrows, int nz, int nzp, const cplx* w) {
  long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nrows * nz) return;
  long row = idx / nz;
  int m = idx % nz;
  c2r_point(reinterpret_cast<const cplx*>(src + row * nzp), dst + row * nzp, nz, m, w);
}

__global__ void k_scale(double* x, long n, double s) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] *= s;
}

// lengths with factors 2, 3, 5, 7, 11, 13: the Stockham tile kernels live in fg_fft_smooth_yz.hip / fg_fft_smooth_x.hip
// (translation units of their own: their many instances compile beside this file)

// The one-kernel sub-line launchers are reached through a route that promised them (fg_fft_route.h): they test the route's own
// predicate, and what it excludes is an error, never a silent fall-through to another family.
[[noreturn]] void no_launcher(const char* what) {
  throw std::runtime_error(std::string("fft: the route names a sub-line kernel that is not built: ") + what);
}

// f(std::integral_constant<int, P>) for the entry of Ps that equals p; a last entry 0 (the kernels with a run-time p) takes
// every other p.  Each call site names the P its kernels are built for: the unrolled and the run-time forms need not round alike.
template <int... Ps, class F>
void dispatch_p(int p, F&& f) {
  if (!((p == Ps || Ps == 0 ? (f(std::integral_constant<int, Ps>{}), true) : false) || ...)) no_launcher("p");
}
// f(std::integral_constant<int, M>) for the sub-line lengths the one-kernel passes are built for (fft::sub_one_m)
template <class F>
void dispatch_sub_m(int m, F&& f) {
  switch (m) {
#define FG_CASE(M) case M: return f(std::integral_constant<int, M>{});
    FG_CASE(8) FG_CASE(16) FG_CASE(32) FG_CASE(64) FG_CASE(128) FG_CASE(256)
#undef FG_CASE
    default: no_launcher("sub-line length");
  }
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wpass-failed"   // the run-time-p instances keep their loops rolled
// ---------------------------------------------------------------- lengths p * 2^k, p odd <= 25
// N = p M: the line is p interleaved sub-lines x_r[m] = x[p m + r] of the power-of-two length M.  Forward: the M-point
// kernels transform the sub-lines in place (line stride p * ls), Y_r[k] then sits at point p k + r, and one combine
// sweep forms  X[k + M s] = sum_r w_N^{r k} w_p^{r s} Y_r[k]  (out of place, through the scratch component).
// Inverse: the combine sweep first,  Z_r[k] = conj(w_N^{r k}) sum_s X[k + M s] conj(w_p^{r s})  to point p k + r,
// then the M-point inverse kernels on the sub-lines.  3x the traffic of a native pass instead of an O(N^2) DFT.
// (p <= fft::kMaxOddFactor; which lengths take this family: fg_fft_route.h)

// w: e^{-2 pi i j / N}, j < N
template <int DIR, int P>   // P = 0: run-time p (indexed local arrays); 3, 5, 7: unrolled, everything in registers
__global__ __launch_bounds__(256) void k_mixed_combine(const cplx* src, cplx* dst, long ls, long os, int ncols, int nouter,
                                                       int M, int p_rt, double scale, const cplx* w) {
  const int p = P ? P : p_rt;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)nouter * M * ncols;
  if (idx >= total) return;
  const int col = (int)(idx % ncols);
  const long rest = idx / ncols;
  const int k = (int)(rest % M);
  const long base = (rest / M) * os + col;
  const int N = p * M;
  cplx in[P ? P : kMaxOddFactor];
#pragma unroll
  for (int r = 0; r < p; ++r) {
    // forward: Y_r[k] at point p k + r;  inverse: X[k + M r] at its natural point
    const long pt = DIR < 0 ? (long)p * k + r : (long)k + (long)M * r;
    in[r] = src[base + pt * ls];
  }
#pragma unroll
  for (int o = 0; o < p; ++o) {
    cplx acc = cmake(0.0, 0.0);
    // the table index r * step mod N advances by step with one conditional subtraction (no division)
    if (DIR < 0) {   // output s = o:  sum_r w_N^{r (k + M s)} Y_r
      const int step = k + M * o;   // < N
      int wi = 0;
#pragma unroll
      for (int r = 0; r < p; ++r) {
        acc = cadd(acc, cmul(in[r], w[wi]));
        wi += step;
        if (wi >= N) wi -= N;
      }
      dst[base + ((long)k + (long)M * o) * ls] = cscale(scale, acc);
    } else {         // output r = o:  conj(w_N^{r k}) sum_s X_s conj(w_p^{r s})
      const int step = (int)(((long)o * M) % N);
      int wi = 0;
#pragma unroll
      for (int sidx = 0; sidx < p; ++sidx) {
        acc = cadd(acc, cmul(in[sidx], cconj(w[wi])));
        wi += step;
        if (wi >= N) wi -= N;
      }
      acc = cmul(acc, cconj(w[o * k]));   // o k < N
      dst[base + ((long)p * k + o) * ls] = cscale(scale, acc);
    }
  }
}

// The same combine in place: a workgroup owns whole lines (a tile of 8 adjacent columns x all N points), computes every
// output of the tile into LDS, and only after a barrier writes the tile back -- no scratch component, no copy
// (2x instead of 3x the traffic of a native pass).  N * 128 bytes of LDS: used while that fits (N <= 1152).
template <int DIR, int P>
__global__ __launch_bounds__(256) void k_mixed_combine_tile(cplx* data, long ls, long os, int ncols, int tiles_per_outer, int M,
                                                            int p_rt, double scale, const cplx* w) {
  extern __shared__ __align__(16) double lds_raw[];
  cplx* img = reinterpret_cast<cplx*>(lds_raw);   // [N][8]
  const int p = P ? P : p_rt;
  const int N = p * M;
  const int o = blockIdx.x / tiles_per_outer;
  const int col0 = (blockIdx.x % tiles_per_outer) * 8;
  const int t = threadIdx.x & 7;
  const bool valid = col0 + t < ncols;
  const long base = (long)o * os + col0 + t;
  for (int k = (int)(threadIdx.x >> 3); k < M; k += 32) {
    cplx in[P ? P : kMaxOddFactor];
#pragma unroll
    for (int r = 0; r < p; ++r) {
      const long pt = DIR < 0 ? (long)p * k + r : (long)k + (long)M * r;
      in[r] = valid ? data[base + pt * ls] : cmake(0.0, 0.0);
    }
#pragma unroll
    for (int q = 0; q < p; ++q) {
      cplx acc = cmake(0.0, 0.0);
      if (DIR < 0) {
        const int step = k + M * q;
        int idx = 0;
#pragma unroll
        for (int r = 0; r < p; ++r) {
          acc = cadd(acc, cmul(in[r], w[idx]));
          idx += step;
          if (idx >= N) idx -= N;
        }
        img[(k + M * q) * 8 + t] = cscale(scale, acc);
      } else {
        const int step = (int)(((long)q * M) % N);
        int idx = 0;
#pragma unroll
        for (int sidx = 0; sidx < p; ++sidx) {
          acc = cadd(acc, cmul(in[sidx], cconj(w[idx])));
          idx += step;
          if (idx >= N) idx -= N;
        }
        img[(p * k + q) * 8 + t] = cscale(scale, cmul(acc, cconj(w[q * k])));
      }
    }
  }
  __syncthreads();
  if (valid)
    for (int pt = (int)(threadIdx.x >> 3); pt < N; pt += 32) data[base + (long)pt * ls] = img[pt * 8 + t];
}

// One kernel for the whole pass where the tile fits (p = 3, 5, 7, 9; N = p M <= 1024 threads, exchange planes <= 144 KB):
// the workgroup holds an 8-column tile of whole lines, thread (jt, r, t) runs the M-point transform of sub-line r of
// column t with the phase code of the power-of-two kernels (the p * 8 sub-lines are just more LDS columns), and the
// combine step goes through an LDS image of the tile -- one read and one write of the data, like a native pass.
template <int M, int DIR, int PH>
struct MixedPhases {
  __device__ __forceinline__ static void run(cplx* v, int jt, double* lds, const fft::LdsMap& L, int c, const cplx* tw) {
    fft::Line<M>::template phase<DIR, PH>(v, jt, lds, L, c, tw);
    if constexpr (PH + 1 < fft::Line<M>::NPHASE) {
      __syncthreads();
      MixedPhases<M, DIR, PH + 1>::run(v, jt, lds, L, c, tw);
    }
  }
};

template <int M, int P, int DIR>
__global__ __launch_bounds__(M * P) void k_strided_mixed(StridedArgs a, long comp_stride, const cplx* wN) {
  using namespace fft;
  constexpr int T = M / 8, COLS = P * 8, THREADS = T * COLS, PN = M + M / 8, N = P * M;
  extern __shared__ __align__(16) double lds[];
  cplx* img = reinterpret_cast<cplx*>(lds);   // [P][M][8], aliases the exchange planes (never live together)
  a.data += (long)blockIdx.y * comp_stride;
  const int tid = threadIdx.x;
  const int cp = tid % COLS, jt = tid / COLS, r = cp / 8, t = cp % 8;
  const int o = blockIdx.x / a.tiles_per_outer;
  const int col = (blockIdx.x % a.tiles_per_outer) * 8 + t;
  const bool valid = col < a.ncols;
  const long base = (long)o * a.os + (valid ? col : 0);
  const LdsMap L = {COLS, 1, PN * COLS};
  cplx v[8];
  auto combine = [&](auto&& get, auto&& put) {   // thread (k, t): p inputs -> p outputs
    for (int k = tid / 8; k < M; k += THREADS / 8) {
      cplx in[P];
#pragma unroll
      for (int q = 0; q < P; ++q) in[q] = get(k, q);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        cplx acc = cmake(0.0, 0.0);
        if (DIR < 0) {   // X[k + M q] = sum_r w_N^{r (k + M q)} Y_r[k]
          const int step = k + M * q;
          int idx = 0;
#pragma unroll
          for (int rr = 0; rr < P; ++rr) {
            acc = cadd(acc, cmul(in[rr], wN[idx]));
            idx += step;
            if (idx >= N) idx -= N;
          }
        } else {         // Z_q[k] = conj(w_N^{q k}) sum_s X[k + M s] conj(w_p^{q s})
          const int step = (q * M) % N;
          int idx = 0;
#pragma unroll
          for (int sidx = 0; sidx < P; ++sidx) {
            acc = cadd(acc, cmul(in[sidx], cconj(wN[idx])));
            idx += step;
            if (idx >= N) idx -= N;
          }
          acc = cmul(acc, cconj(wN[q * k]));
        }
        put(k, q, acc);
      }
    }
  };
  if (DIR < 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      v[q] = valid ? cload_stream(&a.data[base + ((long)P * Line<M>::first_index(jt, q) + r) * a.ls], a.nt) : cmake(0.0, 0.0);
  } else {
    // inverse: combine first, from memory into the image [r][k][t]
    combine([&](int k, int q) { return valid ? cload_stream(&a.data[base + ((long)k + (long)M * q) * a.ls], a.nt) : cmake(0.0, 0.0); },
            [&](int k, int q, cplx z) { img[((long)q * M + k) * 8 + t] = z; });
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = img[((long)r * M + Line<M>::first_index(jt, q)) * 8 + t];
    __syncthreads();   // the image is overwritten by the exchange planes from here on
  }
  // the M-point transform of this thread's sub-line (barrier between phases, as in k_strided)
  MixedPhases<M, DIR, 0>::run(v, jt, lds, L, cp, a.tw);
  if (DIR < 0) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) img[((long)r * M + Line<M>::last_index(jt, q)) * 8 + t] = v[q];
    __syncthreads();
    combine([&](int k, int q) { return img[((long)q * M + k) * 8 + t]; },
            [&](int k, int q, cplx z) {
              if (valid) cstore_stream(&a.data[base + ((long)k + (long)M * q) * a.ls], cscale(a.scale, z), a.nt);
            });
  } else if (valid) {
#pragma unroll
    for (int q = 0; q < 8; ++q)
      cstore_stream(&a.data[base + ((long)P * Line<M>::last_index(jt, q) + r) * a.ls], cscale(a.scale, v[q]), a.nt);
  }
}

template <int M, int P>
void launch_strided_mixed(const StridedArgs& a0, int nouter, int dir, int ncomp, long cs, const cplx* wN, hipStream_t s) {
  constexpr size_t lds = sub_tile_lds(M, P);
  if constexpr (!sub_one_strided_fits(M, P)) {
    no_launcher("y / x pass");
  } else {
    StridedArgs a = a0;
    a.tiles_per_outer = (a.ncols + 7) / 8;
    const dim3 grid((unsigned)((long)a.tiles_per_outer * nouter), ncomp);
    static PerDeviceOnce configured;
    if (auto once = configured.first_use()) {
      FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_strided_mixed<M, P, -1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_strided_mixed<M, P, +1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (dir < 0) hipLaunchKernelGGL((k_strided_mixed<M, P, -1>), grid, dim3(M * P), lds, s, a, cs, wN);
    else hipLaunchKernelGGL((k_strided_mixed<M, P, +1>), grid, dim3(M * P), lds, s, a, cs, wN);
    FG_HIP_CHECK(hipGetLastError());
  }
}

// The z passes in one kernel each, same construction: a workgroup owns LINES packed rows, thread (l, jt, r) runs the
// MP-point transform of sub-row r of row l (lanes run over (jt, r): the loads p * idx + r are contiguous), the
// combine + real split (r2c) / merge + inverse combine (c2r) goes through an LDS image [l][r][k'].
template <int MP, int P, int LINES, bool FWD>
__global__ __launch_bounds__((MP / 8) * P * LINES) void k_z_mixed(double* data, long nrows, int nzp, long comp_stride,
                                                                 const cplx* tw, const cplx* wn) {
  using namespace fft;
  constexpr int T = MP / 8, COLS = P * LINES, THREADS = T * COLS, PN = MP + MP / 8, M = P * MP, nz = 2 * M;
  extern __shared__ __align__(16) double lds[];
  cplx* img = reinterpret_cast<cplx*>(lds);   // [LINES][P][MP]
  data += (long)blockIdx.y * comp_stride;
  const int tid = threadIdx.x;
  // lanes: r fastest, then jt, then the row: global accesses p * idx + r are contiguous along (jt, r)
  const int r = tid % P, jt = (tid / P) % T, l = tid / (P * T);
  const int cp = l * P + r;   // LDS column of this sub-row
  const long row0 = (long)blockIdx.x * LINES;
  const bool valid = row0 + l < nrows;
  cplx* row = reinterpret_cast<cplx*>(data + (row0 + (valid ? l : 0)) * nzp);
  const LdsMap L = {COLS, 1, PN * COLS};
  cplx v[8];
  if (FWD) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = valid ? row[P * Line<MP>::first_index(jt, q) + r] : cmake(0.0, 0.0);
    MixedPhases<MP, -1, 0>::run(v, jt, lds, L, cp, tw);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) img[((long)l * P + r) * MP + Line<MP>::last_index(jt, q)] = v[q];
    __syncthreads();
    // combine + split: item (row, k <= M/2) -> X[k], X[M - k]
    constexpr int half = M / 2 + 1;
    for (int it = tid; it < LINES * half; it += THREADS) {
      const int lr = it / half, k = it % half;
      if (row0 + lr >= nrows) break;
      const cplx* in = img + (long)lr * P * MP;
      auto zfull = [&](int K) {
        const int kk = K % MP, step = 2 * K;
        cplx acc = cmake(0.0, 0.0);
        int idx = 0;
#pragma unroll
        for (int rr = 0; rr < P; ++rr) {
          acc = cadd(acc, cmul(in[rr * MP + kk], wn[idx]));
          idx += step;
          if (idx >= nz) idx -= nz;
        }
        return acc;
      };
      const cplx zk = zfull(k), zm = zfull((M - k) % M);
      cplx* out = reinterpret_cast<cplx*>(data + (row0 + lr) * nzp);
      out[k] = r2c_split(zk, zm, wn[k]);
      out[M - k] = r2c_split(zm, zk, wn[M - k]);
    }
  } else {
    // merge + inverse combine: item (row, k' < MP) -> Z_r[k'] for all r
    for (int it = tid; it < LINES * MP; it += THREADS) {
      const int lr = it / MP, kk = it % MP;
      if (row0 + lr >= nrows) break;
      const cplx* in = reinterpret_cast<const cplx*>(data + (row0 + lr) * nzp);
      cplx z[P];
#pragma unroll
      for (int sidx = 0; sidx < P; ++sidx) {
        const int K = kk + MP * sidx;
        cplx xk = in[K], xm = in[M - K];
        if (K == 0) { xk.im = 0.0; xm.im = 0.0; }
        z[sidx] = c2r_merge(xk, xm, wn[K]);
      }
#pragma unroll
      for (int rr = 0; rr < P; ++rr) {
        cplx acc = cmake(0.0, 0.0);
        const int step = (2 * rr * MP) % nz;
        int idx = 0;
#pragma unroll
        for (int sidx = 0; sidx < P; ++sidx) {
          acc = cadd(acc, cmul(z[sidx], cconj(wn[idx])));
          idx += step;
          if (idx >= nz) idx -= nz;
        }
        img[((long)lr * P + rr) * MP + kk] = cmul(acc, cconj(wn[2 * rr * kk]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = img[((long)l * P + r) * MP + Line<MP>::first_index(jt, q)];
    __syncthreads();
    MixedPhases<MP, +1, 0>::run(v, jt, lds, L, cp, tw);
    if (valid) {
#pragma unroll
      for (int q = 0; q < 8; ++q) row[P * Line<MP>::last_index(jt, q) + r] = v[q];
    }
  }
}

template <int MP, int P>
void launch_z_mixed(double* data, long nrows, int nzp, int ncomp, long comp_stride, bool fwd, const cplx* tw, const cplx* wn,
                    hipStream_t s) {
  constexpr int LINES = sub_z_lines(MP, P), THREADS = sub_z_threads(MP, P);
  constexpr size_t lds = sub_z_lds(MP, P);
  if constexpr (!sub_one_z_fits(MP, P)) {
    no_launcher("z pass");
  } else {
    const dim3 grid((unsigned)((nrows + LINES - 1) / LINES), ncomp);
    static PerDeviceOnce configured;
    if (auto once = configured.first_use()) {
      FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_z_mixed<MP, P, LINES, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_z_mixed<MP, P, LINES, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    if (fwd) hipLaunchKernelGGL((k_z_mixed<MP, P, LINES, true>), grid, dim3(THREADS), lds, s, data, nrows, nzp, comp_stride, tw, wn);
    else hipLaunchKernelGGL((k_z_mixed<MP, P, LINES, false>), grid, dim3(THREADS), lds, s, data, nrows, nzp, comp_stride, tw, wn);
    FG_HIP_CHECK(hipGetLastError());
  }
}

// The fused pass (x-FFT, 1/N, Green operator, x-iFFT on three components) for N = p M, p = 3 or 5: per component the
// sub-line transforms and the LDS image as in k_strided_mixed; the combine outputs X[k + M s] of a (k, column) item stay
// in the registers of the thread that formed them -- the same thread owns every input of the inverse combine of that
// item, so the Green operator and the inverse combine need no exchange.  One read and one write of the three spectra.
template <int M, int P>
__global__ __launch_bounds__(M * P) void k_xfused_mixed(XFusedArgs a, const cplx* wN) {
  using namespace fft;
  constexpr int T = M / 8, COLS = P * 8, THREADS = T * COLS, PN = M + M / 8, N = P * M;
  constexpr int ITEMS = (8 + P - 1) / P;   // (k, column) items per thread: M * 8 items over M * P threads
  extern __shared__ __align__(16) double lds[];
  cplx* img = reinterpret_cast<cplx*>(lds);
  const int tid = threadIdx.x;
  const int cp = tid % COLS, jt = tid / COLS, r = cp / 8, t = cp % 8;
  const int o = blockIdx.x / a.tiles_per_outer;
  const int col = (blockIdx.x % a.tiles_per_outer) * 8 + t;
  const bool valid = col < a.ncols;
  const int colc = valid ? col : a.ncols - 1;
  const long base = (long)o * a.os + colc;
  int jj, kk;
  if (a.flat_cols) {
    const int jl = colc / a.nzc;
    jj = a.jj0 + jl;
    kk = colc - jl * a.nzc;
  } else {
    jj = a.jj0 + o;
    kk = colc;
  }
  const LdsMap L = {COLS, 1, PN * COLS};
  cplx v[8];
  cplx X[ITEMS][3][P];
  // ---- forward: three components
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const cplx* src = a.data + c * a.comp_stride;
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = cload_stream(&src[base + ((long)P * Line<M>::first_index(jt, q) + r) * a.ls], a.nt);
    MixedPhases<M, -1, 0>::run(v, jt, lds, L, cp, a.tw);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) img[((long)r * M + Line<M>::last_index(jt, q)) * 8 + t] = v[q];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int k = tid / 8 + i * (THREADS / 8);
      if (k < M) {
        cplx in[P];
#pragma unroll
        for (int rr = 0; rr < P; ++rr) in[rr] = img[((long)rr * M + k) * 8 + t];
#pragma unroll
        for (int sidx = 0; sidx < P; ++sidx) {
          cplx acc = cmake(0.0, 0.0);
          const int step = k + M * sidx;
          int idx = 0;
#pragma unroll
          for (int rr = 0; rr < P; ++rr) {
            acc = cadd(acc, cmul(in[rr], wN[idx]));
            idx += step;
            if (idx >= N) idx -= N;
          }
          X[i][c][sidx] = cscale(a.scale, acc);
        }
      }
    }
    __syncthreads();   // the image is overwritten by the next component's exchange planes
  }
  // ---- Green operator and inverse combine, in registers
  const bool live = valid && kk < a.nzf;
  const double kpm1 = a.kpm[1][jj], kpm2 = a.kpm[2][live ? kk : 0];
  const cplx kp1 = a.kp[1][jj], kp2 = a.kp[2][live ? kk : 0];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int k = tid / 8 + i * (THREADS / 8);
    if (k < M) {
#pragma unroll
      for (int sidx = 0; sidx < P; ++sidx) {
        const int kx = k + M * sidx;
        const cplx t0 = X[i][0][sidx], t1 = X[i][1][sidx], t2 = X[i][2][sidx];
        if (live) {
          cplx e0, e1, e2;
          g0_point_rcp(t0, t1, t2, a.kpm[0][kx], kpm1, kpm2, a.kp[0][kx], kp1, kp2, a.c10, a.c20, &e0, &e1, &e2);
          const bool zero = kx == 0 && jj == 0 && kk == 0;   // zero frequency  F:19924-19926
          X[i][0][sidx] = zero ? cmake(0.0, 0.0) : e0;
          X[i][1][sidx] = zero ? cmake(0.0, 0.0) : e1;
          X[i][2][sidx] = zero ? cmake(0.0, 0.0) : e2;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        cplx in[P];
#pragma unroll
        for (int sidx = 0; sidx < P; ++sidx) in[sidx] = X[i][c][sidx];
#pragma unroll
        for (int rr = 0; rr < P; ++rr) {   // Z_r[k] = conj(w_N^{r k}) sum_s X[k + M s] conj(w_p^{r s})
          cplx acc = cmake(0.0, 0.0);
          const int step = (rr * M) % N;
          int idx = 0;
#pragma unroll
          for (int sidx = 0; sidx < P; ++sidx) {
            acc = cadd(acc, cmul(in[sidx], cconj(wN[idx])));
            idx += step;
            if (idx >= N) idx -= N;
          }
          X[i][c][rr] = cmul(acc, cconj(wN[rr * k]));
        }
      }
    }
  }
  // ---- inverse: three components
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int k = tid / 8 + i * (THREADS / 8);
      if (k < M) {
#pragma unroll
        for (int rr = 0; rr < P; ++rr) img[((long)rr * M + k) * 8 + t] = X[i][c][rr];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = img[((long)r * M + Line<M>::first_index(jt, q)) * 8 + t];
    __syncthreads();
    MixedPhases<M, +1, 0>::run(v, jt, lds, L, cp, a.tw);
    if (valid) {
      cplx* dst = a.data + c * a.comp_stride;
#pragma unroll
      for (int q = 0; q < 8; ++q) cstore_stream(&dst[base + ((long)P * Line<M>::last_index(jt, q) + r) * a.ls], v[q], a.nt);
    }
    __syncthreads();   // exchange planes -> image of the next component
  }
}

template <int M, int P>
void launch_xfused_mixed(XFusedArgs a, int nouter, const cplx* wN, hipStream_t s) {
  constexpr size_t lds = sub_tile_lds(M, P);
  if constexpr (!sub_one_fused_fits(M, P)) {   // (N <= 512: fg_fft_route.h)
    no_launcher("fused pass");
  } else {
    a.tiles_per_outer = (a.ncols + 7) / 8;
    static PerDeviceOnce configured;
    if (auto once = configured.first_use()) {
      FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xfused_mixed<M, P>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    hipLaunchKernelGGL((k_xfused_mixed<M, P>), dim3((unsigned)((long)a.tiles_per_outer * nouter)), dim3(M * P), lds, s, a, wN);
    FG_HIP_CHECK(hipGetLastError());
  }
}

// z axis, nz = 2 M, M = p M': after the M'-point sub-transforms of the packed rows (Y_r[k'] at complex p k' + r), one
// sweep per row forms the M-point spectrum Z and splits it into the half spectrum of the real row (r2c_split):
// thread k <= M/2 writes X[k] and X[M - k].  wn: e^{-2 pi i j / nz}, j < nz  (w_M^j = wn[2 j]).
// Both z sweeps work in place: a workgroup owns `rows` whole rows, forms their outputs in an LDS image and writes them
// back after a barrier (no scratch component, no copy).
template <int P>
__global__ __launch_bounds__(256) void k_mixed_r2c_finish(double* data, long nrows, int nzp, int M, int p_rt, int rows,
                                                          const cplx* wn) {
  extern __shared__ __align__(16) double lds_raw[];
  cplx* img = reinterpret_cast<cplx*>(lds_raw);   // [rows][M + 1]
  const int p = P ? P : p_rt;
  const int half = M / 2 + 1;
  const long row0 = (long)blockIdx.x * rows;
  const int Mp = M / p, nz = 2 * M;
  for (int it = threadIdx.x; it < rows * half; it += 256) {
  const int lr = it / half;
  const long row = row0 + lr;
  if (row >= nrows) break;
  const int k = it % half;
  const cplx* in = reinterpret_cast<const cplx*>(data + row * nzp);
  cplx* out = img + (long)lr * (M + 1);
  auto zfull = [&](int K) {   // Z[K], K in [0, M)
    const int kk = K % Mp, sidx = K / Mp;
    cplx acc = cmake(0.0, 0.0);
    const int step = 2 * (kk + sidx * Mp);   // = 2 K < nz
    int idx = 0;
#pragma unroll
    for (int r = 0; r < p; ++r) {
      acc = cadd(acc, cmul(in[p * kk + r], wn[idx]));
      idx += step;
      if (idx >= nz) idx -= nz;
    }
    return acc;
  };
  const cplx zk = zfull(k), zm = zfull((M - k) % M);
  out[k] = r2c_split(zk, zm, wn[k]);
  out[M - k] = r2c_split(zm, zk, wn[M - k]);   // k = 0 writes the Nyquist bin X[M] = split(Z[0], Z[0])
  }
  __syncthreads();
  for (int it = threadIdx.x; it < rows * (M + 1); it += 256) {
    const int lr = it / (M + 1);
    if (row0 + lr >= nrows) break;
    reinterpret_cast<cplx*>(data + (row0 + lr) * nzp)[it % (M + 1)] = img[it];
  }
}

// inverse: merge the half spectrum into Z' (c2r_merge), then the inverse combine to the sub-rows:
// thread k' < M' reads X[k' + M' s], X[M - k' - M' s] and writes Z_r[k'] to complex p k' + r.
template <int P>
__global__ __launch_bounds__(256) void k_mixed_c2r_start(double* data, long nrows, int nzp, int M, int p_rt, int rows,
                                                         const cplx* wn) {
  extern __shared__ __align__(16) double lds_raw[];
  cplx* img = reinterpret_cast<cplx*>(lds_raw);   // [rows][M]
  const int p = P ? P : p_rt;
  const int Mp = M / p, nz = 2 * M;
  const long row0 = (long)blockIdx.x * rows;
  for (int it = threadIdx.x; it < rows * Mp; it += 256) {
  const int lr = it / Mp;
  const long row = row0 + lr;
  if (row >= nrows) break;
  const int kk = it % Mp;
  const cplx* in = reinterpret_cast<const cplx*>(data + row * nzp);
  cplx* out = img + (long)lr * M;
  cplx z[P ? P : kMaxOddFactor];
#pragma unroll
  for (int sidx = 0; sidx < p; ++sidx) {
    const int K = kk + Mp * sidx;
    cplx xk = in[K], xm = in[M - K];
    if (K == 0) { xk.im = 0.0; xm.im = 0.0; }   // FFTW's c2r ignores the imaginary parts of the DC and Nyquist bins
    z[sidx] = c2r_merge(xk, xm, wn[K]);
  }
#pragma unroll
  for (int r = 0; r < p; ++r) {
    cplx acc = cmake(0.0, 0.0);
    const int step = (int)((2L * r * Mp) % nz);
    int idx = 0;
#pragma unroll
    for (int sidx = 0; sidx < p; ++sidx) {
      acc = cadd(acc, cmul(z[sidx], cconj(wn[idx])));
      idx += step;
      if (idx >= nz) idx -= nz;
    }
    out[p * kk + r] = cmul(acc, cconj(wn[2 * r * kk]));   // 2 r k' < nz
  }
  }
  __syncthreads();
  for (int it = threadIdx.x; it < rows * M; it += 256) {
    const int lr = it / M;
    if (row0 + lr >= nrows) break;
    reinterpret_cast<cplx*>(data + (row0 + lr) * nzp)[it % M] = img[it];
  }
}
#pragma clang diagnostic pop

// the sweeps of the sub-lines + combine family on one component (P = 0: p at run time)
template <int DIR, int P>
void launch_combine_tile(cplx* d, long ls, long os, int ncols, int nouter, int m, int p, double scale, const cplx* w, hipStream_t s) {
  static PerDeviceOnce configured;
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mixed_combine_tile<DIR, P>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  const int tiles = (ncols + 7) / 8;
  hipLaunchKernelGGL((k_mixed_combine_tile<DIR, P>), dim3((unsigned)((long)tiles * nouter)), dim3(256),
                     (size_t)p * m * 8 * sizeof(cplx), s, d, ls, os, ncols, tiles, m, p, scale, w);
}
template <int DIR, int P>
void launch_combine_scratch(const cplx* src, cplx* dst, long ls, long os, int ncols, int nouter, int m, int p, double scale,
                            const cplx* w, hipStream_t s) {
  const unsigned nb = (unsigned)(((long)nouter * m * ncols + 255) / 256);
  hipLaunchKernelGGL((k_mixed_combine<DIR, P>), dim3(nb), dim3(256), 0, s, src, dst, ls, os, ncols, nouter, m, p, scale, w);
}
// r2c finish (FWD) / c2r start of the z rows: `rows` rows per workgroup in 48 KB of LDS
template <bool FWD, int P>
void launch_z_sweep(double* data, long nrows, int nzp, int M, int p, const cplx* wn, hipStream_t s) {
  constexpr auto kernel = FWD ? &k_mixed_r2c_finish<P> : &k_mixed_c2r_start<P>;
  static PerDeviceOnce configured;
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  int rows = (int)(48 * 1024 / ((M + 1) * sizeof(cplx)));
  if (rows < 1) rows = 1;
  const size_t lds = (size_t)rows * (M + 1) * sizeof(cplx);
  const dim3 grid((unsigned)((nrows + rows - 1) / rows));
  if constexpr (FWD) hipLaunchKernelGGL(k_mixed_r2c_finish<P>, grid, dim3(256), lds, s, data, nrows, nzp, M, p, rows, wn);
  else hipLaunchKernelGGL(k_mixed_c2r_start<P>, grid, dim3(256), lds, s, data, nrows, nzp, M, p, rows, wn);
}

cplx* upload(const std::vector<cplx>& v) {
  cplx* d = nullptr;
  FG_HIP_CHECK(hipMalloc(&d, v.size() * sizeof(cplx)));
  FG_HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(cplx), hipMemcpyHostToDevice));
  return d;
}

template <class K>
void launch_strided(const StridedArgs& a, long nblocks, int ncomp, long comp_stride, hipStream_t s) {
  static PerDeviceOnce configured;
  const size_t lds = K::LDS_DOUBLES * sizeof(double);
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_strided<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(k_strided<K>, dim3((unsigned)nblocks, ncomp), dim3(K::THREADS), lds, s, a, comp_stride);
  FG_HIP_CHECK(hipGetLastError());
}

template <class K>
void launch_plane(const PlaneArgs& a, int nplanes, int ncomp, long comp_stride, hipStream_t s) {
  static PerDeviceOnce configured;
  const size_t lds = K::LDS_DOUBLES * sizeof(double);
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_plane<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(k_plane<K>, dim3((unsigned)nplanes, ncomp), dim3(K::THREADS), lds, s, a, comp_stride);
  FG_HIP_CHECK(hipGetLastError());
}

// (ny, nz / 2) pairs the plane kernels are built for: THREADS = ny * nz / 16 <= 1024, the complex plane within the LDS
template <int NY, int M>
bool plane_nm(int ny, int m, bool probe, const PlaneArgs& a, int nplanes, int ncomp, long cs, int dir, hipStream_t s) {
  if (ny != NY || m != M) return false;
  if (probe) return true;
  if (dir < 0) launch_plane<ZYKernel<NY, M>>(a, nplanes, ncomp, cs, s);
  else launch_plane<YZKernel<NY, M>>(a, nplanes, ncomp, cs, s);
  return true;
}
bool plane_dispatch(int ny, int m, bool probe, const PlaneArgs& a, int nplanes, int ncomp, long cs, int dir, hipStream_t s) {
#define FG_PLANE(NY, M) plane_nm<NY, M>(ny, m, probe, a, nplanes, ncomp, cs, dir, s)
  return FG_PLANE(16, 8) || FG_PLANE(16, 16) || FG_PLANE(16, 32) || FG_PLANE(16, 64) || FG_PLANE(32, 8) || FG_PLANE(32, 16) ||
         FG_PLANE(32, 32) || FG_PLANE(32, 64) || FG_PLANE(64, 8) || FG_PLANE(64, 16) || FG_PLANE(64, 32) || FG_PLANE(64, 64) ||
         FG_PLANE(128, 8) || FG_PLANE(128, 16) || FG_PLANE(128, 32) || FG_PLANE(128, 64) || FG_PLANE(256, 8) ||
         FG_PLANE(256, 16) || FG_PLANE(256, 32);   // (256, 64): 264 KB
#undef FG_PLANE
}

template <class K>
void launch_z(const ZArgs& a, int ncomp, long comp_stride, int lines, hipStream_t s) {
  static PerDeviceOnce configured;
  const size_t lds = K::LDS_DOUBLES * sizeof(double);
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_zpass<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  long nblocks = (a.nrows + lines - 1) / lines;
  hipLaunchKernelGGL(k_zpass<K>, dim3((unsigned)nblocks, ncomp), dim3(K::THREADS), lds, s, a, comp_stride);
  FG_HIP_CHECK(hipGetLastError());
}

template <int N, int C, int NC, bool XSPLIT = false, int NTC = -1>
void xfused_nc(XFusedArgs a, int nouter, hipStream_t s);

template <int N>
void xfused_n(XFusedArgs a, int nouter, int ncomp, hipStream_t s) {
  // (half-segment tiles, C = 4, were measured for N = 512: 2.96 ms against 2.5 ms)
  // three components: 8-column (128-byte) tiles whatever the length -- more, smaller workgroups balance better over the
  // 256 CUs than 256-thread tiles of short lines (128^3: 0.037 -> 0.035 ms, 6 220 -> 6 315 it/s; 64^3: +1 %)
  if constexpr (N == 1024) {
    // 1024-point lines: the exchange buffer of an 8-column tile (147 KB) leaves no room for 512 threads' worth of registers
    // (16 waves: 128 VGPRs each, the three spectra alone take 96) -- half-segment tiles, still one pass instead of three
    if (ncomp == 1) xfused_nc<N, 4, 1>(a, nouter, s);   // (8 columns = 16 waves at 128 VGPRs: 33 spilled)
    else if (a.xjump != 0) throw std::runtime_error("fft: interleaved slab layout: x lines up to 512");
    else xfused_nc<N, 4, 3>(a, nouter, s);
  } else {
    // (r5: the scalar modes' pass keeps its pass twiddles in LDS like the three-component one -- XFusedKernel::TW_LDS -- 256^3 porous
    // K4 0.083 -> 0.073 ms, 2 765 -> 2 830 it/s; on cache-resident grids also the branch-free loads, 128^3 porous 14 030 -> 14 370)
    if (ncomp == 1 && (N == 64 || N == 128) && a.nt == 0)
      xfused_nc<N, XTileCols<N>::value, 1, false, ((N == 64 || N == 128) ? 16 : -1)>(a, nouter, s);
    else if (ncomp == 1) xfused_nc<N, XTileCols<N>::value, 1>(a, nouter, s);
    // Cache-resident fields (nt = 0: three components within the Infinity Cache -- 128^3 and below, and the slabs of 256^3 on 8
    // GPUs) with lines up to 256 points: the tile's loads without branches and all issued up front, so that the first component's
    // transform starts when ITS eight loads have landed (s_waitcnt vmcnt(16)) instead of after all 24.  r5, one job each: K4 at
    // 128^3 31.5 -> 28.5 us (7 560 -> 7 705 it/s), 64^3 10.0 -> 9.3 us; one slab of eight at 256^3 (interleaved layout) 42.6 ->
    // 38.9 us, 256 x 32 x 256 33.4 -> 30.0 us; 256^3 and 512^3 on one GPU (streaming, nt = 3) measured equal and keep the
    // run-time flags
    else if (a.xjump != 0 && (N == 64 || N == 128 || N == 256) && a.nt == 0)
      xfused_nc<N, 8, 3, true, ((N == 64 || N == 128 || N == 256) ? 16 : -1)>(a, nouter, s);
    else if (a.xjump != 0) xfused_nc<N, 8, 3, true>(a, nouter, s);   // slab decomposition, components interleaved per peer
    else if ((N == 64 || N == 128 || N == 256) && a.nt == 0)
      xfused_nc<N, 8, 3, false, ((N == 64 || N == 128 || N == 256) ? 16 : -1)>(a, nouter, s);
    else xfused_nc<N, 8, 3>(a, nouter, s);
  }
}

template <int N, int C, int NC, bool XSPLIT, int NTC>
void xfused_nc(XFusedArgs a, int nouter, hipStream_t s) {
  using K = XFusedKernel<N, C, NC, XSPLIT, NTC>;
  static PerDeviceOnce configured;
  const size_t lds = K::LDS_DOUBLES * sizeof(double);
  if (auto once = configured.first_use()) {
    FG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_xfused<K>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  a.tiles_per_outer = (a.ncols + C - 1) / C;
  const long nblocks = (long)a.tiles_per_outer * nouter;
  a.xcd_order = 1;   // every XCD a contiguous run of tiles (512^3 1.84 -> 1.80 ms, 256^3 0.200 -> 0.188 ms)
  static cplx xq[8];
  static bool have_xq = false;
  if (!have_xq) {
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int q = 0; q < 8; ++q) {
      const long double th = pi * (long double)fft::Line<N>::last_index(0, q) / (long double)N;
      xq[q] = cmake((double)cosl(th), (double)sinl(th));
    }
    have_xq = true;
  }
  for (int q = 0; q < 8; ++q) a.xq[q] = xq[q];
  // (persistent / looping forms of this kernel lose to fresh workgroups: DESIGN 3.4, 3.6)
  hipLaunchKernelGGL(k_xfused<K>, dim3((unsigned)nblocks), dim3(K::THREADS), lds, s, a);
  FG_HIP_CHECK(hipGetLastError());
}

// StridedArgs::images picks the kernel with one or two exchange planes (a one-pass line, N = 8, exchanges nothing)
template <int N, int C>
void launch_strided_images(const StridedArgs& a, long nblocks, int dir, int ncomp, long comp_stride, hipStream_t s) {
  if constexpr (num_passes(N) > 1) {
    if (a.images == 1) {
      if (dir < 0) launch_strided<StridedKernel<N, C, -1, 1>>(a, nblocks, ncomp, comp_stride, s);
      else launch_strided<StridedKernel<N, C, +1, 1>>(a, nblocks, ncomp, comp_stride, s);
      return;
    }
  }
  if (dir < 0) launch_strided<StridedKernel<N, C, -1>>(a, nblocks, ncomp, comp_stride, s);
  else launch_strided<StridedKernel<N, C, +1>>(a, nblocks, ncomp, comp_stride, s);
}

template <int N>
void strided_n(const StridedArgs& a0, int nouter, int dir, int ncomp, long comp_stride, hipStream_t s) {
  constexpr int C = TileCols<N>::value;
  StridedArgs a = a0;
  a.tiles_per_outer = (a.ncols + C - 1) / C;
  long nblocks = (long)a.tiles_per_outer * nouter;
  launch_strided_images<N, C>(a, nblocks, dir, ncomp, comp_stride, s);
}

// the same with 8-column tiles whatever the length (sub-rows of the z pass have only p <= 15 columns)
template <int N>
void strided_n8(const StridedArgs& a0, int nouter, int dir, int ncomp, long comp_stride, hipStream_t s) {
  StridedArgs a = a0;
  a.tiles_per_outer = (a.ncols + 7) / 8;
  long nblocks = (long)a.tiles_per_outer * nouter;
  launch_strided_images<N, 8>(a, nblocks, dir, ncomp, comp_stride, s);
}
void strided_pow2_narrow(int n, const StridedArgs& a, int nouter, int dir, int ncomp, long cs, hipStream_t s) {
  switch (n) {
    case 8: strided_n8<8>(a, nouter, dir, ncomp, cs, s); break;
    case 16: strided_n8<16>(a, nouter, dir, ncomp, cs, s); break;
    case 32: strided_n8<32>(a, nouter, dir, ncomp, cs, s); break;
    case 64: strided_n8<64>(a, nouter, dir, ncomp, cs, s); break;
    case 128: strided_n8<128>(a, nouter, dir, ncomp, cs, s); break;
    case 256: strided_n8<256>(a, nouter, dir, ncomp, cs, s); break;
    case 512: strided_n8<512>(a, nouter, dir, ncomp, cs, s); break;
    case 1024: strided_n8<1024>(a, nouter, dir, ncomp, cs, s); break;
    default: throw std::runtime_error("fft: unsupported fast length");
  }
}

void strided_pow2(int n, const StridedArgs& a, int nouter, int dir, int ncomp, long cs, hipStream_t s) {
  // short lines use 16- to 256-column tiles (256 threads); when the columns do not fill the last tile of a row -- 128^3:
  // 72 columns = 4.5 tiles of 16 -- 8-column tiles waste nothing and balance better: y passes 0.028 -> 0.026 ms,
  // 128^3 6 365 -> 6 590 it/s, 64^3 +2 %
  if (n <= 128 && a.ncols % (2048 / n > 8 ? 2048 / n : 8) != 0) return strided_pow2_narrow(n, a, nouter, dir, ncomp, cs, s);
  switch (n) {
    case 8: strided_n<8>(a, nouter, dir, ncomp, cs, s); break;
    case 16: strided_n<16>(a, nouter, dir, ncomp, cs, s); break;
    case 32: strided_n<32>(a, nouter, dir, ncomp, cs, s); break;
    case 64: strided_n<64>(a, nouter, dir, ncomp, cs, s); break;
    case 128: strided_n<128>(a, nouter, dir, ncomp, cs, s); break;
    case 256: strided_n<256>(a, nouter, dir, ncomp, cs, s); break;
    case 512: strided_n<512>(a, nouter, dir, ncomp, cs, s); break;
    case 1024: strided_n<1024>(a, nouter, dir, ncomp, cs, s); break;
    default: throw std::runtime_error("fft: unsupported fast length");
  }
}

// power-of-two z pass, K = R2CKernel / C2RKernel.  64 ... 512 packed points: the mirrored value of the real split / merge comes
// from the lane that holds it (wave shuffle) instead of a round trip of the spectrum through LDS / a second global load --
// r2c 512^3 1.30 -> 1.16 ms, 256^3 0.158 -> 0.155 ms; c2r 256^3 0.164 -> 0.151 ms, 512^3 1.38 -> 1.19 ms
template <template <int, int, bool, int> class K>
void z_pow2(int m, const ZArgs& a, int ncomp, long cs, hipStream_t s) {
  switch (m) {
#define FG_CASE(M) case M: return launch_z<K<M, ZLines<M>::value, false, 2>>(a, ncomp, cs, ZLines<M>::value, s);
    FG_CASE(8) FG_CASE(16) FG_CASE(32) FG_CASE(1024)
#undef FG_CASE
#define FG_CASE(M)                                                                                              \
  case M:                                                                                                       \
    return a.images == 1 ? launch_z<K<M, ZLines<M>::value, true, 1>>(a, ncomp, cs, ZLines<M>::value, s)         \
                         : launch_z<K<M, ZLines<M>::value, true, 2>>(a, ncomp, cs, ZLines<M>::value, s);
    FG_CASE(64) FG_CASE(128) FG_CASE(256) FG_CASE(512)
#undef FG_CASE
    default: throw std::runtime_error("fft: unsupported fast z length");
  }
}

}  // namespace

Fft3::Fft3(const Grid& g, hipStream_t stream) : g_(g), stream_(stream) {
  const int len[3] = {g.nx, g.ny, g.nz};
  bool need_scratch = false;
  for (int a = 0; a < 3; ++a) {
    const AxisRoute& r = route_[a] = route_axis(a, len[a]);
    if (r.pass_twiddles) tw_[a] = upload(make_pass_twiddles(r.pass_twiddles));
    if (r.half_roots) half_root_[a] = upload(make_unit_roots(2 * len[a], len[a] / 8));
    if (r.z_roots) wz_ = upload(make_unit_roots(g.nz, g.nz / 2 + 1));
    if (r.unit_roots) wgen_[a] = upload(make_unit_roots(len[a], len[a]));
    if (r.blue.n) {
      blue_tab_[a][0] = upload(make_bluestein_chirp(r.line));
      blue_tab_[a][1] = upload(make_bluestein_filter(r.line, r.blue.m()));
      blue_tab_[a][2] = upload(make_unit_roots(r.blue.m(), r.blue.m()));
    }
    need_scratch |= r.scratch;
  }
  route_fused();
  if (need_scratch) FG_HIP_CHECK(hipMalloc(&scratch_, g.n * sizeof(double)));
  // three components larger than the 256 MB Infinity Cache: nothing a pass writes is still cached when the next reads it
  stream_stores_ = 3.0 * (double)g.n * sizeof(double) > 256.0 * 1024 * 1024 ? 1 : 0;
}

void Fft3::route_fused() {
  const int len[2] = {g_.nx, g_.ny};
  for (int a = 0; a < 2; ++a)
    for (int three = 0; three < 2; ++three) fused_[a][three] = route_fused_x(len[a], three ? 3 : 1, joint_x_, a);
}

void Fft3::set_joint_x(bool on) {
  if (on == joint_x_) return;
  joint_x_ = on;
  route_fused();
}

Fft3::~Fft3() {
  for (int a = 0; a < 3; ++a) {
    if (tw_[a]) (void)hipFree(tw_[a]);
    if (a < 2 && half_root_[a]) (void)hipFree(half_root_[a]);
    if (wgen_[a]) (void)hipFree(wgen_[a]);
    for (int k = 0; k < 3; ++k)
      if (blue_tab_[a][k]) (void)hipFree(blue_tab_[a][k]);
  }
  if (wz_) (void)hipFree(wz_);
  if (scratch_) (void)hipFree(scratch_);
}

StridedArgs Fft3::strided_args(double* data, int axis, double scale, int nt) const {
  const long plane = (long)g_.ny * g_.nzc;
  StridedArgs a;
  a.data = reinterpret_cast<cplx*>(data);
  a.ls = axis == 0 ? plane : axis == 1 ? g_.nzc : route_[2].p;
  a.os = axis == 0 ? 0 : axis == 1 ? plane : g_.nzc;
  a.ncols = axis == 0 ? (int)plane : axis == 1 ? g_.nzc : route_[2].p;
  a.tiles_per_outer = 0;
  a.scale = scale;
  a.tw = tw_[axis];
  a.nt = nt;
  a.xcd_order = 0;   // (measured for the y passes: 512^3 -1..2 %, 256^3 +2 %)
  // one or two exchange planes: the power-of-two y / x passes only (sub-line, slab and tile-plan kernels keep two)
  a.images = pow2(axis) ? images_for() : 2;
  return a;
}

void Fft3::strided(double* data, int ncomp, long comp_stride, int axis, int dir, double scale, const PlaneWindow* w) {
  const AxisRoute& r = route_[axis];
  const int n = axis == 0 ? g_.nx : g_.ny;
  int nouter = axis == 0 ? 1 : g_.nx;
  const long cs = comp_stride / 2;
  const bool windowed = w && w->np >= 0;
  if (windowed && (axis != 1 || !pow2(1) || w->x0 < 0 || w->x0 + w->np > g_.nx))
    throw std::runtime_error("fft: plane windows need a power-of-two y pass");
  StridedArgs a = strided_args(data, axis, scale, nt_stream());
  switch (r.resolved(bluestein_)) {
    case Family::Len1: return;   // identity; forward() never folds the scale into a length-1 axis
    case Family::Pow2:
      if (windowed) a.data += (long)w->x0 * a.os, nouter = w->np;
      if (nouter == 0) return;
      if (w && w->nt >= 0) a.nt = w->nt;
      return strided_pow2(n, a, nouter, dir, ncomp, cs, stream_);
    case Family::Tile:
      return launch_smooth_strided(SmoothArgs{a.data, a.ls, a.os, a.ncols, 0, scale, wgen_[axis], a.nt, r.plan}, nouter, dir, ncomp, cs, stream_);
    case Family::SubOne:
      return dispatch_p<3, 5, 7, 9>(r.p, [&](auto P) {
        dispatch_sub_m(r.m, [&](auto M) {
          launch_strided_mixed<decltype(M)::value, decltype(P)::value>(a, nouter, dir, ncomp, cs, wgen_[axis], stream_);
        });
      });
    case Family::SubLds:
    case Family::SubScratch: return strided_sublines(a, nouter, ncomp, comp_stride, axis, dir);
    case Family::Bluestein:
      return launch_bluestein_strided(BluesteinArgs{a.data, a.ls, a.os, a.ncols, 0, scale, a.nt, dir, n, blue_tables(axis), r.blue.pass},
                                      nouter, ncomp, cs, stream_);
    case Family::Quadratic: break;
  }
  // O(n^2) sums: component by component through the scratch buffer
  const long total = (long)nouter * n * a.ncols;
  for (int c = 0; c < ncomp; ++c) {
    cplx* src = reinterpret_cast<cplx*>(data + c * comp_stride);
    hipLaunchKernelGGL(k_dft_strided_generic, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, src,
                       reinterpret_cast<cplx*>(scratch_), a.ls, a.os, a.ncols, nouter, n, dir, scale, wgen_[axis]);
    FG_HIP_CHECK(hipGetLastError());
    FG_HIP_CHECK(hipMemcpyAsync(src, scratch_, g_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
  }
}

// n = p * m: m-point kernels on the p interleaved sub-lines and one combine sweep -- in place through LDS while whole lines of
// an 8-column tile fit (n * 128 bytes), else out of place through the scratch component.  Forward: sub-lines, then combine.
void Fft3::strided_sublines(const StridedArgs& a, int nouter, int ncomp, long comp_stride, int axis, int dir) {
  const AxisRoute& r = route_[axis];
  const int p = r.p, m = r.m;
  const cplx* const w = wgen_[axis];
  auto subs = [&]() {
    for (int q = 0; q < p; ++q) {
      StridedArgs s = a;
      s.data += q * a.ls;
      s.ls = a.ls * p;
      s.scale = 1.0;
      s.nt = 0;
      strided_pow2(m, s, nouter, dir, ncomp, comp_stride / 2, stream_);
    }
  };
  auto combine = [&]() {
    for (int c = 0; c < ncomp; ++c) {
      cplx* d = a.data + c * (comp_stride / 2);
      cplx* const tmp = reinterpret_cast<cplx*>(scratch_);
      if (r.family == Family::SubLds) {
        dispatch_p<3, 5, 7, 9, 15, 25, 0>(p, [&](auto P) {
          if (dir < 0) launch_combine_tile<-1, decltype(P)::value>(d, a.ls, a.os, a.ncols, nouter, m, p, a.scale, w, stream_);
          else launch_combine_tile<+1, decltype(P)::value>(d, a.ls, a.os, a.ncols, nouter, m, p, a.scale, w, stream_);
        });
        FG_HIP_CHECK(hipGetLastError());
      } else {
        dispatch_p<3, 5, 7, 0>(p, [&](auto P) {
          if (dir < 0) launch_combine_scratch<-1, decltype(P)::value>(d, tmp, a.ls, a.os, a.ncols, nouter, m, p, a.scale, w, stream_);
          else launch_combine_scratch<+1, decltype(P)::value>(d, tmp, a.ls, a.os, a.ncols, nouter, m, p, a.scale, w, stream_);
        });
        FG_HIP_CHECK(hipGetLastError());
        FG_HIP_CHECK(hipMemcpyAsync(d, scratch_, g_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
      }
    }
  };
  if (dir < 0) subs(), combine();
  else combine(), subs();
}

// forward transform along `axis` (0 = x of [nx][ny][nzc], 1 = y, used for the x lines of a y-slab),
// scale, Green operator, inverse transform -- one kernel for the three components.
bool Fft3::can_fuse(int axis, int ncomp) const {
  if (axis > 1) return false;
  if (ncomp == 1 || ncomp == 3) return fused_[axis][ncomp == 3].kind != Fused::None;
  return pow2(axis);   // (fused_g0 refuses other component counts)
}

bool Fft3::can_plane() const {
  return pow2(1) && pow2(2) && plane_dispatch(g_.ny, g_.nz / 2, true, PlaneArgs{}, 0, 0, 0, 0, stream_);
}

void Fft3::zy_plane(double* data, int ncomp, long comp_stride, int dir) {
  PlaneArgs a = {data, (long)g_.ny * g_.nzp, g_.nzp, tw_[2], wz_, tw_[1]};
  if (!can_plane() || !plane_dispatch(g_.ny, g_.nz / 2, false, a, g_.nx, ncomp, comp_stride, dir, stream_))
    throw std::runtime_error("fft: plane kernels not available for this grid");
}

bool Fft3::can_xlayout() const {
  return pow2(0) && pow2(1) && g_.nx >= 8 && g_.nx <= 512 && g_.nzc % 8 == 0 && g_.ny >= 8;
}

void Fft3::c2c_y_xlayout(double* in, long in_cs, double* out, long out_cs, int ncomp, int dir, double scale, const PlaneWindow* w) {
  if (!can_xlayout()) throw std::runtime_error("fft: x-contiguous layout not available for this grid");
  const bool windowed = w && w->np >= 0;
  if (windowed && (w->x0 < 0 || w->x0 + w->np > g_.nx)) throw std::runtime_error("fft: plane window out of range");
  const int x0 = windowed ? w->x0 : 0, np = windowed ? w->np : g_.nx;
  if (np == 0) return;
  StridedArgs a = strided_args(in, 1, scale, w && w->nt >= 0 ? w->nt : nt_stream());
  a.out = reinterpret_cast<cplx*>(out);
  a.out_cs = out_cs / 2;
  const long plain_ls = a.ls, plain_os = a.os;
  const long xl_ls = (long)g_.nx * 8, xl_os = 8, xl_ts = (long)g_.ny * g_.nx * 8;
  if (dir < 0) {
    a.ls_out = xl_ls;
    a.os_out = xl_os;
    a.ts_out = xl_ts;
    a.data += (long)x0 * plain_os;
    a.out += (long)x0 * xl_os;
  } else {
    a.ls = xl_ls;
    a.os = xl_os;
    a.ts_in = xl_ts;
    a.ls_out = plain_ls;
    a.os_out = plain_os;
    a.data += (long)x0 * xl_os;
    a.out += (long)x0 * plain_os;
  }
  strided_pow2_narrow(g_.ny, a, np, dir, ncomp, in_cs / 2, stream_);   // 8-column tiles: the layout's inner dimension
}

void Fft3::fused_g0(double* data, long comp_stride, int axis, double scale, const G0Params& gp, int jj0, int ncomp, int xsplit,
                    long xjump, bool xlayout) {
  if (ncomp != 1 && ncomp != 3) throw std::runtime_error("fft: fused Green-operator pass takes 1 or 3 components");
  if (!can_fuse(axis, ncomp)) throw std::runtime_error("fft: fused Green-operator pass not available for this length");
  const FusedXRoute& f = fused_[axis][ncomp == 3];
  const int n = axis == 0 ? g_.nx : g_.ny;
  const StridedArgs geo = strided_args(data, axis, scale, nt_stream());
  XFusedArgs a;
  a.data = geo.data;
  a.comp_stride = comp_stride / 2;
  a.ls = geo.ls;
  a.os = geo.os;
  a.ncols = geo.ncols;
  a.tiles_per_outer = 0;
  a.flat_cols = axis == 0 ? 1 : 0;
  a.nzc = g_.nzc;
  a.nzf = g_.nzf;
  a.jj0 = jj0;
  a.scale = scale;
  a.c10 = gp.c10;
  a.c20 = gp.c20;
  a.tw = geo.tw;
  a.half_root = half_root_[axis];
  a.inv_h = gp.inv_h0;
  a.nt = geo.nt;
  for (int k = 0; k < 3; ++k) {
    a.kpm[k] = gp.kpm[k];
    a.kp[k] = gp.kp[k];
  }
  if (xjump != 0) {
    if (f.kind != Fused::Pow2 || axis != 0 || ncomp != 3) throw std::runtime_error("fft: interleaved layout needs the radix x pass");
    a.xsplit = xsplit;
    a.xjump = xjump / 2;
  }
  if (xlayout) {
    if (!can_xlayout() || axis != 0 || ncomp != 3 || xjump != 0) throw std::runtime_error("fft: x-contiguous layout: three components, x pass");
    a.xl_ny = g_.ny;
    a.ls = 8;
    a.flat_cols = 0;
    a.ncols = g_.ny * g_.nzc;   // (tiles = ncols / 8 = (nzc / 8) * ny)
  }
  const int nouter = axis == 0 ? 1 : g_.nx;
  switch (f.kind) {
    case Fused::Tile: {   // ncomp images in LDS
      if (xjump != 0 || xlayout) throw std::runtime_error("fft: the tile kernels' fused x pass takes the plain layout");
      SmoothXArgs x;
      x.base = SmoothArgs{geo.data, geo.ls, geo.os, geo.ncols, 0, scale, wgen_[0], geo.nt, f.plan};
      x.comp_stride = comp_stride / 2;
      x.ncomp = ncomp;
      x.nzc = g_.nzc;
      x.nzf = g_.nzf;
      x.jj0 = jj0;
      x.c10 = gp.c10;
      x.c20 = gp.c20;
      for (int k = 0; k < 3; ++k) x.kpm[k] = gp.kpm[k], x.kp[k] = gp.kp[k];
      return launch_smooth_xfused(x, stream_);
    }
    case Fused::Sub:   // p * 2^k with p = 3, 5: the three-component form only
      return dispatch_p<3, 5>(f.p, [&](auto P) {
        dispatch_sub_m(f.m, [&](auto M) { launch_xfused_mixed<decltype(M)::value, decltype(P)::value>(a, nouter, wgen_[axis], stream_); });
      });
    case Fused::None:   // (refused above)
    case Fused::Pow2: break;
  }
  switch (n) {
    case 8: xfused_n<8>(a, nouter, ncomp, stream_); break;
    case 16: xfused_n<16>(a, nouter, ncomp, stream_); break;
    case 32: xfused_n<32>(a, nouter, ncomp, stream_); break;
    case 64: xfused_n<64>(a, nouter, ncomp, stream_); break;
    case 128: xfused_n<128>(a, nouter, ncomp, stream_); break;
    case 256: xfused_n<256>(a, nouter, ncomp, stream_); break;
    case 512: xfused_n<512>(a, nouter, ncomp, stream_); break;
    case 1024: xfused_n<1024>(a, nouter, ncomp, stream_); break;
    default: throw std::runtime_error("fft: unsupported fused length");
  }
}

bool Fft3::can_block_y(int nranks) const {
  if (nranks < 1 || g_.ny % nranks) return false;
  return pow2(1) && is_pow2(g_.ny / nranks);
}

void Fft3::c2c_y_blocked(double* in, long in_cs, double* out, long out_cs, int ncomp, int dir, double scale, int nranks,
                         int interleave) {
  if (!can_block_y(nranks)) throw std::runtime_error("fft: blocked y pass not available for this length");
  const int nyl = g_.ny / nranks;
  int sh = 0;
  while ((1 << sh) < nyl) ++sh;
  // interleave = 3: a peer's block holds its three components one after the other ([q][c][nx][ny/P][nzc]; the component
  // stride of the blocked side is then ONE block) -- one message per peer
  const long jump = (long)interleave * g_.nx * nyl * g_.nzc - (long)nyl * g_.nzc;
  StridedArgs a = strided_args(in, 1, scale, nt_stream());
  a.images = 2;   // (set_images never reached the slab's y passes)
  a.out = reinterpret_cast<cplx*>(out);
  a.out_cs = out_cs / 2;
  const long plain_os = a.os, blocked_os = (long)nyl * g_.nzc;
  if (dir < 0) {
    a.os_out = blocked_os;
    a.split_out = sh;
    a.jump_out = jump;
  } else {
    a.os = blocked_os;
    a.os_out = plain_os;
    a.split_in = sh;
    a.jump_in = jump;
  }
  strided_pow2(g_.ny, a, g_.nx, dir, ncomp, in_cs / 2, stream_);
}

void Fft3::c2c_y(double* data, int ncomp, long comp_stride, int dir, double scale, const PlaneWindow* w) {
  strided(data, ncomp, comp_stride, 1, dir, scale, w);
}
void Fft3::c2c_x(double* data, int ncomp, long comp_stride, int dir, double scale) {
  strided(data, ncomp, comp_stride, 0, dir, scale);
}
void Fft3::r2c_z(double* data, int ncomp, long comp_stride, const PlaneWindow* w) { z_pass(data, ncomp, comp_stride, true, w); }
void Fft3::c2r_z(double* data, int ncomp, long comp_stride, const PlaneWindow* w) { z_pass(data, ncomp, comp_stride, false, w); }

// r2c (fwd) / c2r along z: the two directions differ in the kernels the family launches, not in how it is chosen
void Fft3::z_pass(double* data, int ncomp, long comp_stride, bool fwd, const PlaneWindow* w) {
  const AxisRoute& r = route_[2];
  long nrows = (long)g_.nx * g_.ny;
  if (w && w->np >= 0) {
    if (!pow2(2) || w->x0 < 0 || w->x0 + w->np > g_.nx) throw std::runtime_error("fft: plane windows need a power-of-two z pass");
    data += (long)w->x0 * g_.ny * g_.nzp;
    nrows = (long)w->np * g_.ny;
    if (nrows == 0) return;
  }
  switch (r.resolved(bluestein_)) {
    case Family::Pow2: {
      ZArgs a = {data, nrows, g_.nzp, tw_[2], wz_, w && w->nt >= 0 ? w->nt : nt_stream()};
      a.images = images_for();
      return fwd ? z_pow2<R2CKernel>(r.line, a, ncomp, comp_stride, stream_) : z_pow2<C2RKernel>(r.line, a, ncomp, comp_stride, stream_);
    }
    case Family::Tile:
      return launch_smooth_z(SmoothZArgs{data, nrows, g_.nzp, wgen_[2], nt_stream(), r.plan, r.zodd ? 1 : 0}, fwd, ncomp, comp_stride, stream_);
    case Family::SubOne:
      return dispatch_p<3, 5, 7, 9>(r.p, [&](auto P) {
        dispatch_sub_m(r.m, [&](auto M) {
          launch_z_mixed<decltype(M)::value, decltype(P)::value>(data, nrows, g_.nzp, ncomp, comp_stride, fwd, tw_[2], wgen_[2], stream_);
        });
      });
    case Family::SubLds:
    case Family::SubScratch: return z_sublines(data, nrows, ncomp, comp_stride, fwd);
    case Family::Bluestein:
      return launch_bluestein_z(BluesteinZArgs{data, nrows, g_.nzp, nt_stream(), fwd ? 1 : 0, g_.nz % 2, r.blue.n, blue_tables(2), wgen_[2], r.blue.pass},
                                ncomp, comp_stride, stream_);
    case Family::Len1:
    case Family::Quadratic: break;
  }
  const dim3 grid((unsigned)((nrows * (fwd ? g_.nzc : g_.nz) + 255) / 256));
  for (int c = 0; c < ncomp; ++c) {
    double* src = data + c * comp_stride;
    if (fwd) hipLaunchKernelGGL(k_r2c_generic, grid, dim3(256), 0, stream_, src, scratch_, nrows, g_.nz, g_.nzp, wgen_[2]);
    else hipLaunchKernelGGL(k_c2r_generic, grid, dim3(256), 0, stream_, src, scratch_, nrows, g_.nz, g_.nzp, wgen_[2]);
    FG_HIP_CHECK(hipGetLastError());
    FG_HIP_CHECK(hipMemcpyAsync(src, scratch_, g_.n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
  }
}

// nz = 2 M, M = p m: m-point kernels on the sub-rows of the packed real rows ([m][p] complex, line stride p) and one sweep per
// row in place through LDS -- forward: sub-rows, then combine + real split; inverse: merge + inverse combine, then sub-rows
void Fft3::z_sublines(double* data, long nrows, int ncomp, long comp_stride, bool fwd) {
  const int M = g_.nz / 2, p = route_[2].p, m = route_[2].m;
  if (fwd && (size_t)(M + 1) * sizeof(cplx) > kSubLdsMax) throw std::runtime_error("fft: z length too large for the sub-line path");
  auto subs = [&]() {
    strided_pow2_narrow(m, strided_args(data, 2, 1.0, 0), (int)nrows, fwd ? -1 : +1, ncomp, comp_stride / 2, stream_);
  };
  auto sweep = [&]() {
    for (int c = 0; c < ncomp; ++c) {
      dispatch_p<3, 5, 7, 9, 15, 25, 0>(p, [&](auto P) {
        if (fwd) launch_z_sweep<true, decltype(P)::value>(data + c * comp_stride, nrows, g_.nzp, M, p, wgen_[2], stream_);
        else launch_z_sweep<false, decltype(P)::value>(data + c * comp_stride, nrows, g_.nzp, M, p, wgen_[2], stream_);
      });
      FG_HIP_CHECK(hipGetLastError());
    }
  };
  if (fwd) subs(), sweep();
  else sweep(), subs();
}

void Fft3::forward(double* data, int ncomp, long comp_stride, double scale) {
  r2c_z(data, ncomp, comp_stride);
  // fold the scale into the last pass that actually runs
  const bool has_x = g_.nx > 1, has_y = g_.ny > 1;
  c2c_y(data, ncomp, comp_stride, -1, (has_x || !has_y) ? 1.0 : scale);
  c2c_x(data, ncomp, comp_stride, -1, has_x ? scale : 1.0);
  if (!has_x && !has_y && scale != 1.0) this->scale(data, ncomp, comp_stride, scale);
}

// explicit scaling sweep (only for 1-D problems along z, where no strided pass can carry the factor)
void Fft3::scale(double* data, int ncomp, long comp_stride, double scale) {
  const int bs = 256;
  for (int c = 0; c < ncomp; ++c) {
    hipLaunchKernelGGL(k_scale, dim3((unsigned)((g_.n + bs - 1) / bs)), dim3(bs), 0, stream_, data + c * comp_stride, g_.n,
                       scale);
    FG_HIP_CHECK(hipGetLastError());
  }
}

void Fft3::inverse(double* data, int ncomp, long comp_stride) {
  c2c_x(data, ncomp, comp_stride, +1, 1.0);
  c2c_y(data, ncomp, comp_stride, +1, 1.0);
  c2r_z(data, ncomp, comp_stride);
}

}  // namespace fg

