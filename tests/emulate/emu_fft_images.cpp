// Host emulation of the strided pass with ONE exchange plane (StridedKernel<N, C, DIR, 1>, i.e. Line<N, 1>): every phase
// for all threads of a block in turn, which is what the device does between two barriers.  The plane starts as NaN, so a
// gather that runs before its scatter shows; a missing barrier does not (the GPU test compares the two forms bit for bit).
#include <cmath>
#include <vector>

#include "../../fibergen_amd/csrc/fg_fft_kernels.h"
#include "../../fibergen_amd/csrc/fg_fft_tables.h"

using namespace fg;
using namespace fg::fft;

template <class K, int PH>
struct PhaseLoop {
  static void run(std::vector<typename K::Regs>& regs, int block, double* lds, const StridedArgs& a) {
    for (int tid = 0; tid < K::THREADS; ++tid) K::template phase<PH>(regs[tid], block, tid, lds, a);
    if constexpr (PH + 1 < K::NPHASE) PhaseLoop<K, PH + 1>::run(regs, block, lds, a);
  }
};

template <class K>
static void run_blocks(long nblocks, const StridedArgs& a) {
  std::vector<typename K::Regs> regs(K::THREADS);
  std::vector<double> lds(K::LDS_DOUBLES);
  for (long b = 0; b < nblocks; ++b) {
    for (auto& x : lds) x = NAN;
    PhaseLoop<K, 0>::run(regs, (int)b, lds.data(), a);
  }
}

template <int N, int C, int IMAGES>
static void strided_dir(const StridedArgs& a, long nblocks, int dir) {
  if (dir < 0) run_blocks<StridedKernel<N, C, -1, IMAGES>>(nblocks, a);
  else run_blocks<StridedKernel<N, C, +1, IMAGES>>(nblocks, a);
}

extern "C" {

// c2c along the strided axis of data[nouter][N][ncols], device tile geometry; images = 1 | 2.  LDS doubles of the kernel in
// *lds_doubles.  Returns 1 for a length without a kernel.
int emu_strided_images(int N, int dir, double* data, int ncols, int nouter, double scale, int images, int* lds_doubles) {
  std::vector<cplx> tw = make_pass_twiddles(N);
  StridedArgs a;
  a.nt = 0;
  a.xcd_order = 0;
  a.data = reinterpret_cast<cplx*>(data);
  a.ls = ncols;
  a.os = (long)N * ncols;
  a.ncols = ncols;
  a.scale = scale;
  a.tw = tw.data();
#define CASE(n)                                                                           \
  if (N == n) {                                                                           \
    constexpr int C = TileCols<n>::value;                                                 \
    a.tiles_per_outer = (ncols + C - 1) / C;                                              \
    const long nb = (long)a.tiles_per_outer * nouter;                                     \
    if (images == 1) strided_dir<n, C, 1>(a, nb, dir), *lds_doubles = StridedKernel<n, C, -1, 1>::LDS_DOUBLES; \
    else strided_dir<n, C, 2>(a, nb, dir), *lds_doubles = StridedKernel<n, C, -1, 2>::LDS_DOUBLES;             \
    return 0;                                                                             \
  }
  CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
  return 1;
}

}  // extern "C"
