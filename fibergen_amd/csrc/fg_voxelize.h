// The voxeliser in two parts (fg_voxelize.hip): shape parsing on the host, the per-material voxelisation on the device.
// fg_voxelize is "device part + copy out"; Solver::voxelize_into keeps the result on the device and normalises it there.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/fibergen_amd.h"

namespace fg {

// makes `device` current for a scope and gives the caller's current device back on the way out
class DeviceScope {
 public:
  explicit DeviceScope(int device);
  ~DeviceScope();
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;

 private:
  int prev_ = -1;
};

class Voxelizer {
 public:
  // host part: fg_fiber -> shapes; throws std::runtime_error with fg_voxelize's messages (material out of range, zero
  // normal, capsule without orientation, unknown kind)
  Voxelizer(const fg_fiber* fibers, int nfibers, int nphases);
  ~Voxelizer();
  Voxelizer(const Voxelizer&) = delete;
  Voxelizer& operator=(const Voxelizer&) = delete;

  int num_shapes() const;
  void real_volume(double* out /* [nphases] */) const;   // analytic volume per phase (infinite with a half space)

  // device part, on the CURRENT device; every copy, memset and kernel goes to `stream`.
  // begin: the cell (nx, ny, nz voxels of a box of dx x dy x dz at x0) and the buffers all materials share
  void begin(int nx, int ny, int nz, double dx, double dy, double dz, const double* x0, hipStream_t stream);
  // material m -> d_phi, dense [nx][ny][nz], before normalizePhi: brick candidate lists (host), k_vox_classify, k_vox_refine*.
  // Returns once the stream has drained (the host reads the number of interface voxels).
  void material(int m, int smooth_levels, double smooth_tol, double* d_phi);
  // throws if a refinement ran past 20 levels in any material() since begin (waits for the stream)
  void check_refinement();
  // interface normals on (nx, ny, nz) voxels of begin's box (the fine form samples them on the solver's own grid): component c
  // of voxel (i, j, k) -> d_normals[c * comp_stride + (i * ny + j) * row_pitch + k]; after begin, needs num_shapes() > 0
  void normals(int nx, int ny, int nz, double* d_normals, long row_pitch, long comp_stride);

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// normalizePhi (F:17588-17646) on the device, one thread per voxel of `nvox` voxels in rows of nz: walking the materials from
// last to first each takes min(remaining, phi_m), the matrix material entering as the constant 1 (in[matrix_mat] is not read).
// in[m] is dense [..][nz]; out[m] has rows of row_pitch doubles, whose cells past nz are not written.  out[m] == in[m] with
// row_pitch == nz normalises in place.  Only min and subtraction, in the host's order: bit-identical to fg.py's _normalize_phi.
void launch_vox_normalize(const double* const* in, double* const* out, int nphases, int matrix_mat, long nvox, int nz,
                          long row_pitch, hipStream_t stream);

}  // namespace fg
