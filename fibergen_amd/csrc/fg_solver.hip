#include "fg_solver.h"
#include "fg_voxelize.h"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

#include "fg_hip_util.h"
#include "fg_slab.h"
#include "fg_willot_math.h"

namespace fg {

using namespace hostmath;

using namespace slots;

namespace {
constexpr double kEps = 2.220446049250313e-16;

// The stop rule's hand-over to the host: the reduced sums (a block of dscal_) and the error flag are written straight into
// pinned host memory, followed by a sequence number the host spins on -- one tiny kernel instead of two or three small
// copies and an event wait (128^3: 0.37 -> 0.2x ms per pass of fg_run_load_case, the copies sat on the stream's critical path).
__global__ void k_publish(const double* dsc, int n, const double* dsc2, int n2, const int* derr, double* hsc, double* hsc2,
                          int* herr, volatile unsigned* hseq, unsigned seq) {
  const int t = threadIdx.x;
  if (t < n) hsc[t] = dsc[t];
  if (t < n2) hsc2[t] = dsc2[t];
  if (t == 0) *herr = *derr;
  __threadfence_system();
  __syncthreads();
  if (t == 0) *hseq = seq;
}

// Viscosity mode with mixed boundary conditions: DeltaOperatorStaggered F:20422-20460 hands adj = E - 2 alpha m <tau> to
// GammaOperatorStaggered, whose applyBCProjector (F:20263-20270, bc_relax = 1) adds alpha MQ:<tau> at the end.  The tail sweep
// forms  adj_c = E_c - coef * sums_c / N  from the six sums the divergence sweep left on the device (coef = 2 alpha m); this
// kernel replaces the sums by  s - (alpha / coef) B s,  B the plain 6 x 6 matrix of v -> MQ:v, so that the sweep's adj carries
// both terms -- no host round trip.
struct Mat36 {
  double a[36];
};
__global__ void k_bc_adjust_sums(double* sums, Mat36 B, double factor) {
  if (threadIdx.x != 0) return;
  double s[6], o[6];
  for (int c = 0; c < 6; ++c) s[c] = sums[c];
  for (int c = 0; c < 6; ++c) {
    double t = 0.0;
    for (int j = 0; j < 6; ++j) t += B.a[c * 6 + j] * s[j];
    o[c] = s[c] - factor * t;
  }
  for (int c = 0; c < 6; ++c) sums[c] = o[c];
}
}  // namespace

Solver::Solver(int nx, int ny, int nz, double dx, double dy, double dz, int device, int rank, int nranks, bool slab_layout,
               hipStream_t shared_stream)
    : slab_layout_(slab_layout), device_(device), rank_(rank), nranks_(nranks), nxg_(nx) {
  if (nx < 1 || ny < 1 || nz < 1) throw std::runtime_error("grid dimensions must be >= 1");
  if (!(dx > 0) || !(dy > 0) || !(dz > 0)) throw std::runtime_error("RVE dimensions must be > 0");
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("invalid rank / number of ranks");
  if (nranks > 1 && (nx % nranks != 0 || ny % nranks != 0))
    throw std::runtime_error("slab decomposition needs nx and ny divisible by the number of ranks");
  // x-slab: this rank owns planes [rank*nxl, (rank+1)*nxl) of every component; cell sizes stay global
  const int nxl = nx / nranks;
  nyl_ = ny / nranks;
  g_ = make_grid(nxl, ny, nz, dx, dy, dz);
  g_.hx = nx / dx;
  nglobal_ = (long)nx * ny * nz;
  if (g_.n >= (1L << 31)) throw std::runtime_error("grid too large: padded component exceeds 2^31 reals");
  int ndev = 0;
  FG_HIP_CHECK(hipGetDeviceCount(&ndev));
  if (ndev < 1) throw std::runtime_error("no HIP device available: fibergen_amd needs an AMD GPU (gfx950)");
  if (device < 0 || device >= ndev) throw std::runtime_error("invalid device index");
  FG_HIP_CHECK(hipSetDevice(device));
  try {   // a failure half way (out of memory at 512^3, say) must give everything back: the destructor will not run
  if (shared_stream) {
    stream_ = shared_stream;
    owns_stream_ = false;
  } else {
    FG_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  }
  comm_stream_ = stream_;
  FG_HIP_CHECK(hipEventCreate(&ev_[0]));
  FG_HIP_CHECK(hipEventCreate(&ev_[1]));
  FG_HIP_CHECK(hipEventCreateWithFlags(&ev_copy_, hipEventDisableTiming));
  pt_.n = 0;
  for (int i = 0; i < kMaxPhases; ++i) {
    pt_.mu[i] = pt_.lambda[i] = 0.0;
    pt_.law[i] = kLawIso;
    sc_law_[i] = kScLawIso;
    for (int c = 0; c < 6; ++c) sc_K_[i][c] = 0.0;
    for (int k = 0; k < 36; ++k) pt_.C[i][k] = 0.0;
  }
  opt_.mu_0 = std::numeric_limits<double>::quiet_NaN();  // F:15340
  opt_.eps_a = std::pow(kEps, 2.0 / 3.0);

  const size_t comp = g_.n * sizeof(double);
  FG_HIP_CHECK(hipMalloc(&eps_, 6 * comp));
  FG_HIP_CHECK(hipMalloc(&tau_, 6 * comp));
  FG_HIP_CHECK(hipMalloc(&fu_, 3 * comp));
  FG_HIP_CHECK(hipMalloc(&fu_alt_, 3 * comp));
  FG_HIP_CHECK(hipMemsetAsync(fu_alt_, 0, 3 * comp, stream_));
  FG_HIP_CHECK(hipMemsetAsync(eps_, 0, 6 * comp, stream_));
  FG_HIP_CHECK(hipMemsetAsync(tau_, 0, 6 * comp, stream_));
  FG_HIP_CHECK(hipMemsetAsync(fu_, 0, 3 * comp, stream_));
  {
    const long rows = std::max<long>(partial_rows(g_), kMaxReduceBlocks);
    FG_HIP_CHECK(hipMalloc(&partial_, (size_t)rows * 8 * sizeof(double)));
  }
  FG_HIP_CHECK(hipMalloc(&dscal_, kNumSlots * sizeof(double)));
  FG_HIP_CHECK(hipHostMalloc(&hscal_, kNumSlots * sizeof(double)));
  FG_HIP_CHECK(hipMalloc(&derr_, 2 * sizeof(int)));   // [0] kernel error flag, [1] scratch of two_phase_complementary
  FG_HIP_CHECK(hipHostMalloc(&herr_, 2 * sizeof(int)));   // [0] error flag, [1] sequence number of k_publish
  herr_[1] = 0;
  hseq_ = reinterpret_cast<unsigned*>(herr_ + 1);
  FG_HIP_CHECK(hipMemsetAsync(derr_, 0, sizeof(int), stream_));
  // fields of this size come back through the staged pipeline: its pinned buffers (a one-time cost of the process, ~18 ms)
  // are allocated here rather than inside the first fg_get_field
  if (staged_copy(6 * comp, true)) (void)HostStager::of_device(device_);

  fft_.reset(new Fft3(g_, stream_));
  fft_->set_images(opt_.fft_images);
  if (slab_layout_) {   // halo planes of the strain-state pipeline of the slab driver (tau going out, tau coming in)
    const size_t plane = (size_t)g_.nyzp * sizeof(double);
    for (int k = 0; k < 4; ++k) {
      FG_HIP_CHECK(hipMalloc(&halo_[k], 2 * plane));
      FG_HIP_CHECK(hipMemsetAsync(halo_[k], 0, 2 * plane, stream_));
    }
  }

  // Separable factors of G0OperatorFourierStaggeredGeneral  F:19838-19876, evaluated on the
  // host with the same libm calls the reference makes per frequency.
  const int len[3] = {nxg_, ny, nz};
  const double d[3] = {dx, dy, dz};
  for (int a = 0; a < 3; ++a) {
    const int n = len[a];
    const int cnt = (a == 2) ? g_.nzc : n;
    std::vector<double> kpm(cnt);
    std::vector<cplx> kp(cnt);
    const double h = d[a] / (2 * n);
    const double xi_0 = 2 * M_PI * h / d[a];
    const bool even = (n & 1) == 0;
    const size_t half = even ? (size_t)(n / 2 - 1) : (size_t)(n / 2);
    for (size_t i = 0; i < (size_t)cnt; ++i) {
      const double xi = xi_0 * ((i <= half) ? (double)i : ((double)i - (double)n));
      const double s = std::sin(xi) / h;
      const std::complex<double> z = s * std::exp(std::complex<double>(0, xi));
      kpm[i] = s;
      kp[i] = cmake(z.real(), z.imag());
    }
    FG_HIP_CHECK(hipMalloc(&g0_kpm_[a], cnt * sizeof(double)));
    FG_HIP_CHECK(hipMalloc(&g0_kp_[a], cnt * sizeof(cplx)));
    FG_HIP_CHECK(hipMemcpy(g0_kpm_[a], kpm.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    FG_HIP_CHECK(hipMemcpy(g0_kp_[a], kp.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice));
    // GammaOperatorFourierCollocated  F:19385, 19411-19424: xi = (1/d) * signed index
    std::vector<double> xi(cnt);
    const double xi_c0 = 1 / d[a];
    for (size_t i = 0; i < (size_t)cnt; ++i) xi[i] = xi_c0 * ((i <= half) ? (double)i : ((double)i - (double)n));
    FG_HIP_CHECK(hipMalloc(&xi_[a], cnt * sizeof(double)));
    FG_HIP_CHECK(hipMemcpy(xi_[a], xi.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
  }

  BC_P_ = voigt_id4();
  for (int i = 0; i < 6; ++i) F00_[i] = 0.0, sumsq_[i] = 0.0;
  recompute_bc();
  reset_stage_times();
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  } catch (...) {
    release();
    throw;
  }
}

Solver::~Solver() {
  (void)hipSetDevice(device_);
  if (group_) group_->invalidate();
  release();
}

// frees every device / host resource the object holds (idempotent; also the constructor's failure path)
void Solver::release() {
  if (!stream_) return;
  (void)hipStreamSynchronize(stream_);
  if (comm_stream_ && comm_stream_ != stream_) (void)hipStreamSynchronize(comm_stream_);
  fft_.reset();
  for (int k = 0; k < 4; ++k)
    if (halo_[k]) (void)hipFree(halo_[k]);
  for (void* p : {(void*)lam_phic_, (void*)lam_nrmc_, (void*)lam_epsc_})
    if (p) (void)hipFree(p);
  if (mixed_list_) (void)hipFree(mixed_list_);
  if (aff_list_) (void)hipFree(aff_list_);
  if (aff_slots_) (void)hipFree(aff_slots_);
  if (dtau_) (void)hipFree(dtau_);
  double* bufs[] = {eps_, tau_, fu_, fu_alt_, phi_, normals_, partial_, dscal_, cg_r_, cg_p_, cg_w_, mod_, fu_cg_, phis_, mod5_};
  for (double* b : bufs)
    if (b) (void)hipFree(b);
  if (hscal_) (void)hipHostFree(hscal_);
  if (derr_) (void)hipFree(derr_);
  if (herr_) (void)hipHostFree(herr_);
  for (int a = 0; a < 3; ++a) {
    if (g0_kpm_[a]) (void)hipFree(g0_kpm_[a]);
    if (g0_kp_[a]) (void)hipFree(g0_kp_[a]);
    if (xi_[a]) (void)hipFree(xi_[a]);
    if (wil_t_[a]) (void)hipFree(wil_t_[a]);
    if (wil_e_[a]) (void)hipFree(wil_e_[a]);
    if (poi_cs_[a]) (void)hipFree(poi_cs_[a]);
  }
  for (hipEvent_t e : {ev_[0], ev_[1], ev_copy_})
    if (e) (void)hipEventDestroy(e);
  if (aux_stream_) {
    (void)hipStreamSynchronize(aux_stream_);
    (void)hipStreamDestroy(aux_stream_);
    (void)hipEventDestroy(ev_fork_);
    (void)hipEventDestroy(ev_join_);
  }
  comm_.reset();
  fft_ys_.reset();
  for (double* b : {su_[0], su_[1], smod_, scg_, scg2_, su_alt_})
    if (b) (void)hipFree(b);
  if (ev_c2x_) (void)hipEventDestroy(ev_c2x_);
  if (ev_norm_) (void)hipEventDestroy(ev_norm_);
  for (hipEvent_t e : ev_ct_)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_x_)
    if (e) (void)hipEventDestroy(e);
  if (owns_comm_stream_ && comm_stream_) (void)hipStreamDestroy(comm_stream_);
  if (owns_stream_) (void)hipStreamDestroy(stream_);
  stream_ = comm_stream_ = nullptr;
}

// ------------------------------------------------------------------ configuration
void Solver::set_num_phases(int n) {
  if (n < 1 || n > kMaxPhases) throw std::runtime_error("number of phases must be in [1, 8]");
  polar_settle();
  FG_HIP_CHECK(hipSetDevice(device_));
  if (phi_) FG_HIP_CHECK(hipFree(phi_));
  phi_ = nullptr;
  FG_HIP_CHECK(hipMalloc(&phi_, (size_t)n * g_.n * sizeof(double)));
  FG_HIP_CHECK(hipMemsetAsync(phi_, 0, (size_t)n * g_.n * sizeof(double), stream_));
  if (phis_) FG_HIP_CHECK(hipFree(phis_));
  phis_ = nullptr;
  fine_set_ = 0;
  pt_.n = n;
  for (int p = 0; p < kMaxPhases; ++p) {   // a fresh set of phases: no general / aniso phase outlives it (their mu = NaN goes too)
    if (pt_.law[p] != kLawIso || sc_law_[p] != kScLawIso) pt_.mu[p] = pt_.lambda[p] = 0.0;
    pt_.law[p] = kLawIso;
    sc_law_[p] = kScLawIso;
  }
  mod_dirty_ = mod5_dirty_ = true;
  smod_dirty_ = mod5_dirty_ = true;
  complement_dirty_ = true;
  mixed_dirty_ = true;
}

void Solver::set_phase_material(int p, double mu, double lambda) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  polar_settle();
  mod_dirty_ = mod5_dirty_ = true;
  smod_dirty_ = mod5_dirty_ = true;
  complement_dirty_ = true;
  mixed_dirty_ = true;
  pt_.mu[p] = mu;
  pt_.lambda[p] = lambda;
  pt_.law[p] = kLawIso;
  sc_law_[p] = kScLawIso;
}

void Solver::set_phase_stiffness(int p, const double* C36) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  if (!C36) throw std::runtime_error("stiffness pointer is NULL");
  if (nranks_ != 1 || slab_layout_) throw std::runtime_error(plan::kGeneralSlab);
  double cmax = 0.0;
  for (int i = 0; i < 36; ++i) {
    if (!std::isfinite(C36[i])) throw std::runtime_error("phase stiffness is not finite");
    cmax = std::max(cmax, std::fabs(C36[i]));
  }
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j)
      if (std::fabs(C36[6 * i + j] - C36[6 * j + i]) > 1e-12 * cmax) throw std::runtime_error("phase stiffness is not symmetric");
  polar_settle();
  invalidate_moduli();
  mixed_dirty_ = true;
  for (int i = 0; i < 36; ++i) pt_.C[p][i] = C36[i];
  pt_.law[p] = kLawGeneral;
  sc_law_[p] = kScLawIso;
  // the safety net: whatever still reads (mu, lambda) of a general phase computes NaN, not an isotropic answer
  pt_.mu[p] = pt_.lambda[p] = std::numeric_limits<double>::quiet_NaN();
}

// law "aniso" of the scalar modes (MatrixLinearAnisotropicMaterialLaw  F:11087-11156): c11 c22 c33 c23 c13 c12
void Solver::set_phase_conductivity(int p, const double* c6) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  if (!c6) throw std::runtime_error("conductivity pointer is NULL");
  if (opt_.mode != 1) throw std::runtime_error(plan::kAnisoMode);
  if (nranks_ != 1 || slab_layout_) throw std::runtime_error(plan::kAnisoSlab);
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(c6[i])) throw std::runtime_error("phase conductivity is not finite");
  invalidate_moduli();
  for (int i = 0; i < 6; ++i) sc_K_[p][i] = c6[i];
  sc_law_[p] = kScLawAniso;
  pt_.law[p] = kLawIso;
  // the convention of general phases: whatever still reads mu of an aniso phase computes NaN, not an isotropic answer
  pt_.mu[p] = pt_.lambda[p] = std::numeric_limits<double>::quiet_NaN();
}

bool Solver::aniso_phase() const {
  bool a = false;
  for (int p = 0; p < pt_.n; ++p) a = a || sc_law_[p] != kScLawIso;
  return a;
}

void Solver::set_phase_field(int p, const double* phi_host) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  polar_settle();
  mod_dirty_ = mod5_dirty_ = true;
  smod_dirty_ = mod5_dirty_ = true;
  complement_dirty_ = true;
  mixed_dirty_ = true;
  fine_set_ &= ~(1u << p);
  ++phase_uploads_;
  upload_padded(phi_ + (long)p * g_.n, phi_host);
}

void Solver::set_phase_field_fine(int p, const double* fine_host) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  if (willot()) throw std::runtime_error("gamma_scheme willot takes phase fields on the solver's grid (a fine phase field needs full_staggered)");
  if (!dfg()) throw std::runtime_error("a phase field on the doubly fine grid needs gamma_scheme full_staggered (2)");
  if (nranks_ != 1 || slab_layout_) throw std::runtime_error(plan::kDfgSlab);
  FG_HIP_CHECK(hipSetDevice(device_));
  ++phase_uploads_;
  const size_t nfine = 8 * (size_t)g_.nxyz;
  if (!phis_) {
    FG_HIP_CHECK(hipMalloc(&phis_, 3 * (size_t)pt_.n * g_.n * sizeof(double)));
    FG_HIP_CHECK(hipMemsetAsync(phis_, 0, 3 * (size_t)pt_.n * g_.n * sizeof(double), stream_));
  }
  double* fine = nullptr;
  FG_HIP_CHECK(hipMalloc(&fine, nfine * sizeof(double)));
  FG_HIP_CHECK(hipMemcpyAsync(fine, fine_host, nfine * sizeof(double), hipMemcpyHostToDevice, stream_));
  FieldPtrs<3> s;
  for (int c = 0; c < 3; ++c) s.p[c] = phis_ + (3L * p + c) * g_.n;
  launch_dfg_fractions_fine(g_, fine, phi_ + (long)p * g_.n, s, stream_);
  FG_HIP_CHECK(hipStreamSynchronize(stream_));   // the caller's image may go once this returns; ours goes now
  FG_HIP_CHECK(hipFree(fine));
  mod_dirty_ = mod5_dirty_ = true;
  smod_dirty_ = complement_dirty_ = mixed_dirty_ = true;
  fine_set_ |= 1u << p;
}

void Solver::set_normals(const double* n_host) {
  FG_HIP_CHECK(hipSetDevice(device_));
  mixed_dirty_ = true;   // the interface lists carry compact copies of the normals
  ++phase_uploads_;
  if (!normals_) {
    FG_HIP_CHECK(hipMalloc(&normals_, 3 * g_.n * sizeof(double)));
    FG_HIP_CHECK(hipMemsetAsync(normals_, 0, 3 * g_.n * sizeof(double), stream_));
  }
  upload_padded(normals_, n_host, 3, g_.n);
}

namespace {
struct DeviceDoubles {   // scratch images of voxelize_into
  std::vector<double*> p;
  ~DeviceDoubles() {
    for (double* q : p)
      if (q) (void)hipFree(q);
  }
  double* alloc(size_t n) {
    double* q = nullptr;
    FG_HIP_CHECK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(double)));
    p.push_back(q);
    return q;
  }
};
}  // namespace

void Solver::voxelize_into(const fg_fiber* fibers, int nfibers, const double* x0, int matrix_mat, int smooth_levels,
                           double smooth_tol, int flags, double* real_volume) {
  const bool fine = (flags & FG_VOX_FINE) != 0, want_normals = (flags & FG_VOX_NORMALS) != 0;
  const int nph = pt_.n;
  if (nph < 1 || !x0 || nfibers < 0 || !phi_) throw std::runtime_error("fg_voxelize: bad arguments");
  if (nranks_ != 1 || slab_layout_) throw std::runtime_error("fg_voxelize_into is not available on slab-decomposed solvers");
  if (fine) {
    if (willot()) throw std::runtime_error("gamma_scheme willot takes phase fields on the solver's grid (a fine phase field needs full_staggered)");
    if (!dfg()) throw std::runtime_error("a phase field on the doubly fine grid needs gamma_scheme full_staggered (2)");
  }
  DeviceScope scope(device_);
  Voxelizer vox(fibers, nfibers, nph);   // host part: the argument errors come before anything changes
  if (real_volume) vox.real_volume(real_volume);
  const int f = fine ? 2 : 1;
  const int vx = f * g_.nx, vy = f * g_.ny, vz = f * g_.nz;
  const size_t nvox = (size_t)vx * vy * vz;
  vox.begin(vx, vy, vz, g_.dx, g_.dy, g_.dz, x0, stream_);
  // dense images before normalizePhi; the matrix enters as the constant 1 and needs one only where its normalised image
  // is read again (the reduction of the fine form)
  DeviceDoubles scratch;
  const double* in[kMaxPhases] = {};
  double* out[kMaxPhases] = {};
  for (int m = 0; m < nph; ++m) {
    double* img = (m != matrix_mat || fine) ? scratch.alloc(nvox) : nullptr;
    in[m] = img;
    out[m] = fine ? img : phi_ + (long)m * g_.n;
    if (m != matrix_mat) vox.material(m, smooth_levels, smooth_tol, img);
  }
  vox.check_refinement();

  mod_dirty_ = mod5_dirty_ = true;
  smod_dirty_ = complement_dirty_ = mixed_dirty_ = true;
  if (!fine) {
    launch_vox_normalize(in, out, nph, matrix_mat, (long)nvox, g_.nz, g_.nzp, stream_);
    fine_set_ = 0;
  } else {
    if (!phis_) {
      FG_HIP_CHECK(hipMalloc(&phis_, 3 * (size_t)nph * g_.n * sizeof(double)));
      FG_HIP_CHECK(hipMemsetAsync(phis_, 0, 3 * (size_t)nph * g_.n * sizeof(double), stream_));
    }
    launch_vox_normalize(in, out, nph, matrix_mat, (long)nvox, vz, vz, stream_);   // in place
    for (int p = 0; p < nph; ++p) {
      FieldPtrs<3> s;
      for (int c = 0; c < 3; ++c) s.p[c] = phis_ + (3L * p + c) * g_.n;
      launch_dfg_fractions_fine(g_, out[p], phi_ + (long)p * g_.n, s, stream_);
      fine_set_ |= 1u << p;
    }
  }
  if (want_normals) {   // always on the solver's own grid
    if (!normals_) {
      FG_HIP_CHECK(hipMalloc(&normals_, 3 * g_.n * sizeof(double)));
      FG_HIP_CHECK(hipMemsetAsync(normals_, 0, 3 * g_.n * sizeof(double), stream_));
    }
    if (vox.num_shapes() == 0) {
      FG_HIP_CHECK(hipMemsetAsync(normals_, 0, 3 * g_.n * sizeof(double), stream_));
    } else {
      vox.normals(g_.nx, g_.ny, g_.nz, normals_, g_.nzp, g_.n);
    }
  }
  FG_HIP_CHECK(hipStreamSynchronize(stream_));   // the scratch images go now
}

void Solver::set_bc_projector(const double* P36) {
  // setBCProjector checks  F:20601-20615
  Mat6 P;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) P.a[i][j] = P36[i * 6 + j];
  const double se = std::sqrt(kEps);
  Mat6 D = P;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) D.a[i][j] = P.a[i][j] - P.a[j][i];
  if (frobenius(D) > se) throw std::runtime_error("Projector is not symmetric");
  Mat6 PP = voigt_mm(P, P);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) D.a[i][j] = P.a[i][j] - PP.a[i][j];
  if (frobenius(D) > se) throw std::runtime_error("Specified Projector is not a projector");
  BC_P_ = P;
  recompute_bc();
}

// setBCProjector body  F:20617-20664 (depends on the current reference material)
void Solver::recompute_bc() {
  const Mat6 Id = voigt_id4(), II = voigt_ii4();
  bool q_zero = true;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      BC_Q_.a[i][j] = Id.a[i][j] - BC_P_.a[i][j];
      if (BC_Q_.a[i][j] != 0.0) q_zero = false;
    }
  if (q_zero) {  // pure strain BC: Q:C0, M, MQ vanish whatever C0 is (also while mu_0 is NaN)
    BC_QC0_ = BC_M_ = BC_MQ_ = mat6_zero();
    return;
  }
  Mat6 C0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) C0.a[i][j] = 2 * opt_.mu_0 * Id.a[i][j] + opt_.lambda_0 * II.a[i][j];
  BC_QC0_ = voigt_mm(BC_Q_, C0);
  if (std::isnan(opt_.mu_0)) {
    // run() calls setBCProjector before calcRefMaterial replaced the NaN (F:21354 vs F:21742);
    // the values are recomputed before their first use.
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) BC_M_.a[i][j] = BC_MQ_.a[i][j] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  BC_M_ = bc_pseudo_inverse(voigt_mm(BC_QC0_, BC_Q_));
  BC_MQ_ = voigt_mm(BC_M_, BC_Q_);
}

// ------------------------------------------------------------------ helpers
FieldPtrs<6> Solver::ptrs6(double* base) const {
  FieldPtrs<6> f;
  for (int c = 0; c < 6; ++c) f.p[c] = base + (long)c * g_.n;
  return f;
}
FieldPtrs<3> Solver::ptrs3(double* base) const {
  FieldPtrs<3> f;
  for (int c = 0; c < 3; ++c) f.p[c] = base + (long)c * g_.n;
  return f;
}

// mode = viscosity: ScalarLinearIsotropicMaterialLaw(6) with mu *= 0.5 (F:15234-15239), S = E * (alpha * mu / 2).
// The Hooke kernels give S = E * (2 alpha mu') + alpha lambda' tr(E): mu' = mu / 4, lambda' = 0 is the same
// arithmetic (scalings by powers of two are exact, the added zero changes nothing).
PhaseTable Solver::phase_table() const {
  PhaseTable t = pt_;
  if (opt_.mode == 2)
    for (int q = 0; q < kMaxPhases; ++q) t.mu[q] = 0.25 * pt_.mu[q], t.lambda[q] = 0.0;
  return t;
}

StressParams Solver::stress_params(double mu_0, double lambda_0, double alpha) const {
  StressParams sp;
  sp.pt = phase_table();
  sp.mixing = opt_.mixing;
  sp.mu_0 = mu_0;
  sp.lambda_0 = lambda_0;
  sp.alpha = alpha;
  sp.eps_g = opt_.eps_g;
  sp.eps_a = opt_.eps_a;
  return sp;
}

// Boundary transfers (GetField / SetField F:26931-27010 copy row by row): large fields go through the staged pipeline of
// fg_transfer.h (padding stripped / added on the device, whole chunks over the link, a team of host threads on the pageable
// side), small ones through one strided copy.
// Measured on the MI355X boxes (tools/transfer_probe.py, 805 MB): uploads from pageable memory already run at the link's
// rate through the runtime's own staging (54 GB/s), downloads into FRESH pageable memory do not (48 ms: the page faults of
// the destination are taken one by one by the copying thread) -- the pipeline takes them on its team of host threads while
// the next chunks are on the link: 18-19 ms (14.2 ms into memory that is already mapped, either way).
bool Solver::staged_copy(size_t bytes, bool download) const {
  return opt_.staged_copy > 0 || (opt_.staged_copy < 0 && download && bytes >= (size_t)8 << 20);
}

void Solver::upload_rows(const std::vector<RowBlock>& blocks, long len, long pitch) {
  FG_HIP_CHECK(hipSetDevice(device_));
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  size_t bytes = 0;
  for (const RowBlock& b : blocks) bytes += (size_t)b.nrows * len * sizeof(double);
  if (staged_copy(bytes, false)) {
    HostStager::of_device(device_).upload(blocks, len, pitch, (size_t)std::max(1, opt_.stage_chunk_kb) << 10);
    return;
  }
  for (const RowBlock& b : blocks)
    FG_HIP_CHECK(hipMemcpy2D(b.dev, pitch * sizeof(double), b.host, len * sizeof(double), len * sizeof(double), (size_t)b.nrows,
                             hipMemcpyHostToDevice));
}

void Solver::download_rows(const std::vector<RowBlock>& blocks, long len, long pitch) {
  FG_HIP_CHECK(hipSetDevice(device_));
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  size_t bytes = 0;
  for (const RowBlock& b : blocks) bytes += (size_t)b.nrows * len * sizeof(double);
  if (staged_copy(bytes, true)) {
    HostStager::of_device(device_).download(blocks, len, pitch, (size_t)std::max(1, opt_.stage_chunk_kb) << 10);
    return;
  }
  for (const RowBlock& b : blocks)
    FG_HIP_CHECK(hipMemcpy2D(b.host, len * sizeof(double), b.dev, pitch * sizeof(double), len * sizeof(double), (size_t)b.nrows,
                             hipMemcpyDeviceToHost));
}

// nc padded components [nx][ny][nzp], `dstride` doubles apart on the device <-> nc unpadded host components
void Solver::upload_padded(double* dst, const double* src, int nc, long dstride) {
  std::vector<RowBlock> blocks;
  for (int c = 0; c < nc; ++c)
    blocks.push_back(RowBlock{dst + (long)c * dstride, const_cast<double*>(src) + (long)c * g_.nxyz, (long)g_.nx * g_.ny});
  upload_rows(blocks, g_.nz, g_.nzp);
}

void Solver::download_unpadded(const double* src, double* dst, int nc, long dstride) {
  std::vector<RowBlock> blocks;
  for (int c = 0; c < nc; ++c)
    blocks.push_back(RowBlock{const_cast<double*>(src) + (long)c * dstride, dst + (long)c * g_.nxyz, (long)g_.nx * g_.ny});
  download_rows(blocks, g_.nz, g_.nzp);
}

void Solver::check_device_error(const char* where) {
  FG_HIP_CHECK(hipMemcpyAsync(herr_, derr_, sizeof(int), hipMemcpyDeviceToHost, stream_));
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  if (*herr_ != 0) {
    FG_HIP_CHECK(hipMemsetAsync(derr_, 0, sizeof(int), stream_));
    if (opt_.mixing == kMixLaminate)
      throw std::runtime_error(std::string("The laminate mixing rule supports only two phase mixtures (") + where + ")");
    throw std::runtime_error(std::string("device kernel reported an error (") + where + ")");
  }
}

// The same check, but the host waits only for the copies enqueued so far (an event), not for work enqueued after them.
void Solver::fetch_norms_and_errors(const char* where) {
  static_assert(kSlotMean == kSlotSumSq + 6, "the displacement sweep writes norms and tau sums as one block of 12");
  const bool mixed_u = pending_back_ && mixed_bc();
  const int nfetch = mixed_u ? 12 : 6;
  const int n2 = (mixed_u && opt_.mixing == kMixLaminate) ? 6 : 0;   // mixed BC + laminate: + sums of the interface differences
  {
    // one tiny kernel publishes sums + error flag + sequence number in pinned host memory; the host spins on the number
    const unsigned seq = ++publish_seq_;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, stream_, dscal_ + kSlotSumSq, nfetch, dscal_ + kSlotScratch, n2, derr_,
                       hscal_ + kSlotSumSq, hscal_ + kSlotScratch, herr_, hseq_, seq);
    FG_HIP_CHECK(hipGetLastError());
    if (pending_back_) launch_pending_back();   // speculative: u_{k+1} is built while the host looks at the norms of eps_k
    long spins = 0;
    while (__atomic_load_n(hseq_, __ATOMIC_ACQUIRE) != seq) {
      if (++spins > (1L << 22)) {   // a long pass (or a stuck device): fall back to a blocking wait once in a while
        FG_HIP_CHECK(hipStreamQuery(stream_) == hipErrorNotReady ? hipSuccess : hipStreamSynchronize(stream_));
        spins = 0;
      }
#if defined(__x86_64__)
      __builtin_ia32_pause();
#endif
    }
  }
  if (*herr_ != 0) {
    FG_HIP_CHECK(hipMemsetAsync(derr_, 0, sizeof(int), stream_));
    if (opt_.mixing == kMixLaminate)
      throw std::runtime_error(std::string("The laminate mixing rule supports only two phase mixtures (") + where + ")");
    throw std::runtime_error(std::string("device kernel reported an error (") + where + ")");
  }
}

// FFT / Green-operator chain of the displacement loop, enqueued without touching the host-side state: fu_alt_ then holds
// u_{k+1}; adopt_back() makes it the current state.  If the iteration stops first, it is simply never adopted.
void Solver::launch_pending_back() {
  fft_g0_chain(fu_alt_, -1.0, nullptr, opt_.mode == 0 ? tau_ : nullptr);   // tau_ is free in the displacement loop
  pending_back_ = false;
  back_ready_ = true;
}

void Solver::adopt_back() {
  if (!back_ready_) launch_pending_back();
  back_ready_ = false;
  double* t = fu_;
  fu_ = fu_alt_;
  fu_alt_ = t;
  u_valid_ = true;
  eps_stale_ = true;
  for (int c = 0; c < 6; ++c) E_cur_[c] = E_next_[c];
  if (timing_) times_.count++;
}

void Solver::enable_stage_timing(bool on) {
  if (on && !timing_) {
    reset_stage_times();   // a new measurement starts from zero
    // what a pair of events reads with NOTHING between them (the smallest of 16 pairs on the idle stream): every
    // measurement carries it on top of the kernel's duration, so it is subtracted (rocprofv3's kernel durations then agree)
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    double bias = 1e30;
    for (int i = 0; i < 16; ++i) {
      FG_HIP_CHECK(hipEventRecord(ev_[0], stream_));
      FG_HIP_CHECK(hipEventRecord(ev_[1], stream_));
      FG_HIP_CHECK(hipEventSynchronize(ev_[1]));
      float ms = 0.f;
      FG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
      if (ms < bias) bias = ms;
    }
    event_bias_ms_ = bias;
  }
  timing_ = on;
}
void Solver::apply_fft_images() {   // (the slab passes of fft_ys_ keep two planes)
  if (fft_) fft_->set_images(opt_.fft_images);
}
void Solver::apply_bluestein() {
  if (fft_) fft_->set_bluestein(opt_.bluestein != 0);
  if (fft_ys_) fft_ys_->set_bluestein(opt_.bluestein != 0);
}

long Solver::counter(const std::string& name) const {
  // how each axis is transformed (Fft3::path) and the padded length of its Bluestein pass; slab solvers transform x on the y-slab
  if (fft_ && (name.rfind("fft_path_", 0) == 0 || name.rfind("fft_bluestein_m_", 0) == 0) && !name.empty()) {
    const char c = name.back();
    const int axis = c == 'x' ? 0 : (c == 'y' ? 1 : (c == 'z' ? 2 : -1));
    const Fft3* f = axis == 0 && fft_ys_ ? fft_ys_.get() : fft_.get();
    if (axis >= 0 && name == std::string("fft_path_") + c) return f->path(axis);
    if (axis >= 0 && name == std::string("fft_bluestein_m_") + c) return f->bluestein_m(axis);
  }
  // lists held from an earlier geometry (mixed_dirty_) are not this geometry's: they are rebuilt before a pass uses them
  if (name == "interface_voxels") return mixed_dirty_ ? 0 : (long)mixed_n_;
  if (name == "affected_voxels") return mixed_dirty_ ? 0 : (long)aff_n_;
  if (name == "phase_uploads") return phase_uploads_;
  if (name == "complement_checks") return complement_checks_;
  if (name == "front_sweep") return front_sweep_;
  if (name == "cg_dir_sweep") return cg_dir_sweep_;
  if (name == "u_tile_aniso") return u_tile_aniso_;
  if (name == "u_tile_reuss") return u_tile_reuss_;
  if (name == "sc_tile_aniso") return sc_tile_aniso_;
  if (name == "polarization_generic_voxels") {   // left on the device by the last forward launch of k_polarize
    double v = 0.0;
    FG_HIP_CHECK(hipSetDevice(device_));
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    FG_HIP_CHECK(hipMemcpy(&v, dscal_ + kSlotPolar + 6, sizeof(double), hipMemcpyDeviceToHost));
    return (long)v;
  }
  if (name == "pair_chunk_planes") return (long)pair_chunk_planes();
  return -1;
}

void Solver::reset_stage_times() {
  for (int i = 0; i < kNumTimedKernels; ++i) times_.ms[i] = 0.0;
  for (int i = 0; i < 4; ++i) comm_ms_[i] = 0.0;
  times_.count = 0;
}
void Solver::time_begin(int) {
  if (timing_) FG_HIP_CHECK(hipEventRecord(ev_[0], stream_));
}
void Solver::time_end(int stage) {
  if (!timing_) return;
  FG_HIP_CHECK(hipEventRecord(ev_[1], stream_));
  FG_HIP_CHECK(hipEventSynchronize(ev_[1]));
  float ms = 0.f;
  FG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
  times_.ms[stage] += ms > event_bias_ms_ ? ms - event_bias_ms_ : 0.0;
}

// ------------------------------------------------------------------ one pass of the basic scheme
// basicScheme  F:20558-20578: the checks, the strain state and the mean of the operator's argument, then the operator of the
// mode and gamma_scheme; every operator ends in pass_done
void Solver::basic_scheme(const double* E6, double* src, double* dst) {
  if (!src) src = eps_;
  if (!dst) dst = eps_;
  require_plan(plan::Entry::Pass);

  ensure_eps();  // the displacement-based loop may have left the strain implicit
  if (opt_.bc_relax != 1.0) {  // F:20563-20565: mean of the operator's argument
    launch_sum6(g_, ptrs6(src), false, partial_, dscal_ + kSlotMean, stream_);
    fetch_mean6(F00_);
  }
  if (willot()) willot_scheme(E6, src, dst);
  else if (opt_.mode == 2) pass_viscosity(E6, src, dst);
  else if (opt_.gamma_scheme == 1) pass_collocated(E6, src, dst);
  else pass_staggered(E6, src, dst);
}

void Solver::pass_done(const double* E6, const double* dst, bool u_valid) {
  if (timing_) times_.count++;
  u_valid_ = u_valid;
  if (dst == eps_) eps_stale_ = false;
  for (int c = 0; c < 6; ++c) E_cur_[c] = E6[c];
}

void Solver::fetch_mean6(double* F0, bool spectrum) {
  if (spectrum) {   // the forward transform is scaled by 1/N: Re tau_hat(0) is the mean
    for (int c = 0; c < 6; ++c)
      FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotMean + c, tau_ + (long)c * g_.n, sizeof(double), hipMemcpyDeviceToHost, stream_));
  } else {
    FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotMean, dscal_ + kSlotMean, 6 * sizeof(double), hipMemcpyDeviceToHost, stream_));
  }
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  for (int c = 0; c < 6; ++c) F0[c] = spectrum ? hscal_[kSlotMean + c] : hscal_[kSlotMean + c] / (double)nglobal_;
}

void Solver::bc_adjust_sums(double factor) {
  Mat36 B;
  for (int j = 0; j < 6; ++j) {
    double e[6] = {0, 0, 0, 0, 0, 0}, col[6];
    e[j] = 1.0;
    voigt_mv(BC_MQ_, e, col);
    for (int c = 0; c < 6; ++c) B.a[c * 6 + j] = col[c];
  }
  hipLaunchKernelGGL(k_bc_adjust_sums, dim3(1), dim3(64), 0, stream_, dscal_ + kSlotMean, B, factor);
  FG_HIP_CHECK(hipGetLastError());
}

// DeltaOperatorStaggered  F:20422-20460 (dual Stokes scheme), called with alpha = -1 by basicScheme:
//   m = 1/(4 mu0);  adj = E - 2 alpha m <tau>;  eta = GammaStaggered(adj; mu = -1/(4 m), lambda = inf)(tau)
//   + 2 alpha m tau.   lambda0 = inf makes c20 = c10 in G0OperatorFourierStaggered (F:19749-19755).
void Solver::pass_viscosity(const double* E6, double* src, double* dst) {
  const double alpha = -1.0;  // GammaOperator(..., -1)  F:20575
  const double m = 1 / (4 * opt_.mu_0);
  const StressParams sp = stress_params(opt_.mu_0, opt_.lambda_0, 1.0);
  // full_staggered: the fused form exists as the tiled sweep only (other grids store the polarisation)
  // (Reuss mixing: the fused forms re-evaluate the Voigt rule from the phase fractions in their tail sweep -- the stored form)
  const plan::Viscosity form = sweep_plan(0).viscosity;
  const bool fused = form != plan::Viscosity::Stored;
  // fused: the polarisation is a point-wise function of the strain: it is evaluated inside the divergence sweep (with its
  // six sums) and again in the tail sweep, and never stored
  time_begin(0);
  switch (form) {
    case plan::Viscosity::TileDfg:
      launch_eps_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs6(src), dfg_moduli(), ptrs3(fu_), partial_, dscal_ + kSlotMean, stream_);
      break;
    case plan::Viscosity::Tile:   // fast kernels allowed: the LDS-tiled marching form
      launch_eps_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs6(src), effective_moduli(), ptrs3(fu_), partial_, dscal_ + kSlotMean, stream_);
      break;
    case plan::Viscosity::FusedVoigt:
      launch_stress_div_sum_voigt(g_, sp, ptrs6(src), phase_ptrs(), ptrs3(fu_), partial_, dscal_ + kSlotMean, stream_);
      break;
    case plan::Viscosity::Stored:
      stress_to_tau(sp, src);
      time_end(0);
      launch_sum6(g_, ptrs6(tau_), false, partial_, dscal_ + kSlotMean, stream_);   // tau_copy->average(), stays on the device
      time_begin(1);
      launch_div(g_, ptrs6(tau_), ptrs3(fu_), kNoXHalo, stream_);
      break;
  }
  time_end(fused ? 0 : 1);
  // initBCProjector / applyBCProjector inside GammaOperatorStaggered (k_bc_adjust_sums has the algebra)
  if (mixed_bc()) bc_adjust_sums(alpha / (2 * alpha * m));
  const double mu_g = -1.0 / (4 * m);
  const double c12[2] = {-alpha / mu_g, -alpha / mu_g};
  fft_g0_chain(fu_, alpha, c12, fused ? tau_ : nullptr);   // (fused: the polarisation is never stored, its field is free for the x-contiguous layout)
  // adj = E - 2 alpha m <tau>;  eta = adj + sym grad u;  eta.xpay(eta, 2 alpha m, tau_copy)  F:20438-20452, one sweep
  Vec6 Ev;
  for (int c = 0; c < 6; ++c) Ev.v[c] = E6[c];
  time_begin(9);
  if (fused && dfg())
    launch_eps_delta_recompute(g_, ptrs3(fu_), ptrs6(src), sp, dfg_moduli(), dscal_ + kSlotMean, (double)nglobal_, Ev,
                               2 * alpha * m, ptrs6(dst), partial_, dscal_ + kSlotSumSq, stream_);
  else if (fused)
    launch_eps_delta_recompute(g_, ptrs3(fu_), ptrs6(src), sp, phase_ptrs(), dscal_ + kSlotMean, (double)nglobal_, Ev,
                               2 * alpha * m, ptrs6(dst), partial_, dscal_ + kSlotSumSq, stream_);
  else
    launch_eps_delta(g_, ptrs3(fu_), ptrs6(tau_), dscal_ + kSlotMean, (double)nglobal_, Ev, 2 * alpha * m, ptrs6(dst),
                     partial_, dscal_ + kSlotSumSq, stream_);
  time_end(9);
  pass_done(E6, dst, false);
}

// The six-component Fourier pass of the collocated and the willot operators (fftTensor, Gamma0_hat, fftInvTensor), also
// method polarization's.  op.bc: F0 = Re tau_hat(0) (initBCProjector(tau_hat) F:20219-20225) and the zero frequency of eta_hat
// becomes mean + R (applyBCProjector(eta_hat, alpha) F:20272-20279) -- the Fourier kernels set it to the value handed in.
// xpay: dst holds a field that is added with this weight (eta.xpay of the Delta operators) instead of being overwritten.
void Solver::fourier_pass6(const GammaHat& op, double* dst, const double* xpay) {
  time_begin(2);
  fft_->forward(tau_, 6, g_.n, 1 / (double)nglobal_);   // fftTensor: 1/N on the forward transform  F:18531-18560
  time_end(2);
  Vec6 mean = op.mean;
  if (op.bc) {
    double F0[6], R[6];
    fetch_mean6(F0, true);
    bc_correction(BC_MQ_, BC_M_, BC_QC0_, opt_.bc_relax, op.alpha, F0, F00_, R);
    for (int c = 0; c < 6; ++c) mean.v[c] += R[c];
  }
  if (op.willot) {
    const WillotTables wt = willot_tables();   // (built on first use, outside the slot)
    time_begin(5);
    launch_gamma_willot(g_, ptrs6(tau_), wt, op.mu, op.lambda, op.alpha, op.beta, mean, op.sums, op.sums_scale, stream_);
    time_end(5);
  } else {
    XiTables xt;
    for (int a = 0; a < 3; ++a) xt.xi[a] = xi_[a];
    const double c10 = op.alpha / (4 * op.mu);
    const double c20 = -op.alpha / (op.mu * (1 + op.mu / (op.lambda + op.mu)));
    time_begin(5);
    launch_gamma_collocated(g_, ptrs6(tau_), xt, c10, c20, op.beta, mean, stream_, op.sums, op.sums_scale);
    time_end(5);
  }
  time_begin(8);
  fft_->inverse(tau_, 6, g_.n);
  time_end(8);
  time_begin(9);
  if (xpay) {
    const double* in[2] = {tau_, dst};
    const double w[2] = {1.0, *xpay};
    launch_lincomb(2, in, w, dst, 6 * g_.n, stream_);
  } else {
    launch_copy(tau_, dst, 6 * g_.n, stream_);
  }
  launch_sum6(g_, ptrs6(dst), true, partial_, dscal_ + kSlotSumSq, stream_);
  time_end(9);
}

// GammaOperatorCollocated  F:20302-20310: fftTensor, initBCProjector, Gamma0_hat, applyBCProjector, fftInvTensor on the
// six components
void Solver::pass_collocated(const double* E6, double* src, double* dst) {
  time_begin(0);
  stress_to_tau(stress_params(opt_.mu_0, opt_.lambda_0, 1.0), src);
  time_end(0);
  GammaHat op = {false, opt_.mu_0, opt_.lambda_0, -1.0, 0.0, {}, mixed_bc() || opt_.bc_relax != 1.0, nullptr, 0.0};
  for (int c = 0; c < 6; ++c) op.mean.v[c] = E6[c];
  fourier_pass6(op, dst);
  pass_done(E6, dst, false);
}

// GammaOperatorStaggered  F:20288-20300:  tau = (C - C0):eps ; f = div tau ; u = G0 f ; eps = E + sym grad u (+ R)
void Solver::pass_staggered(const double* E6, double* src, double* dst) {
  const double alpha = -1.0;  // GammaOperator(..., -1)  F:20575
  const StressParams sp = stress_params(opt_.mu_0, opt_.lambda_0, 1.0);
  // initBCProjector  F:20228-20239 needs <tau> only for mixed boundary conditions
  double F0[6] = {0, 0, 0, 0, 0, 0};
  const bool mixed = mixed_bc();
  const plan::SweepPlan sweeps = sweep_plan(0);
  time_begin(0);
  switch (sweeps.staggered) {
    case plan::Staggered::Tile:
      // the fast kernels allowed (u_loop = 2) and a grid the tiles fit: the LDS-tiled form on the moduli arrays (Voigt and Reuss);
      // it also delivers the sums of tau, so mixed boundary conditions keep the fused sweep
      if (sweeps.staggered_dfg)
        launch_eps_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs6(src), dfg_moduli(), ptrs3(fu_), partial_, dscal_ + kSlotMean, stream_);
      else
        launch_eps_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs6(src), effective_moduli(), ptrs3(fu_), partial_, dscal_ + kSlotMean, stream_);
      time_end(0);
      if (mixed) fetch_mean6(F0);
      break;
    case plan::Staggered::FusedVoigt:   // Voigt mixing: polarisation and divergence in one sweep (tau never stored)
      launch_stress_div_voigt(g_, sp, ptrs6(src), phase_ptrs(), ptrs3(fu_), stream_);
      time_end(0);
      break;
    case plan::Staggered::Stored:
      // the laminate rule (its per-voxel Newton solve is too costly to repeat at the six neighbours) and general phases (both
      // fused forms evaluate the polarisation from (mu, lambda))
      stress_to_tau(sp, src);
      time_end(0);
      if (mixed) {
        launch_sum6(g_, ptrs6(tau_), false, partial_, dscal_ + kSlotMean, stream_);
        fetch_mean6(F0);
      }
      time_begin(1);
      launch_div(g_, ptrs6(tau_), ptrs3(fu_), kNoXHalo, stream_);
      time_end(1);
      break;
  }
  fft_g0_chain(fu_, alpha, nullptr, tau_);   // the polarisation is dead once its divergence is taken

  // applyBCProjector  F:20247-20270
  Vec6 E, R;
  for (int c = 0; c < 6; ++c) E.v[c] = E6[c], R.v[c] = 0.0;
  if (mixed || opt_.bc_relax != 1.0) bc_correction(BC_MQ_, BC_M_, BC_QC0_, opt_.bc_relax, alpha, F0, F00_, R.v);
  bool add_R = false;
  for (int c = 0; c < 6; ++c)
    if (R.v[c] != 0.0) add_R = true;
  time_begin(9);
  launch_eps_norm(g_, ptrs3(fu_), ptrs6(dst), E, R, add_R, partial_, dscal_ + kSlotSumSq, kNoXHalo, stream_);
  time_end(9);
  // fu_ now holds the displacement this strain was built from (eps = E + sym grad u when R == 0)
  pass_done(E6, dst, !add_R && dst == eps_);
}

// GammaOperatorFourierWillotR  F:19130-19152: tan(q / 2) / (4 w) and 1 + e^{iq} per axis, host libm; built and uploaded on
// the first pass of the scheme (the grid of a solver never changes), so solvers that never ask for it pay nothing
WillotTables Solver::willot_tables() {
  const int len[3] = {nxg_, g_.ny, g_.nz};
  const double d[3] = {g_.dx, g_.dy, g_.dz};
  for (int a = 0; a < 3; ++a) {
    if (wil_e_[a]) continue;
    const int cnt = (a == 2) ? g_.nzc : len[a];
    std::vector<double> wt;
    std::vector<cplx> we;
    willot_axis_table(len[a], d[a], cnt, &wt, &we);
    FG_HIP_CHECK(hipMalloc(&wil_t_[a], cnt * sizeof(double)));
    FG_HIP_CHECK(hipMalloc(&wil_e_[a], cnt * sizeof(cplx)));
    FG_HIP_CHECK(hipMemcpy(wil_t_[a], wt.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
    FG_HIP_CHECK(hipMemcpy(wil_e_[a], we.data(), cnt * sizeof(cplx), hipMemcpyHostToDevice));
  }
  WillotTables t;
  for (int a = 0; a < 3; ++a) t.t[a] = wil_t_[a], t.e[a] = wil_e_[a];
  return t;
}

// gamma_scheme willot, one pass.  Elasticity: GammaOperatorWillotR  F:20322-20330 = fftTensor, initBCProjector(tau_hat),
// GammaOperatorFourierWillotR, applyBCProjector(eta_hat), fftInvTensor on the six components, routed like the collocated
// scheme.  Viscosity: DeltaOperatorWillotR  F:20380-20418: m = 1 / (4 mu0); adj = E - 2 alpha m <tau>;
// eta = GammaWillotR(adj; mu = -1 / (4 m), lambda = inf)(tau) + 2 alpha m tau_copy -- tau_copy lives in dst (the strain the
// polarisation was made from is dead by then), <tau> stays on the device as in the staggered Delta path.
void Solver::willot_scheme(const double* E6, double* src, double* dst) {
  const double alpha = -1.0;  // GammaOperator(..., -1)  F:20575
  const bool visc = opt_.mode == 2;
  const double m = visc ? 1 / (4 * opt_.mu_0) : 0.0;
  time_begin(0);
  stress_to_tau(stress_params(opt_.mu_0, opt_.lambda_0, 1.0), src);
  time_end(0);
  GammaHat op = {true, opt_.mu_0, opt_.lambda_0, alpha, 0.0, {}, mixed_bc() || opt_.bc_relax != 1.0, nullptr, 0.0};
  for (int c = 0; c < 6; ++c) op.mean.v[c] = E6[c];
  if (!visc) {
    fourier_pass6(op, dst);
  } else {
    launch_sum6(g_, ptrs6(tau_), false, partial_, dscal_ + kSlotMean, stream_);   // tau_copy->average(), stays on the device
    // applyBCProjector(eta_hat, alpha): R = alpha MQ <tau> folded into the sums, as in the staggered Delta path
    if (mixed_bc()) bc_adjust_sums(alpha / (2 * alpha * m));
    launch_copy(tau_, dst, 6 * g_.n, stream_);   // tau_copy
    op.mu = -1.0 / (4 * m);
    op.lambda = INFINITY;
    op.bc = false;
    op.sums = dscal_ + kSlotMean;
    op.sums_scale = -(2 * alpha * m) / (double)nglobal_;
    const double xpay = 2 * alpha * m;   // eta.xpay(eta, 2 alpha m, tau_copy)  F:20411
    fourier_pass6(op, dst, &xpay);
  }
  pass_done(E6, dst, false);
}

// z and y transforms of a plane in one kernel (grids whose complex z-y plane fits the LDS): option plane_fft (-1 = where
// available, 0 = off for A/B runs)
bool Solver::plane_fft_on() const {
  return opt_.plane_fft != 0 && nranks_ == 1 && fft_->can_plane();
}

// The transform chain of a pass on buf (one component in the scalar modes, else three): the decisions, made once, and the
// Green operator's constants; g0_chain (fg_g0_chain.h) has the schedule and the timing slots.
// alpha = -1: GammaOperator(..., -1)  F:20575
void Solver::fft_g0_chain(double* buf, double alpha, const double* c12, double* xscratch) {
  fft_->set_joint_x(opt_.joint_x != 0);
  const bool scalar = opt_.mode == 1;
  G0ChainPlan p;
  p.ncomp = scalar ? 1 : 3;
  p.nx = g_.nx;
  p.has_x = g_.nx > 1;
  p.has_y = g_.ny > 1;
  p.scale = 1 / (double)nglobal_;
  // x-contiguous layout for the fused pass: on by size (fields beyond the Infinity Cache, where the fused pass's tile of nx
  // segments 2 MB apart is what bounds it) unless the option x_layout says otherwise
  const int xl_opt = opt_.x_layout;
  p.xlayout = !scalar && xscratch && opt_.fuse_x && fft_->can_fuse(0) && fft_->can_xlayout() && p.has_x && p.has_y &&
              (xl_opt > 0 || (xl_opt < 0 && 3.0 * (double)g_.n * sizeof(double) > 1024.0 * 1024 * 1024));
  p.plane = !p.xlayout && plane_fft_on() && p.has_x;   // small grids
  p.pair_chunk = pair_chunk_planes();                  // (0 where the plane kernel is on)
  p.fuse_x = opt_.fuse_x && fft_->can_fuse(0, p.ncomp);   // (no length-1 x pass is fusable: has_x need not be asked)
  if (scalar) {
    p.c10 = -alpha / (2 * opt_.mu_0);  // G0OperatorFourierStaggeredHeat  F:19759-19764
    p.c20 = 0.0;
  } else {
    p.c10 = -alpha / (opt_.mu_0);      // G0OperatorFourierStaggered  F:19749-19755
    p.c20 = -alpha / (opt_.mu_0 * (1 + opt_.mu_0 / (opt_.lambda_0 + opt_.mu_0)));
    if (c12) p.c10 = c12[0], p.c20 = c12[1];
  }
  g0_chain(*this, p, buf, xscratch);
}

// the passes g0_chain calls back; a window (x0, np) with np < 0 is the whole field
void Solver::chain_r2c_z(double* buf, int ncomp, int x0, int np) {
  const PlaneWindow w = {x0, np};
  fft_->r2c_z(buf, ncomp, g_.n, np < 0 ? nullptr : &w);
}
void Solver::chain_c2r_z(double* buf, int ncomp, int x0, int np) {
  const PlaneWindow w = {x0, np};
  fft_->c2r_z(buf, ncomp, g_.n, np < 0 ? nullptr : &w);
}
void Solver::chain_c2c_y(double* buf, int ncomp, int dir, double scale, int x0, int np) {
  const PlaneWindow w = {x0, np};
  fft_->c2c_y(buf, ncomp, g_.n, dir, scale, np < 0 ? nullptr : &w);
}
void Solver::chain_c2c_y_xlayout(double* in, double* out, int ncomp, int dir, int x0, int np) {
  const PlaneWindow w = {x0, np};
  fft_->c2c_y_xlayout(in, g_.n, out, g_.n, ncomp, dir, 1.0, np < 0 ? nullptr : &w);
}
void Solver::chain_c2c_x(double* buf, int ncomp, int dir, double scale) { fft_->c2c_x(buf, ncomp, g_.n, dir, scale); }
void Solver::chain_zy_plane(double* buf, int ncomp, int dir) { fft_->zy_plane(buf, ncomp, g_.n, dir); }
void Solver::chain_scale(double* buf, int ncomp, double scale) { fft_->scale(buf, ncomp, g_.n, scale); }

// x transform, 1/N, Green operator and inverse x transform in one kernel (spectrum stays in registers)
void Solver::chain_fused_x(double* data, int ncomp, double scale, double c10, double c20, bool xlayout) {
  G0Params gp;
  for (int a = 0; a < 3; ++a) gp.kpm[a] = g0_kpm_[a], gp.kp[a] = g0_kp_[a];
  gp.c10 = c10;
  gp.c20 = c20;
  gp.inv_h0 = 2.0 * nxg_ / g_.dx;
  fft_->fused_g0(data, g_.n, 0, scale, gp, 0, ncomp, 31, 0, xlayout);   // (xsplit 31, xjump 0: the defaults, no slab layout)
}

void Solver::chain_green(double* buf, int ncomp, double c10, double c20) {
  G0Tables tb;
  for (int a = 0; a < 3; ++a) {
    tb.kpm[a] = g0_kpm_[a];
    tb.kp[a] = g0_kp_[a];
  }
  if (ncomp == 1) launch_g0_heat(g_, buf, tb, c10, stream_);   // G0OperatorStaggeredHeat  F:20118-20135: c1 = c10 / |k|^2
  else launch_g0(g_, ptrs3(buf), tb, c10, c20, G0Layout{0, 0, 0}, stream_);
}

// Planes per chunk of the paired z / y passes (0 = whole-field passes, the default).  Measured in round 6 and NOT faster:
// a bytes-only pair of copy passes gains 1.32 x from 128-MB chunks (tools/mall_chunk_probe.hip), the transform passes lose
// 3-10 % at every chunk size (EXPERIMENTS.md, round 6) -- they are bound by the requests a workgroup keeps in flight, which an
// Infinity-Cache hit does not shorten.  Kept as an option: same kernels on the same lines, bit-identical iterates.
int Solver::pair_chunk_planes() const {
  if (opt_.pair_chunk <= 0 || !fft_->can_window() || g_.nx < 2 || g_.ny < 2 || plane_fft_on()) return 0;
  return std::min(opt_.pair_chunk, g_.nx);
}


// ------------------------------------------------------------------ displacement-based pass
// eps_k = E + sym grad u_k is implied by the displacement of the previous pass, so the loop can carry
// u (3 components) instead of eps (6): one sweep turns u_k into the sums of squares of eps_k (the
// error estimator of pass k) and f_{k+1} = div (C - C0):eps_k, then the transform chain gives u_{k+1}.
// Same values as strain operator + polarisation + divergence (bit for bit), 2 kernels fewer per pass.
ScalarParams Solver::scalar_params(double mu_0, double alpha) const {
  ScalarParams sp;
  sp.n = pt_.n;
  for (int q = 0; q < kMaxPhases; ++q) {
    sp.mu[q] = q < pt_.n ? pt_.mu[q] : 0.0;
    sp.law[q] = q < pt_.n ? sc_law_[q] : kScLawIso;
    for (int c = 0; c < 6; ++c) sp.K[q][c] = q < pt_.n ? sc_K_[q][c] : 0.0;
  }
  sp.alpha = alpha;
  sp.beta = -alpha * 2 * mu_0;  // calcStress  F:18138
  sp.mixing = opt_.mixing;
  return sp;
}

FieldPtrs<kMaxPhases> Solver::phase_ptrs() const {
  FieldPtrs<kMaxPhases> phi;
  for (int q = 0; q < kMaxPhases; ++q) phi.p[q] = q < pt_.n ? phi_ + (long)q * g_.n : nullptr;
  return phi;
}

FieldPtrs<3> Solver::normal_ptrs() const {
  FieldPtrs<3> nrm;
  for (int c = 0; c < 3; ++c) nrm.p[c] = normals_ ? normals_ + (long)c * g_.n : nullptr;
  return nrm;
}

// What the refusals and the choice of sweeps read (fg_sweep_plan.h).  ask: 0 the refusals and the strain-state passes (no
// complement check), 1 the loop decision, 2 the sweeps of the displacement / potential loop.
plan::PlanInput Solver::plan_input(plan::Entry entry, int ask) {
  plan::PlanInput in;
  in.mode = opt_.mode, in.mixing = opt_.mixing, in.gamma_scheme = opt_.gamma_scheme, in.method = opt_.method;
  in.error_estimator = opt_.error_estimator, in.u_loop = opt_.u_loop;
  in.u_tile = opt_.u_tile != 0, in.fuse_stress_div = opt_.fuse_stress_div != 0, in.cg_fused = opt_.cg_fused != 0;
  in.phi_sweep = opt_.phi_sweep != 0, in.aniso_tile = opt_.aniso_tile != 0, in.aniso_sc_tile = opt_.aniso_sc_tile != 0;
  in.reuss_sweep = opt_.reuss_sweep != 0, in.bc_relaxed = opt_.bc_relax != 1.0;
  in.n_phases = pt_.n, in.general_phase = general_phase(), in.aniso_phase = aniso_phase();
  for (int p = 0; p < pt_.n && in.mixing == kMixReuss; ++p)
    in.reuss_invertible = in.reuss_invertible && (opt_.mode == 0 ? 2 * pt_.mu[p] > 0 && 2 * pt_.mu[p] + 3 * pt_.lambda[p] > 0 : pt_.mu[p] > 0);
  in.tiled = u_tile_supported(g_), in.normals = normals_ != nullptr;
  in.multi_rank = nranks_ != 1, in.slab = in.multi_rank || slab_layout_, in.slab_ys = fft_ys_ != nullptr;
  in.mixed_bc = mixed_bc(), in.bc_identity = frobenius(BC_Q_) == 0.0;   // Q = Id - P != 0  <=>  |MQ| >= eps
  in.entry = entry, in.in_run = in_run_;
  in.complementary = ask > 0 && plan::reads_complement(in, ask > 1) && two_phase_complementary();
  return in;
}

void Solver::require_plan(plan::Entry entry) {
  if (const char* refusal = plan::plan_error(plan_input(entry))) throw std::runtime_error(refusal);
}

// Two phases whose fractions are complementary bit for bit (phi_0 == 1 - phi_1: what normalizePhi leaves for two
// materials), checked once per geometry on the device.  Option phi_sweep = 0 switches the shortcut off (A/B runs).
bool Solver::two_phase_complementary() {
  if (complement_dirty_) {
    ++complement_checks_;
    int one = 1;
    FG_HIP_CHECK(hipMemcpyAsync(derr_ + 1, &one, sizeof(int), hipMemcpyHostToDevice, stream_));
    launch_complement_check(g_, phi_, phi_ + g_.n, derr_ + 1, stream_);
    int flag = 0;
    FG_HIP_CHECK(hipMemcpyAsync(&flag, derr_ + 1, sizeof(int), hipMemcpyDeviceToHost, stream_));
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    complementary_ = flag != 0;
    complement_dirty_ = false;
  }
  return complementary_;
}

// A = sum_p phi_p 2 mu_p, B = sum_p phi_p lambda_p per voxel (k_effective_moduli; Reuss mixing: 2 mu_bar, lambda_bar of the harmonic
// means), computed once per geometry and rule
FieldPtrs<2> Solver::effective_moduli() {
  if (general_phase() || aniso_phase())
    throw std::logic_error("effective moduli (sum phi 2 mu, sum phi lambda) do not exist with a general or an aniso phase");
  if (!mod_) {
    FG_HIP_CHECK(hipMalloc(&mod_, 2 * (size_t)g_.n * sizeof(double)));
    mod_dirty_ = mod5_dirty_ = true;
  }
  FieldPtrs<2> mod;
  mod.p[0] = mod_;
  mod.p[1] = mod_ + g_.n;
  const int rule = opt_.mixing == kMixReuss ? kMixReuss : kMixVoigt;   // (laminate: the Voigt sweep + its correction)
  if (rule != mod_rule_) mod_dirty_ = true;   // the rule changed on a live solver
  if (mod_dirty_) {
    PhaseTable t = phase_table();
    if (opt_.mode == 1)   // scalar modes: k_effective_moduli stores sum phi 2 mu (its harmonic mean), the sweep wants that of mu
      for (int q = 0; q < kMaxPhases; ++q) t.mu[q] = 0.5 * pt_.mu[q], t.lambda[q] = 0.0;
    launch_effective_moduli(g_, t, phase_ptrs(), mod, stream_, rule);
    mod_dirty_ = false;
    mod_rule_ = rule;
  }
  return mod;
}

void Solver::sc_aniso_constants(double* K0, double* K1) const {
  for (int p = 0; p < 2; ++p) {
    double* K = p ? K1 : K0;
    for (int c = 0; c < 6; ++c) K[c] = sc_law_[p] == kScLawAniso ? sc_K_[p][c] : (c < 3 ? pt_.mu[p] : 0.0);
  }
}

FieldPtrs<5> Solver::dfg_moduli() {
  plan::PlanInput in;   // (what dfg_refusal reads)
  in.gamma_scheme = opt_.gamma_scheme, in.mode = opt_.mode, in.mixing = opt_.mixing, in.slab = nranks_ != 1 || slab_layout_;
  if (const char* refusal = plan::dfg_refusal(in)) throw std::runtime_error(refusal);
  if (!mod5_) {
    FG_HIP_CHECK(hipMalloc(&mod5_, 5 * (size_t)g_.n * sizeof(double)));
    mod5_dirty_ = true;
  }
  FieldPtrs<5> mod;
  for (int q = 0; q < 5; ++q) mod.p[q] = mod5_ + (long)q * g_.n;
  if (mod5_dirty_) {
    if (!phis_) {
      FG_HIP_CHECK(hipMalloc(&phis_, 3 * (size_t)pt_.n * g_.n * sizeof(double)));
      FG_HIP_CHECK(hipMemsetAsync(phis_, 0, 3 * (size_t)pt_.n * g_.n * sizeof(double), stream_));
    }
    for (int p = 0; p < pt_.n; ++p) {   // coarse input: the fine field is its piecewise-constant replica
      if (fine_set_ & (1u << p)) continue;
      FieldPtrs<3> s;
      for (int c = 0; c < 3; ++c) s.p[c] = phis_ + (3L * p + c) * g_.n;
      launch_dfg_fractions_replica(g_, phi_ + (long)p * g_.n, s, stream_);
    }
    launch_dfg_moduli(g_, phase_table(), phi_, phis_, mod, stream_);
    mod5_dirty_ = false;
  }
  return mod;
}

void Solver::stress_to_tau(const StressParams& sp, double* src) {
  if (dfg()) launch_dfg_stress(0, g_, sp, ptrs6(src), dfg_moduli(), ptrs6(tau_), nullptr, nullptr, stream_);
  else launch_stress(g_, sp, ptrs6(src), phase_ptrs(), normal_ptrs(), ptrs6(tau_), derr_, stream_);
}

void Solver::build_laminate_lists() {
  if (!mixed_dirty_) return;
  const FieldPtrs<kMaxPhases> phi = phase_ptrs();
  for (void* p : {(void*)mixed_list_, (void*)aff_list_, (void*)aff_slots_, (void*)dtau_})
    if (p) FG_HIP_CHECK(hipFree(p));
  mixed_list_ = aff_list_ = nullptr;
  aff_slots_ = nullptr;
  dtau_ = nullptr;
  aff_n_ = 0;
  for (void* p : {(void*)lam_phic_, (void*)lam_nrmc_, (void*)lam_epsc_})
    if (p) FG_HIP_CHECK(hipFree(p));
  lam_phic_ = lam_nrmc_ = lam_epsc_ = nullptr;
  mixed_n_ = launch_mixed_list(g_, pt_.n, phi, &mixed_list_, stream_);
  if (mixed_n_) {
    FG_HIP_CHECK(hipMalloc(&dtau_, (size_t)mixed_n_ * 6 * sizeof(double)));
    // compact static copies for the interface solve (k_interface_solve) and its strain scratch
    const size_t n = mixed_n_;
    FG_HIP_CHECK(hipMalloc(&lam_phic_, n * pt_.n * sizeof(double)));
    FG_HIP_CHECK(hipMalloc(&lam_nrmc_, n * 3 * sizeof(double)));
    FG_HIP_CHECK(hipMalloc(&lam_epsc_, n * 6 * sizeof(double)));
    launch_interface_static(g_, pt_.n, phi, normal_ptrs(), mixed_list_, mixed_n_, lam_phic_, lam_nrmc_, stream_);
    // x-slab: no x neighbours across the slab faces in the slots (gu_: the grid with the slab's plane mapping)
    aff_n_ = launch_affected_list(slab_layout_ ? gu_ : g_, mixed_list_, mixed_n_, &aff_list_, &aff_slots_, stream_);
  }
  mixed_dirty_ = false;
}

// laminate mixing = the Voigt sweep over all voxels + the divergence of (tau_laminate - tau_voigt), which lives on the interface
// voxels (lists built once per geometry, see k_interface_strain).  d depends on u only: its two kernels (a light gather, a short
// solve) run on a second stream beside the sweep (option laminate_overlap).  Fork: u_k is complete, the previous pass is done with d
void Solver::laminate_fork() {
  build_laminate_lists();
  if (!opt_.laminate_overlap) return;
  if (!aux_stream_) {
    int lo = 0, hi = 0;
    FG_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));   // hi = numerically lowest = highest priority
    FG_HIP_CHECK(hipStreamCreateWithPriority(&aux_stream_, hipStreamNonBlocking, hi));
    FG_HIP_CHECK(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
    FG_HIP_CHECK(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
  }
  FG_HIP_CHECK(hipEventRecord(ev_fork_, stream_));
}

void Solver::laminate_correction(const Vec6& E) {
  hipStream_t ds = opt_.laminate_overlap ? aux_stream_ : stream_;
  if (ds != stream_) FG_HIP_CHECK(hipStreamWaitEvent(ds, ev_fork_, 0));
  launch_interface_delta(g_, stress_params(opt_.mu_0, opt_.lambda_0, 1.0), ptrs3(fu_), E, mixed_list_, mixed_n_, lam_epsc_,
                         lam_phic_, lam_nrmc_, dtau_, derr_, ds);
  if (ds != stream_) {
    FG_HIP_CHECK(hipEventRecord(ev_join_, ds));
    FG_HIP_CHECK(hipStreamWaitEvent(stream_, ev_join_, 0));
  }
  launch_delta_div(g_, aff_list_, aff_slots_, aff_n_, dtau_, ptrs3(fu_alt_), stream_);
  if (mixed_bc())   // mixed BC: <tau_laminate> = <tau_voigt> (from the sweep) + sum of the differences / N
    launch_sum_dtau(dtau_, mixed_n_, partial_, dscal_ + kSlotScratch, stream_);
}

void Solver::u_pass_front(const double* E6) {
  using plan::Front;
  const FieldPtrs<kMaxPhases> phi = phase_ptrs();
  // the strain that belongs to u_k was built with the prescribed strain of ITS pass (E_cur_);
  // E6 is the prescribed strain of the pass being started and takes effect with u_{k+1}
  Vec6 E;
  for (int c = 0; c < 6; ++c) {
    E.v[c] = E_cur_[c];
    E_next_[c] = E6[c];
  }
  const plan::SweepPlan sweeps = sweep_plan();
  const bool sum_tau = sweeps.sum_tau;   // mixed BC: sums of tau land in kSlotMean
  const StressParams sp = stress_params(opt_.mu_0, opt_.lambda_0, 1.0);
  const PhaseTable t = phase_table();
  FieldPtrs<2> ph;   // two phases with phi_0 = 1 - phi_1: the sweep reads phi_1 and forms the moduli itself (8 B per voxel less)
  ph.p[0] = phi_ + g_.n;
  ph.p[1] = nullptr;
  double K0[6], K1[6];
  time_begin(0);
  if (sweeps.laminate_correction) laminate_fork();
  switch (sweeps.front) {
    case Front::ScFast:   // effective conductivity a = sum_p phi_p mu_p precomputed (first moduli array)
      sc_tau_sums_ = launch_sc_sweep_fast(g_, opt_.mu_0, fu_, effective_moduli().p[0], fu_alt_, E, partial_, dscal_ + kSlotSumSq, stream_,
                                          sum_tau ? dscal_ + kSlotMean : nullptr);
      front_sweep_ = (long)Front::ScFast;
      break;
    case Front::ScTileAniso:
      sc_aniso_constants(K0, K1);
      sc_tau_sums_ = false;
      launch_sc_tile_aniso(g_, opt_.mu_0, K0, K1, fu_, phi_ + g_.n, fu_alt_, E, partial_, dscal_ + kSlotSumSq, stream_);
      ++sc_tile_aniso_;
      front_sweep_ = (long)Front::ScTileAniso;
      break;
    case Front::ScExact:   // (an aniso phase has no conductivity array: the 13-point form of the exact-order sweep)
      sc_tau_sums_ = false;
      launch_sc_sweep(g_, scalar_params(opt_.mu_0, 1.0), fu_, phi, fu_alt_, E, partial_, dscal_ + kSlotSumSq, stream_);
      front_sweep_ = (long)Front::ScExact;
      break;
    case Front::UStressThenDiv:
      // laminate / Reuss mixing, exact order: strain + polarisation from u in one sweep (tau stored), divergence as its own sweep
      launch_u_stress(g_, sp, ptrs3(fu_), phi, normal_ptrs(), ptrs6(tau_), E, partial_, dscal_ + kSlotSumSq, derr_, stream_);
      time_end(0);
      time_begin(1);
      launch_div(g_, ptrs6(tau_), ptrs3(fu_alt_), kNoXHalo, stream_);
      time_end(1);
      front_sweep_ = (long)Front::UStressThenDiv;
      eps_stale_ = true;
      return;
    case Front::UTileDfg:   // full_staggered: the five moduli, also for two complementary phases
      launch_u_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), dfg_moduli(), ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_, sum_tau);
      front_sweep_ = (long)Front::UTileDfg;
      break;
    case Front::UTileAniso:
      launch_u_tile_aniso(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), phi_ + g_.n, ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_,
                          sum_tau, t);
      ++u_tile_aniso_;
      front_sweep_ = (long)Front::UTileAniso;
      break;
    case Front::UTilePhi:
      launch_u_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), ph, ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_, sum_tau, &t, false);
      front_sweep_ = (long)Front::UTilePhi;
      break;
    case Front::UTilePhiReuss:
      launch_u_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), ph, ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_, sum_tau, &t, true);
      ++u_tile_reuss_;
      front_sweep_ = (long)Front::UTilePhiReuss;
      break;
    case Front::UTileModuli:   // per-voxel effective moduli instead of the per-phase accumulation (once per geometry, on first use)
      launch_u_tile(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), effective_moduli(), ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_,
                    sum_tau);
      front_sweep_ = (long)Front::UTileModuli;
      break;
    case Front::UFastModuli:   // grids the tiles do not fit (odd nz, short rows): the untiled sweep
      launch_u_fast(g_, opt_.mu_0, opt_.lambda_0, ptrs3(fu_), effective_moduli(), ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_);
      front_sweep_ = (long)Front::UFastModuli;
      break;
    case Front::UStressDivVoigt:
      launch_u_stress_div_voigt(g_, sp, ptrs3(fu_), phi, ptrs3(fu_alt_), E, partial_, dscal_ + kSlotSumSq, stream_);
      front_sweep_ = (long)Front::UStressDivVoigt;
      break;
    case Front::None:
      throw std::logic_error("u_pass_front: this configuration has no displacement / potential loop");
  }
  if (sweeps.laminate_correction) laminate_correction(E);
  time_end(0);
  eps_stale_ = true;
}

void Solver::u_pass_back() {
  back_ready_ = false;
  launch_pending_back();
  adopt_back();
}

void Solver::ensure_eps() {
  if (pol_state_) polar_to_strain();   // method polarization left P in eps_
  if (slab_layout_ && su_valid_ && eps_stale_) {   // slab driver: the state is su_[cur] with its halo planes
    slab_materialise_eps();
    return;
  }
  if (!eps_stale_ || !u_valid_) return;
  Vec6 E, R;
  for (int c = 0; c < 6; ++c) E.v[c] = E_cur_[c], R.v[c] = 0.0;
  if (opt_.mode == 1) {
    launch_sc_grad(g_, fu_, ptrs3(eps_), E, partial_, dscal_ + kSlotScratch, stream_);
    eps_stale_ = false;
    return;
  }
  launch_eps_norm(g_, ptrs3(fu_), ptrs6(eps_), E, R, false, partial_, dscal_ + kSlotScratch,
                  kNoXHalo, stream_);
  eps_stale_ = false;
}

void Solver::iterate(const double* E6, int n) {
  FG_HIP_CHECK(hipSetDevice(device_));
  require_plan(plan::Entry::Iterate);
  int i = 0;
  if (opt_.method == 2) {   // the polarisation loop: from P = 4 mu_0 E unless a polarisation state is there already
    if (pol_state_ && opt_.mu_0 != pol_mu0_) ensure_eps();   // the reference material changed: that state is of another operator
    if (!pol_state_) polar_start(E6);
    for (; i < n; ++i) polar_pass(E6);
    return;
  }
  ensure_eps();   // a polarisation state left by method polarization becomes the strain before another method iterates on it
  if (plan::plan_sweeps(plan_input(plan::Entry::Iterate, 1)).u_loop) {
    if (!u_valid_ && n > 0 && opt_.mode == 1) {
      // no potential yet: the zero gradient field is E = 0, T = 0
      FG_HIP_CHECK(hipMemsetAsync(fu_, 0, g_.n * sizeof(double), stream_));
      for (int c = 0; c < 6; ++c) E_cur_[c] = 0.0;
      u_valid_ = true;
      eps_stale_ = true;
    }
    if (!u_valid_ && n > 0) {
      ensure_eps();
      basic_scheme(E6);  // leaves u in fu_ and eps in eps_
      ++i;
    }
    for (; i < n; ++i) {
      u_pass_front(E6);
      u_pass_back();
    }
    return;
  }
  for (; i < n; ++i) basic_scheme(E6);
}

// ------------------------------------------------------------------ means
// The local halves of the measurements: this solver's (a slab's) contribution enqueued into dscal_ + slot, nothing else.  The lone
// solver fetches and scales it; SlabGroup (fg_slab.hip) all-reduces the members' contributions first.
void Solver::enqueue_strain_sums(int slot, bool squared) {
  launch_sum6(g_, ptrs6(eps_), squared, partial_, dscal_ + slot, stream_);
}

// meanPK1: alpha /= nxyz (global), accumulate  F:12318-12340; heat / porous: the mean flux in the first three slots
void Solver::enqueue_mean_stress(int slot) {
  if (opt_.mode == 1)
    launch_sc_flux_mean(g_, scalar_params(0.0, 1.0 / (double)nglobal_), ptrs3(eps_), phase_ptrs(), partial_, dscal_ + slot, stream_);
  else if (dfg())
    launch_dfg_stress(1, g_, stress_params(0.0, 0.0, 1.0 / (double)nglobal_), ptrs6(eps_), dfg_moduli(), FieldPtrs<6>{}, partial_,
                      dscal_ + slot, stream_);
  else
    launch_stress_mean(g_, stress_params(0.0, 0.0, 1.0 / (double)nglobal_), ptrs6(eps_), phase_ptrs(), normal_ptrs(), partial_,
                       dscal_ + slot, derr_, stream_);
}

// meanW  F:12239-12262: the sum, not yet divided by N
void Solver::enqueue_mean_energy(int slot) {
  if (dfg())
    launch_dfg_stress(2, g_, stress_params(0.0, 0.0, 1.0), ptrs6(eps_), dfg_moduli(), FieldPtrs<6>{}, partial_, dscal_ + slot, stream_);
  else
    launch_energy_mean(g_, stress_params(0.0, 0.0, 1.0), ptrs6(eps_), phase_ptrs(), normal_ptrs(), partial_, dscal_ + slot, derr_,
                       stream_);
}

// extreme eigenvalues of the tangents as (min, -max)
void Solver::enqueue_tangent_minmax(int slot) {
  if (opt_.mode == 1)
    launch_sc_minmax(g_, scalar_params(0.0, 1.0), phase_ptrs(), partial_, dscal_ + slot, stream_);
  else
    launch_tangent_minmax(g_, phase_table(), opt_.mixing, phase_ptrs(), partial_, dscal_ + slot, derr_, stream_);
}

void Solver::enqueue_phase_sum(int p, int slot) { launch_sum1(g_, phi_ + (long)p * g_.n, partial_, dscal_ + slot, stream_); }

// n sums of dscal_ + slot brought to hscal_ + slot, waited for
void Solver::fetch_sums(int slot, int n) {
  FG_HIP_CHECK(hipMemcpyAsync(hscal_ + slot, dscal_ + slot, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Solver::mean_stress(double* out6) {
  FG_HIP_CHECK(hipSetDevice(device_));
  ensure_eps();
  if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
  enqueue_mean_stress(kSlotMean);
  fetch_sums(kSlotMean, 6);
  for (int c = 0; c < 6; ++c) out6[c] = (opt_.mode == 1 && c >= 3) ? 0.0 : hscal_[kSlotMean + c];
}

double Solver::mean_energy() {
  FG_HIP_CHECK(hipSetDevice(device_));
  ensure_eps();
  if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
  if (opt_.mode == 1) throw std::runtime_error("the energy error estimator is not available in heat / porous mode");
  if (opt_.mixing == kMixReuss) throw std::runtime_error("Reuss MaterialLaw energy not implemented");   // F:12657-12661
  enqueue_mean_energy(kSlotMean);
  fetch_sums(kSlotMean, 1);
  return hscal_[kSlotMean] / (double)nglobal_;
}

// estimators 2 (sigma), 3 (energy), 4 (none): fg_stop_rule.h
void Solver::estimator_begin(bool fresh) { fg::estimator_begin(*this, opt_.error_estimator, fresh); }
void Solver::estimator_update(double* abs_err, double* rel_err) { fg::estimator_update(*this, opt_.error_estimator, abs_err, rel_err); }

void Solver::mean_strain(double* out6) {
  FG_HIP_CHECK(hipSetDevice(device_));
  ensure_eps();
  enqueue_strain_sums(kSlotMean, false);
  fetch_mean6(out6);
}

double Solver::volume_fraction(int p) {
  if (p < 0 || p >= pt_.n) throw std::runtime_error("phase index out of range");
  FG_HIP_CHECK(hipSetDevice(device_));
  enqueue_phase_sum(p, kSlotMisc);
  fetch_sums(kSlotMisc, 1);
  return hscal_[kSlotMisc] / (double)nglobal_;
}

// calcRefMaterial  F:22283-22313 -> getRefMaterial  F:12153-12236 (hostmath::ref_mu0)
void Solver::calc_ref_material() {
  FG_HIP_CHECK(hipSetDevice(device_));
  require_plan(plan::Entry::RefMaterial);
  enqueue_tangent_minmax(kSlotMinMax);
  FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotMinMax, dscal_ + kSlotMinMax, 2 * sizeof(double), hipMemcpyDeviceToHost, stream_));
  check_device_error("reference material");
  opt_.mu_0 = ref_mu0(hscal_[kSlotMinMax], -hscal_[kSlotMinMax + 1], opt_.method, opt_.ref_scale);
  recompute_bc();  // F:22312
}

// bc_error  F:21129-21161
double Solver::bc_error(const double* E_cur, const double* S_cur) {
  double Emean[6], Smean[6];
  mean_strain(Emean);
  mean_stress(Smean);
  return bc_error_value(BC_P_, BC_Q_, opt_.bc_tol, Emean, Smean, E_cur, S_cur);
}

// ------------------------------------------------------------------ the solver loop
// The lone solver's side of the stop rule (fg_stop_rule.h): a stop request is fg_cancel, the callback is its own.
template <class BcOk>
bool Solver::converged(const StopRule& rule, long iter, BcOk bc_ok, bool* failed) {
  auto record = [&](double rel_err) { residuals_.push_back(rel_err); };
  auto poll = [&] {
    StopPoll p;
    p.stop = cb_ && cb_(cb_user_);
    p.cancelled = cancel_;   // cancelled from inside the callback
    return p;
  };
  const StopDecision d = rule.decide(iter, stop_hooks([&] { return cancel_.load(); }, record, poll, bc_ok));
  *failed = d == StopDecision::kFail;
  return d != StopDecision::kContinue;
}

// The CG loops' fetch (fg_cg_loop.h): the seven sums of dscal_[slot ..] and the error word start for the host; what is enqueued
// between cg_fetch and cg_wait runs while the host waits for them.
void Solver::cg_fetch(int slot) {
  FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotCg, dscal_ + slot, 7 * sizeof(double), hipMemcpyDeviceToHost, stream_));
  FG_HIP_CHECK(hipMemcpyAsync(herr_, derr_, sizeof(int), hipMemcpyDeviceToHost, stream_));
  FG_HIP_CHECK(hipEventRecord(ev_copy_, stream_));
}

void Solver::cg_wait() {
  FG_HIP_CHECK(hipEventSynchronize(ev_copy_));
  if (*herr_ != 0) check_device_error("cg");
}

// one sum (or n) fetched at once; returns the first
double Solver::cg_fetch_now(int slot, int n) {
  FG_HIP_CHECK(hipMemcpyAsync(hscal_ + slot, dscal_ + slot, n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  check_device_error("cg");
  return hscal_[slot];
}

// the fetched sums of squares as sumsq_ (ncomp of them: 3 in the scalar modes)
const double* Solver::cg_sumsq(int ncomp) {
  for (int c = 0; c < 6; ++c) sumsq_[c] = c < ncomp ? hscal_[kSlotCg + c] : 0.0;
  return sumsq_;
}

// CG in displacement / potential space: w = operator(u_in) with prescribed mean Eadd, i.e. u -> f = div((C - C0)(Eadd + grad_s u))
// -> FFT chain (alpha = -1) -> fu_alt_
void Solver::cg_apply(double* u_in, const double* Eadd, double* xscratch) {
  double* keep = fu_;
  fu_ = u_in;
  for (int c = 0; c < 6; ++c) E_cur_[c] = Eadd[c];
  u_pass_front(Eadd);   // sweeps fu_ (with E_cur_) into fu_alt_; its norm sums are not used here
  fu_ = keep;
  fft_g0_chain(fu_alt_, -1.0, nullptr, xscratch);
}

// CG in displacement / potential space: what accessors called from a callback / bc_error see is eps = E + grad_s fu_
void Solver::cg_set_state(const Vec6& E) {
  u_valid_ = true;
  eps_stale_ = true;
  for (int c = 0; c < 6; ++c) E_cur_[c] = E.v[c];
}

// end of a CG run; E: the run was carried in displacement / potential space, the strain field is materialised from (E, fu_)
void Solver::cg_finish(long iter, double t_start, const Vec6* E) {
  iterations_ = iter;
  if (E) {
    cg_u_active_ = false;
    cg_set_state(*E);
    ensure_eps();
  }
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  solve_time_ += now_seconds() - t_start;
}

// run F:21247-21398 -> runLoadsteppingSolver (single load step, t = 1) F:21584-21685
// -> runSolver -> runBasic F:21716-21805 with the stop rule of _converged F:21177-21244.
bool Solver::run(const double* E6, const double* S6) {
  const double one = 1.0;
  return run_load_steps(E6, S6, &one, 1, 0, nullptr, nullptr);
}

// norm of the current strain field as EpsilonErrorEstimator's constructor takes it (F:14612-14618): a load step that
// continues from the previous one starts its error estimate there, the first one at the zero field
double Solver::current_norm9() {
  ensure_eps();
  enqueue_strain_sums(kSlotScratch, true);
  fetch_sums(kSlotScratch, 6);
  double s9 = 0.0;
  const int nc = opt_.mode == 1 ? 3 : 6;
  for (int c = 0; c < nc; ++c) {
    const double m = std::sqrt(hscal_[kSlotScratch + c] / (double)nglobal_);
    s9 += m * m * ((c >= 3) ? 2.0 : 1.0);   // shear norms mirrored to 9 entries (fix_dim)
  }
  return std::sqrt(s9);
}

// runLoadsteppingSolver  F:21584-21685: the prescribed values are scaled by the parameter of every load step, every
// step continues from the strain field of the one before (the field is zeroed once, in run(), F:21379), and after each
// step the load-step action runs (performLoadstepActions F:21435-21447: the caller's callback, non-zero = stop).
// Load-step extrapolation (loadstep_extrapolation_order > 0, polynomial method F:21468-21514): from the second step on the
// step starts from the polynomial through the converged strain fields of the last order + 1 steps evaluated at its parameter.
bool Solver::run_load_steps(const double* E6, const double* S6, const double* params, int nparams, int first,
                            LoadstepCallback step_cb, void* user) {
  FG_HIP_CHECK(hipSetDevice(device_));
  if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
  check_load_steps(params, nparams, first);
  solve_time_ = 0.0;
  cg_u_active_ = false;
  residuals_.clear();
  iterations_ = 0;
  cancel_ = false;
  double Emax[6], Smax[6];
  for (int i = 0; i < 6; ++i) {
    Emax[i] = E6[i];
    Smax[i] = S6 ? S6[i] : 0.0;
  }
  recompute_bc();  // F:21354
  check_bc_compatible(BC_P_, BC_Q_, Emax, Smax);
  FG_HIP_CHECK(hipMemsetAsync(eps_, 0, 6 * (size_t)g_.n * sizeof(double), stream_));  // F:21379
  pol_state_ = false;
  u_valid_ = false;
  eps_stale_ = false;
  // converged strain fields of the last steps (device copies, oldest first)  F:21586
  struct Kept {
    double t;
    double* eps;
  };
  std::vector<Kept> last;
  struct Release {
    std::vector<Kept>& v;
    ~Release() {
      for (Kept& k : v) (void)hipFree(k.eps);
    }
  } release{last};
  const size_t f6 = 6 * (size_t)g_.n * sizeof(double);
  for (int istep = first; istep < nparams; ++istep) {
    double E[6], S[6];
    load_step_values(params[istep], Emax, Smax, E, S);
    fresh_step_ = istep == first;
    const int order = opt_.loadstep_extrapolation_order;
    if (order > 0 && istep > first) {   // F:21634-21650
      if (slab_layout_) throw std::runtime_error("load-step extrapolation is not available on slab-decomposed solvers");
      double* buf = nullptr;
      while ((int)last.size() > order) {   // the oldest buffer is reused for the new copy
        if (buf) FG_HIP_CHECK(hipFree(buf));
        buf = last.front().eps;
        last.erase(last.begin());
      }
      if (!buf) FG_HIP_CHECK(hipMalloc(&buf, f6));
      ensure_eps();
      FG_HIP_CHECK(hipMemcpyAsync(buf, eps_, f6, hipMemcpyDeviceToDevice, stream_));
      last.push_back(Kept{params[istep - 1], buf});
      const int n = (int)last.size();
      if (n >= 2) {
        double t[8], w[8];
        for (int i = 0; i < n; ++i) t[i] = last[i].t;
        if (!extrapolation_weights(t, n, params[istep], w)) throw std::runtime_error("Error inverting Vandermonde matrix");   // F:21487-21490
        const double* in[8];
        for (int i = 0; i < n; ++i) in[i] = last[i].eps;
        launch_lincomb(n, in, w, eps_, 6 * g_.n, stream_);
        u_valid_ = false;      // the state is the extrapolated strain field: one strain-state pass, then the displacement loop
        eps_stale_ = false;
      }
    }
    if (run_one_step(E, S)) return true;
    if (step_cb && step_cb(user, istep)) return true;   // "Loadstep callback break request."
  }
  return false;
}

// runSolver  F:21400-21433 for one load step
bool Solver::run_one_step(const double* E0, const double* S0) {
  require_plan(plan::Entry::Run);
  // EpsilonErrorEstimator  F:14591-14637: constructed on the field the step starts from (zero for the first step)
  const double prev0 = fresh_step_ ? 0.0 : current_norm9();
  if (opt_.error_estimator >= 2) estimator_begin(fresh_step_);
  if (opt_.method == 1 && opt_.mode == 1) return run_cg_scalar(E0, prev0);
  if (opt_.method == 1) return run_cg(E0, S0, prev0);
  if (opt_.method == 2) return run_polarization(E0, S0, prev0);
  const double t_start = now_seconds();
  for (int i = 0; i < 6; ++i) F00_[i] = 0.0;
  // Displacement-based loop: eps_0 = 0 gives tau = 0, u_1 = 0 and eps_1 = E, so the loop starts from
  // u = 0 and every pass is [u_k -> norms of eps_k, f_{k+1}] + [f_{k+1} -> u_{k+1}] (see u_pass_front).
  const bool uloop = plan::plan_sweeps(plan_input(plan::Entry::Run, 1)).u_loop;
  const bool mixed_bc = this->mixed_bc();   // (NaN until calcRefMaterial ran: Q != 0)
  if (uloop && fresh_step_) {
    FG_HIP_CHECK(hipMemsetAsync(fu_, 0, 3 * g_.n * sizeof(double), stream_));
    u_valid_ = true;
    eps_stale_ = true;
    for (int i = 0; i < 6; ++i) E_cur_[i] = E0[i];
  }
  in_run_ = true;
  pending_back_ = back_ready_ = false;

  StopRule rule = stop_rule(prev0);
  const double nglobal = (double)nglobal_;
  BasicLoopOps ops;   // the iteration itself: fg_basic_loop.h
  ops.refresh_ref = [&](double* E) {
    calc_ref_material();
    bc_mean(BC_QC0_, BC_M_, opt_.bc_relax, E0, S0, E);
  };
  ops.have_u = [&] { return u_valid_; };
  ops.mixed_bc = [&] { return mixed_bc; };   // as read before the reference material was refreshed
  ops.start_from = [&](const double* E) {
    for (int i = 0; i < 6; ++i) E_cur_[i] = E[i];
  };
  ops.carry_pass = [&](const double* E) {
    u_pass_front(E);
    u_pass_back();
  };
  ops.u_pass = [&](const double* E, bool) {   // (the sweep plan has asked mixed_bc() itself)
    u_pass_front(E);
    if (opt_.mode == 1 && mixed_bc && !sc_tau_sums_) {
      // heat / porous with mixed boundary conditions (initBCProjector in GammaOperatorStaggeredHeat F:20342-20350): the
      // LDS-tiled sweep leaves the sums of tau in kSlotMean; where it does not apply, <tau> = <P(g) - 2 mu0 g> is taken
      // from the gradient field (two extra sweeps per pass)
      ensure_eps();
      launch_sc_flux_mean(g_, scalar_params(opt_.mu_0, 1.0 / (double)nglobal_), ptrs3(eps_), phase_ptrs(), partial_,
                          dscal_ + kSlotMean, stream_);
      eps_stale_ = true;
    }
    pending_back_ = true;   // fetch_norms_and_errors enqueues the FFT chain behind the copies
  };
  ops.strain_pass = [&](const double* E, bool) { basic_scheme(E); };
  ops.wait = [&] { fetch_norms_and_errors("stress"); };
  ops.mq_mean_tau = [&](double* t6) {
    double F0[6];
    for (int c = 0; c < 6; ++c) F0[c] = hscal_[kSlotMean + c] / nglobal;
    if (opt_.mode == 1)   // components 3..5 do not exist; the flux-mean sweep has divided by N already, the tiled sweep has not
      for (int c = 0; c < 6; ++c) F0[c] = c < 3 ? hscal_[kSlotMean + c] / (sc_tau_sums_ ? nglobal : 1.0) : 0.0;
    if (opt_.mixing == kMixLaminate)
      for (int c = 0; c < 6; ++c) F0[c] += hscal_[kSlotScratch + c] / nglobal;
    voigt_mv(BC_MQ_, F0, t6);
  };
  ops.norm = [&] {
    for (int c = 0; c < 6; ++c) sumsq_[c] = hscal_[kSlotSumSq + c];
    return norm9_of_sums(sumsq_, nglobal);
  };
  ops.estimator = [&](StopRule& r) {
    if (opt_.error_estimator >= 2) estimator_update(&r.abs_err, &r.rel_err);
  };
  ops.bc_ok = [&] { return bc_error(E0, S0) <= opt_.bc_tol; };
  ops.adopt = [&](const double* E_next) {
    for (int c = 0; c < 6; ++c) E_next_[c] = E_next[c];
    adopt_back();
  };
  const BasicResult end = basic_loop(*this, ops, rule, E0, fresh_step_, uloop, opt_.update_ref != 0);
  pending_back_ = back_ready_ = false;
  in_run_ = false;
  iterations_ = end.iter;
  ensure_eps();
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  solve_time_ += now_seconds() - t_start;
  return end.failed;
}

// ------------------------------------------------------------------ the polarisation loop
// method "polarization": Eyre & Milton's scheme as runPolarization F:21808-21851 drives it.  The state is the polarisation
// P = (C + C0) : eps with C0 = 2 mu_0 Id, held in eps_ (pol_state_); one pass is polarizationScheme F:20536-20554:
//   Q = (C - C0)(C + C0)^-1 P per voxel,  P00 = <Q>,  P_hat = -4 mu_0 Gamma0_hat : Q_hat + Q_hat,  P_hat(0) = P00 + 4 mu_0 E.
void Solver::polar_start(const double* E6) {
  Vec6 P0;
  for (int c = 0; c < 6; ++c) P0.v[c] = 4 * opt_.mu_0 * E6[c];
  launch_set_const6(g_, ptrs6(eps_), P0, stream_);   // epsilon.setConstant(4 mu_0 E)  F:21828
  pol_mu0_ = opt_.mu_0;
  pol_state_ = true;
  u_valid_ = false;
  eps_stale_ = false;
}

void Solver::polar_pass(const double* E6) {
  if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
  const double mu_0 = opt_.mu_0, alpha = -4 * mu_0;   // GammaOperator(P00 + P0, ..., -4 mu_0, 1)  F:20553
  Vec6 P0;
  for (int c = 0; c < 6; ++c) P0.v[c] = 4 * mu_0 * E6[c];   // F:21836
  double* sums = dscal_ + kSlotPolar;
  time_begin(0);
  launch_polarize(g_, phase_table(), mu_0, false, ptrs6(eps_), phase_ptrs(), ptrs6(tau_), partial_, sums, stream_);
  time_end(0);
  if (opt_.gamma_scheme == 0) {
    // the consistent staggered form (SolverOptions::method): u = -4 mu_0 G0 div_h Q, P = Q + sym grad_h u + P0; <Q> passes through
    time_begin(1);
    launch_div(g_, ptrs6(tau_), ptrs3(fu_), kNoXHalo, stream_);
    time_end(1);
    fft_g0_chain(fu_, alpha, nullptr, nullptr);   // (Q stays in tau_: no scratch for the x-contiguous layout)
    time_begin(9);
    launch_polar_back(g_, ptrs3(fu_), ptrs6(tau_), ptrs6(eps_), P0, partial_, dscal_ + kSlotSumSq, stream_);
    time_end(9);
  } else {
    const GammaHat op = {willot(), mu_0, opt_.lambda_0, alpha, 1.0, P0, false, sums, 1 / (double)nglobal_};
    fourier_pass6(op, eps_);
  }
  pass_done(E6, eps_, false);
  pol_state_ = true;
}

void Solver::polar_settle() {
  if (!pol_state_) return;
  FG_HIP_CHECK(hipSetDevice(device_));
  polar_to_strain();
}

void Solver::polar_to_strain() {
  launch_polarize(g_, phase_table(), pol_mu0_, true, ptrs6(eps_), phase_ptrs(), ptrs6(eps_), partial_, nullptr, stream_);
  pol_state_ = false;
  u_valid_ = false;
  eps_stale_ = false;
}

// runPolarization  F:21808-21851 for one load step.  The estimator watches the polarisation field (ee->update() on it), the
// boundary-condition check is off (check_bc = false F:21819).  The reference never advances its iteration counter in this loop
// (so its maxiter cannot end it); here the counter runs like in every other loop.
bool Solver::run_polarization(const double* E0, const double* S0, double prev0) {
  const double t_start = now_seconds();
  for (int i = 0; i < 6; ++i) F00_[i] = 0.0;
  if (opt_.update_ref != 0) calc_ref_material();   // F:21823-21825
  double E[6];
  bc_mean(BC_QC0_, BC_M_, opt_.bc_relax, E0, S0, E);   // F:21826
  polar_start(E);
  pending_back_ = back_ready_ = false;
  in_run_ = true;
  StopRule rule = stop_rule(prev0);
  long iter = 1;
  bool failed = false;
  for (;;) {
    polar_pass(E);
    fetch_norms_and_errors("polarization");
    for (int c = 0; c < 6; ++c) sumsq_[c] = hscal_[kSlotSumSq + c];
    rule.measure(norm9_of_sums(sumsq_, (double)nglobal_));
    if (opt_.error_estimator >= 2) estimator_update(&rule.abs_err, &rule.rel_err);   // none
    if (converged(rule, iter, [] { return true; }, &failed)) break;
    iter++;
  }
  in_run_ = false;
  iterations_ = iter;
  ensure_eps();   // calcPolarization(..., inv = true)  F:21850
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
  solve_time_ += now_seconds() - t_start;
  return failed;
}

// ------------------------------------------------------------------ conjugate gradients
// runCGElasticity  F:23153-23247 on the operator  eps -> -Gamma0 : (C - C0) : eps  (krylovOperator
// F:20583-20587 = one basicScheme pass with E = 0), l2 inner product, epsilon error estimator.
// The same iteration carried in displacement space (see k_cgu_dot): eps = E + grad_s u_e, r / p / w = grad_s u_r / u_p / u_w.
//   u_e = fu_ (so the strain is materialised from it afterwards), u_w = fu_alt_ (output of the FFT chain),
//   u_r, u_p = the two halves of the 6-component buffer cg_r_.  The iteration itself: cg_pipelined (fg_cg_loop.h).
bool Solver::run_cg_u(const double* E0, double prev0) {
  const double t_start = now_seconds();
  const size_t f3 = 3 * (size_t)g_.n * sizeof(double);
  if (!cg_r_) FG_HIP_CHECK(hipMalloc(&cg_r_, 2 * f3));
  double* u_r = cg_r_;
  double* u_p = cg_r_ + 3 * g_.n;
  // Fused form (option cg_fused, default where the tiled sweep fits; Voigt mixing): the vector work of an iteration is two
  // tiled sweeps instead of four kernels -- p:(p - w) (launch_cgu_tile mode 0), and the update of eps and r together with the
  // norms of the new eps and r:r (mode 1) -- and the direction update p = r + beta p is formed inside the operator's
  // displacement sweep (launch_u_tile_cg).  Updates are out of place (the tiles' halo rows re-evaluate them), so u_e, u_r and
  // u_p alternate between two buffers each; fu_ stays the current iterate.
  const plan::SweepPlan sweeps = plan::plan_sweeps(plan_input(plan::Entry::Run, 2));
  bool fused = sweeps.cg_fused_wanted;
  if (fused && (!cg_p_ || !fu_cg_)) {
    // nine more components (the alternates of u_e, u_r, u_p): on grids that fill the card (1024^3: 78 GB) the four-kernel form
    size_t free_b = 0, total_b = 0;
    FG_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t need = (cg_p_ ? 0 : 2 * f3) + (fu_cg_ ? 0 : f3);
    if (free_b < need + (size_t)(0.02 * (double)total_b)) fused = false;
  }
  const bool fused_dir = fused && sweeps.cg_fused_dir;   // laminate mixing: the interface kernels read u_p as a stored field
  double *r_alt = nullptr, *p_alt = nullptr;
  if (fused) {
    if (!cg_p_) FG_HIP_CHECK(hipMalloc(&cg_p_, 2 * f3));
    if (!fu_cg_) FG_HIP_CHECK(hipMalloc(&fu_cg_, f3));
    r_alt = cg_p_;
    p_alt = cg_p_ + 3 * g_.n;
  }
  for (int i = 0; i < 6; ++i) F00_[i] = 0.0;
  in_run_ = true;
  cg_u_active_ = true;
  const double small = std::numeric_limits<double>::min();
  if (opt_.update_ref) calc_ref_material();
  Vec6 E, Z;
  for (int i = 0; i < 6; ++i) E.v[i] = E0[i], Z.v[i] = 0.0;   // Q = 0: calcBCMean leaves E0
  auto apply = [&](double* u_in, const double* Eadd) { cg_apply(u_in, Eadd, tau_); };
  // fused form: u_p := u_r + beta u_p (beta from the sums at dscal_[i_num] / dscal_[i_den]) inside the sweep of the operator
  auto apply_dir = [&](int i_num, int i_den) {
    using plan::Front;
    const PhaseTable t = phase_table();
    const double tiny = std::numeric_limits<double>::min();
    FieldPtrs<2> ph;   // two complementary phases: the sweep reads phi_1
    ph.p[0] = phi_ + g_.n;
    ph.p[1] = nullptr;
    time_begin(0);
    switch (sweeps.cg_dir) {
      case Front::UTileDfg:
        launch_u_tile_cg(g_, opt_.mu_0, opt_.lambda_0, ptrs3(u_p), ptrs3(u_r), ptrs3(p_alt), dfg_moduli(), ptrs3(fu_alt_), Z, dscal_, i_num,
                         i_den, (double)nglobal_, tiny, partial_, dscal_ + kSlotSumSq, stream_);
        cg_dir_sweep_ = (long)Front::UTileDfg;
        break;
      case Front::UTileAniso:
        launch_u_tile_aniso_cg(g_, opt_.mu_0, opt_.lambda_0, ptrs3(u_p), ptrs3(u_r), ptrs3(p_alt), phi_ + g_.n, ptrs3(fu_alt_), Z, dscal_,
                               i_num, i_den, (double)nglobal_, tiny, partial_, dscal_ + kSlotSumSq, stream_, t);
        ++u_tile_aniso_;
        cg_dir_sweep_ = (long)Front::UTileAniso;
        break;
      case Front::UTilePhi:
        launch_u_tile_cg(g_, opt_.mu_0, opt_.lambda_0, ptrs3(u_p), ptrs3(u_r), ptrs3(p_alt), ph, ptrs3(fu_alt_), Z, dscal_, i_num, i_den,
                         (double)nglobal_, tiny, partial_, dscal_ + kSlotSumSq, stream_, &t);
        cg_dir_sweep_ = (long)Front::UTilePhi;
        break;
      case Front::UTileModuli:   // (Reuss mixing: the CG sweep reads the moduli arrays)
        launch_u_tile_cg(g_, opt_.mu_0, opt_.lambda_0, ptrs3(u_p), ptrs3(u_r), ptrs3(p_alt), effective_moduli(), ptrs3(fu_alt_), Z, dscal_,
                         i_num, i_den, (double)nglobal_, tiny, partial_, dscal_ + kSlotSumSq, stream_, nullptr);
        cg_dir_sweep_ = (long)Front::UTileModuli;
        break;
      default:
        throw std::logic_error("run_cg_u: no direction sweep for this configuration");
    }
    time_end(0);
    fft_g0_chain(fu_alt_, -1.0, nullptr, tau_);
    std::swap(u_p, p_alt);
  };
  // eps_0 = E (u_e = 0);  r = -Gamma0 (C - C0) E  (+ E - eps_0 = 0, adjustResidual F:10012-10022)
  // The CG scalars stay on the device: k_cgu_axpy forms alpha and beta from the sums the dot sweeps leave in dscal_ (cg_pipelined).
  const CgSlots slot = cg_slots(kSlotCg);
  const double nvox = (double)nglobal_;
  FG_HIP_CHECK(hipMemsetAsync(fu_, 0, f3, stream_));
  apply(fu_, E.v);
  FG_HIP_CHECK(hipMemcpyAsync(u_r, fu_alt_, f3, hipMemcpyDeviceToDevice, stream_));
  FG_HIP_CHECK(hipMemcpyAsync(u_p, fu_alt_, f3, hipMemcpyDeviceToDevice, stream_));   // p = r
  launch_cgu_dot(1, g_, ptrs3(fu_), ptrs3(u_r), E, partial_, dscal_ + slot.blk[0], stream_);   // gamma_0 = r:r / N + tiny
  double gamma_0 = 0.0;   // r:r / N + tiny at the start: only the residual estimator reads it
  if (opt_.error_estimator == 1) {
    FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotCg + 6, dscal_ + slot.rr(0), sizeof(double), hipMemcpyDeviceToHost, stream_));
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    gamma_0 = hscal_[kSlotCg + 6] / (double)nglobal_ + small;
  }
  StopRule rule = stop_rule(prev0, gamma_0);
  const double S_zero[6] = {0, 0, 0, 0, 0, 0};
  CgPipelinedOps ops;
  ops.fused_dir = fused_dir;
  ops.apply_p = [&] { apply(u_p, Z.v); };   // u_w = operator(u_p)
  ops.apply_dir = apply_dir;
  ops.direction = [&](int num, int den) {   // p = r + beta p (beta = delta / gamma)
    launch_cgu_axpy(1, g_, ptrs3(fu_), ptrs3(u_p), ptrs3(u_r), ptrs3(fu_alt_), dscal_, num, den, nvox, small, stream_);
  };
  ops.dot_pw = [&](int out) {   // p : (p - w)
    if (fused)
      launch_cgu_tile(0, g_, ptrs3(u_p), ptrs3(fu_alt_), ptrs3(u_p), ptrs3(fu_alt_), ptrs3(fu_cg_), ptrs3(r_alt), Z, dscal_, 0, 0, nvox,
                      small, partial_, dscal_ + out, stream_);
    else
      launch_cgu_dot(0, g_, ptrs3(u_p), ptrs3(fu_alt_), Z, partial_, dscal_ + out, stream_);
  };
  ops.update = [&](int gamma, int pw, int out) {   // eps += alpha p ; r -= alpha (p - w), with the norms of the new eps and r : r
    if (fused) {   // into the alternate buffers
      launch_cgu_tile(1, g_, ptrs3(fu_), ptrs3(u_r), ptrs3(u_p), ptrs3(fu_alt_), ptrs3(fu_cg_), ptrs3(r_alt), E, dscal_, gamma, pw, nvox,
                      small, partial_, dscal_ + out, stream_);
      std::swap(fu_, fu_cg_);
      std::swap(u_r, r_alt);
    } else {
      launch_cgu_axpy(0, g_, ptrs3(fu_), ptrs3(u_p), ptrs3(u_r), ptrs3(fu_alt_), dscal_, gamma, pw, nvox, small, stream_);
      launch_cgu_dot(1, g_, ptrs3(fu_), ptrs3(u_r), E, partial_, dscal_ + out, stream_);
    }
  };
  ops.sums = [&] {
    cg_set_state(E);   // eps = E + grad_s fu_
    return CgSums{norm9_of_sums(cg_sumsq(6), nvox), hscal_[kSlotCg + 6]};
  };
  ops.bc_ok = [&] { return bc_error(E0, S_zero) <= opt_.bc_tol; };
  const CgResult end = cg_pipelined(*this, ops, rule, slot, nvox);
  cg_finish(end.iter, t_start, &E);
  return end.failed;
}

// Scalar modes: the same CG in potential space (g = E + grad T_e; r, p, w = grad T_r, T_p, T_w): runCG dispatches every
// non-hyperelastic mode to runCGElasticity (F:22056-22066), whose inner product is the plain sum for 3 components
// (F:20961-20980).  T_e = fu_[0], T_w = fu_alt_[0], T_r / T_p = components 1, 2 of fu_alt_'s buffer mate cg_r_.
bool Solver::run_cg_scalar(const double* E0, double prev0) {
  const double t_start = now_seconds();
  const size_t f1 = (size_t)g_.n * sizeof(double);
  if (!cg_r_) FG_HIP_CHECK(hipMalloc(&cg_r_, 6 * f1));
  double* T_r = cg_r_;
  double* T_p = cg_r_ + g_.n;
  in_run_ = true;
  cg_u_active_ = true;
  const double small = std::numeric_limits<double>::min();
  if (opt_.update_ref) calc_ref_material();
  Vec6 E, Z;
  for (int i = 0; i < 6; ++i) E.v[i] = i < 3 ? E0[i] : 0.0, Z.v[i] = 0.0;
  const double S_zero[6] = {0, 0, 0, 0, 0, 0};
  auto apply = [&](double* T_in, const double* Eadd) { cg_apply(T_in, Eadd, nullptr); };
  FG_HIP_CHECK(hipMemsetAsync(fu_, 0, f1, stream_));
  apply(fu_, E.v);
  FG_HIP_CHECK(hipMemcpyAsync(T_r, fu_alt_, f1, hipMemcpyDeviceToDevice, stream_));
  FG_HIP_CHECK(hipMemcpyAsync(T_p, fu_alt_, f1, hipMemcpyDeviceToDevice, stream_));
  // Fused form (option cg_fused; as in run_cg_u, cg_pipelined with the direction inside the operator's sweep).  Out of place:
  // T_e, T_r, T_p alternate between two components each (the spare components of fu_ and cg_r_).  Not with a convergence
  // callback (accessors read fu_'s first component in between).
  const double nvox = (double)nglobal_;
  const plan::SweepPlan sweeps = sweep_plan();
  const bool aniso = sweeps.cg_dir == plan::Front::ScTileAniso;   // the fused form needs the tiled sweep: for aniso phases its two-phase form
  if (sweeps.cg_fused_wanted && !cb_) {
    const CgSlots slot = cg_slots(kSlotCg);
    double *e_cur = fu_, *e_alt = fu_ + g_.n, *r_cur = T_r, *r_alt = cg_r_ + 2 * g_.n, *p_cur = T_p, *p_alt = cg_r_ + 3 * g_.n;
    const double* cond = aniso ? nullptr : effective_moduli().p[0];
    double K0[6], K1[6];
    if (aniso) sc_aniso_constants(K0, K1);
    launch_sc_cg_dot(1, g_, e_cur, r_cur, E, partial_, dscal_ + slot.blk[0], stream_);   // gamma_0 = r.r / N + tiny
    FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotCg + 6, dscal_ + slot.rr(0), sizeof(double), hipMemcpyDeviceToHost, stream_));
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    check_device_error("cg");
    StopRule rule = stop_rule(prev0, hscal_[kSlotCg + 6] / nvox + small);
    CgPipelinedOps ops;
    ops.fused_dir = true;
    ops.apply_p = [&] { apply(p_cur, Z.v); };
    ops.apply_dir = [&](int num, int den) {   // T_p := T_r + beta T_p inside the sweep; T_w = operator(T_p)
      time_begin(0);
      if (aniso) {
        launch_sc_tile_aniso(g_, opt_.mu_0, K0, K1, p_cur, phi_ + g_.n, fu_alt_, Z, partial_, dscal_ + kSlotSumSq, stream_, r_cur, p_alt,
                             dscal_, num, den, nvox, small);
        ++sc_tile_aniso_;
        cg_dir_sweep_ = (long)plan::Front::ScTileAniso;
      } else {
        launch_sc_sweep_cg(g_, opt_.mu_0, p_cur, r_cur, p_alt, cond, fu_alt_, Z, dscal_, num, den, nvox, small, partial_,
                           dscal_ + kSlotSumSq, stream_);
        cg_dir_sweep_ = (long)plan::Front::ScFast;
      }
      time_end(0);
      fft_g0_chain(fu_alt_);
      std::swap(p_cur, p_alt);
    };
    ops.dot_pw = [&](int out) {
      launch_sc_cgu_tile(0, g_, p_cur, fu_alt_, p_cur, fu_alt_, e_alt, r_alt, Z, dscal_, 0, 0, nvox, small, partial_, dscal_ + out,
                         stream_);
    };
    ops.update = [&](int gamma, int pw, int out) {
      launch_sc_cgu_tile(1, g_, e_cur, r_cur, p_cur, fu_alt_, e_alt, r_alt, E, dscal_, gamma, pw, nvox, small, partial_, dscal_ + out,
                         stream_);
      std::swap(e_cur, e_alt);
      std::swap(r_cur, r_alt);
    };
    ops.sums = [&] { return CgSums{norm3_of_sums(cg_sumsq(3), nvox), hscal_[kSlotCg + 6]}; };
    ops.bc_ok = [&] {
      // bc_error reads the strain of the current iterate: fu_'s first component must be it
      if (e_cur != fu_) {
        FG_HIP_CHECK(hipMemcpyAsync(fu_, e_cur, f1, hipMemcpyDeviceToDevice, stream_));
        std::swap(e_cur, e_alt);
      }
      cg_set_state(E);
      return bc_error(E.v, S_zero) <= opt_.bc_tol;
    };
    const CgResult end = cg_pipelined(*this, ops, rule, slot, nvox);   // (cb_ is not set in this form: every iteration runs ahead)
    if (e_cur != fu_) FG_HIP_CHECK(hipMemcpyAsync(fu_, e_cur, f1, hipMemcpyDeviceToDevice, stream_));
    in_run_ = false;
    cg_finish(end.iter, t_start, &E);
    return end.failed;
  }
  launch_sc_cg_dot(1, g_, fu_, T_r, E, partial_, dscal_ + kSlotSumSq, stream_);
  cg_fetch_now(kSlotSumSq, 7);
  StopRule rule = stop_rule(prev0, hscal_[kSlotSumSq + 6] / nvox + small);
  double& gamma = rule.gamma_cur;
  long iter = 0;
  bool failed = false;
  for (;;) {   // alpha and beta on the host
    apply(T_p, Z.v);
    launch_sc_cg_dot(0, g_, T_p, fu_alt_, Z, partial_, dscal_ + kSlotMean, stream_);
    const double alpha = gamma / (cg_fetch_now(kSlotMean, 1) / nvox + small);
    launch_sc_cg_axpy(0, g_, fu_, T_p, T_r, fu_alt_, alpha, stream_);
    launch_sc_cg_dot(1, g_, fu_, T_r, E, partial_, dscal_ + kSlotSumSq, stream_);
    cg_fetch_now(kSlotSumSq, 7);
    const double rr = hscal_[kSlotSumSq + 6];
    cg_set_state(E);
    for (int c = 0; c < 6; ++c) sumsq_[c] = c < 3 ? hscal_[kSlotSumSq + c] : 0.0;
    rule.measure(norm3_of_sums(sumsq_, nvox));
    if (converged(rule, iter, [&] { return bc_error(E.v, S_zero) <= opt_.bc_tol; }, &failed)) break;
    iter++;
    const double delta = rr / nvox + small;
    const double beta = delta / gamma;
    gamma = delta;
    launch_sc_cg_axpy(1, g_, fu_, T_p, T_r, fu_alt_, beta, stream_);
  }
  in_run_ = false;
  cg_finish(iter, t_start, &E);
  return failed;
}

bool Solver::run_cg(const double* E0, const double* S0, double prev0) {
  // (prescribed stresses run in strain space, like the estimators that measure a mean of the strain field)
  if (plan::plan_sweeps(plan_input(plan::Entry::Run, 1)).cg == plan::Cg::DisplacementSpace && norm2(S0, 6) == 0.0) return run_cg_u(E0, prev0);
  const double t_start = now_seconds();
  const size_t f6 = 6 * (size_t)g_.n * sizeof(double);
  for (double** b : {&cg_r_, &cg_p_, &cg_w_})
    if (!*b) FG_HIP_CHECK(hipMalloc(b, f6));
  for (int i = 0; i < 6; ++i) F00_[i] = 0.0;
  u_valid_ = false;
  eps_stale_ = false;
  in_run_ = true;
  const double small = std::numeric_limits<double>::min();
  if (opt_.update_ref) calc_ref_material();
  Vec6 E, Z;
  bc_mean(BC_QC0_, BC_M_, opt_.bc_relax, E0, S0, E.v);
  for (int i = 0; i < 6; ++i) Z.v[i] = 0.0;
  const FieldPtrs<6> e = ptrs6(eps_), r = ptrs6(cg_r_), p = ptrs6(cg_p_), w = ptrs6(cg_w_);
  launch_set_const6(g_, e, E, stream_);
  basic_scheme(Z.v, eps_, cg_r_);                                                  // r = -Gamma0 (C - C0) eps
  launch_cg(0, g_, r, e, e, E, 0.0, partial_, dscal_ + kSlotMean, stream_);        // r += E - eps ; r:r
  StopRule rule = stop_rule(prev0, cg_fetch_now(kSlotMean, 1) / (double)nglobal_ + small);   // gamma_0 = r:r / N + tiny
  FG_HIP_CHECK(hipMemcpyAsync(cg_p_, cg_r_, f6, hipMemcpyDeviceToDevice, stream_));  // p = r
  // option cg_fused (cg_pipelined): the updates of eps and r as ONE sweep with their norms -- one host synchronisation per
  // iteration instead of three, 528 instead of 576 bytes per voxel of vector work; otherwise cg_host_scalars
  const double nvox = (double)nglobal_;
  auto bc_ok = [&] { return bc_error(E0, S0) <= opt_.bc_tol; };
  if (opt_.cg_fused != 0) {
    const CgSlots slot = cg_slots(kSlotCg);
    FG_HIP_CHECK(hipMemcpyAsync(dscal_ + slot.rr(0), dscal_ + kSlotMean, sizeof(double), hipMemcpyDeviceToDevice, stream_));   // gamma_0
    CgPipelinedOps ops;
    ops.apply_p = [&] { basic_scheme(Z.v, cg_p_, cg_w_); };   // w = -Gamma0 (C - C0) p
    ops.direction = [&](int num, int den) { launch_cg_dev(6, g_, e, r, p, w, dscal_, num, den, nvox, small, partial_, nullptr, stream_); };
    ops.dot_pw = [&](int out) { launch_cg(1, g_, p, w, w, E, 0.0, partial_, dscal_ + out, stream_); };   // p:(p - w)
    ops.update = [&](int gamma_slot, int pw, int out) {   // eps += alpha p ; r -= alpha (p - w) ; norms of eps ; r:r
      launch_cg_dev(5, g_, e, r, p, w, dscal_, gamma_slot, pw, nvox, small, partial_, dscal_ + out, stream_);
    };
    ops.sums = [&] { return CgSums{norm9_of_sums(cg_sumsq(6), nvox), hscal_[kSlotCg + 6]}; };
    if (opt_.error_estimator >= 2)   // update_cg -> update  F:14465, F:14584
      ops.estimator = [&](StopRule& r) { estimator_update(&r.abs_err, &r.rel_err); };
    ops.bc_ok = bc_ok;
    const CgResult end = cg_pipelined(*this, ops, rule, slot, nvox);
    in_run_ = false;
    cg_finish(end.iter, t_start, nullptr);
    return end.failed;
  }
  double& gamma = rule.gamma_cur;
  long iter = 0;
  bool failed = false;
  for (;;) {   // alpha and beta on the host
    basic_scheme(Z.v, cg_p_, cg_w_);                                               // w = -Gamma0 (C - C0) p
    launch_cg(1, g_, p, w, w, E, 0.0, partial_, dscal_ + kSlotMean, stream_);      // p:(p - w)
    const double alpha = gamma / (cg_fetch_now(kSlotMean, 1) / nvox + small);
    launch_cg(2, g_, e, p, p, E, alpha, partial_, dscal_ + kSlotSumSq, stream_);   // eps += alpha p ; norms
    cg_fetch_now(kSlotSumSq, 6);
    for (int c = 0; c < 6; ++c) sumsq_[c] = hscal_[kSlotSumSq + c];
    rule.measure(norm9_of_sums(sumsq_, nvox));
    if (opt_.error_estimator >= 2) estimator_update(&rule.abs_err, &rule.rel_err);   // update_cg -> update  F:14465, F:14584
    if (converged(rule, iter, bc_ok, &failed)) break;
    iter++;
    launch_cg(3, g_, r, p, w, E, -alpha, partial_, dscal_ + kSlotMean, stream_);   // r -= alpha (p - w) ; r:r
    const double delta = cg_fetch_now(kSlotMean, 1) / nvox + small;
    const double beta = delta / gamma;
    gamma = delta;
    launch_cg(4, g_, p, r, r, E, beta, partial_, dscal_ + kSlotMean, stream_);     // p = r + beta p
  }
  in_run_ = false;
  cg_finish(iter, t_start, nullptr);
  return failed;
}

// ------------------------------------------------------------------ stages and fields
void Solver::run_stage(int stage, const double* E6) {
  FG_HIP_CHECK(hipSetDevice(device_));
  if (opt_.mode == 1) {
    if (stage != kStageIteration) throw std::runtime_error("single stages are not available in heat / porous mode");
    iterate(E6, 1);
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    return;
  }
  ensure_eps();
  if (stage != kStageIteration) u_valid_ = false;  // the stage buffers are being used as scratch
  const double zero6[6] = {0, 0, 0, 0, 0, 0};
  const double* E = E6 ? E6 : zero6;
  switch (stage) {
    case kStageStress:
      if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
      stress_to_tau(stress_params(opt_.mu_0, opt_.lambda_0, 1.0), eps_);
      check_device_error("stress");
      break;
    case kStageStressConst:
      launch_stress_const(g_, opt_.mu_0, opt_.lambda_0, ptrs6(eps_), ptrs6(tau_), stream_);
      break;
    case kStageDiv:
      launch_div(g_, ptrs6(tau_), ptrs3(fu_), kNoXHalo, stream_);
      break;
    case kStageFftForward:
      fft_->forward(fu_, 3, g_.n, 1 / (double)nglobal_);
      break;
    case kStageG0: {
      const double alpha = E6 ? E6[0] : -1.0;  // stage tests pass alpha in E6[0]
      const double c10 = -alpha / (opt_.mu_0);
      const double c20 = -alpha / (opt_.mu_0 * (1 + opt_.mu_0 / (opt_.lambda_0 + opt_.mu_0)));
      G0Tables tb;
      for (int a = 0; a < 3; ++a) {
        tb.kpm[a] = g0_kpm_[a];
        tb.kp[a] = g0_kp_[a];
      }
      launch_g0(g_, ptrs3(fu_), tb, c10, c20, G0Layout{0, 0, 0}, stream_);
      break;
    }
    case kStageFftInverse:
      fft_->inverse(fu_, 3, g_.n);
      break;
    case kStageEps: {
      Vec6 Ev, R;
      for (int c = 0; c < 6; ++c) Ev.v[c] = E[c], R.v[c] = 0.0;
      launch_eps_norm(g_, ptrs3(fu_), ptrs6(eps_), Ev, R, false, partial_, dscal_ + kSlotSumSq,
                      kNoXHalo, stream_);
      FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotSumSq, dscal_ + kSlotSumSq, 6 * sizeof(double), hipMemcpyDeviceToHost, stream_));
      FG_HIP_CHECK(hipStreamSynchronize(stream_));
      for (int c = 0; c < 6; ++c) sumsq_[c] = hscal_[kSlotSumSq + c];
      break;
    }
    case kStageIteration:
      basic_scheme(E);
      check_device_error("stress");
      break;
    default:
      throw std::runtime_error("unknown stage");
  }
  FG_HIP_CHECK(hipStreamSynchronize(stream_));
}

int Solver::field_components(const std::string& name) const {
  if (opt_.mode == 1) {
    if (name == "epsilon" || name == "sigma") return 3;
    if (name == "u") return 1;
    if (name == "phi") return pt_.n;
    if (name == "sumsq") return 6;
    return 0;
  }
  if (name == "epsilon" || name == "sigma" || name == "tau" || name == "polarization") return 6;
  if (name == "u" || name == "f" || name == "normals") return 3;
  if (name == "f_hat") return 3;
  if (name == "p") return opt_.mode == 2 ? 1 : 0;   // the pressure of the dual Stokes scheme
  if (name == "phi") return pt_.n;
  if (name == "sumsq") return 6;
  return 0;
}

double* Solver::device_component(const std::string& name, int c) {
  if (name == "epsilon" && c >= 0 && c < 6) return eps_ + (long)c * g_.n;
  if (name == "polarization" && pol_state_ && c >= 0 && c < 6) return eps_ + (long)c * g_.n;   // the state of method polarization
  if (name == "tau" && c >= 0 && c < 6) return tau_ + (long)c * g_.n;
  if ((name == "f" || name == "u" || name == "f_hat") && c >= 0 && c < 3) return fu_ + (long)c * g_.n;
  if (name == "phi" && c >= 0 && c < pt_.n) return phi_ + (long)c * g_.n;
  if (name == "normals" && normals_ && c >= 0 && c < 3) return normals_ + (long)c * g_.n;
  return nullptr;
}

// calcStressDiff(epsilon, sigma) F:18030-18033 + divOperatorStaggered(sigma, sigma): the body force both fields of the dual
// Stokes scheme start from, with the solver's mixing rule and under gamma_scheme 2 the five moduli (stress_to_tau).
// tau_ and fu_ hold nothing between passes in this mode (pass_viscosity rebuilds both from the strain state).
void Solver::viscosity_force(const char* what) {
  stress_to_tau(stress_params(opt_.mu_0, opt_.lambda_0, 1.0), eps_);
  check_device_error(what);
  launch_div(g_, ptrs6(tau_), ptrs3(fu_), kNoXHalo, stream_);
}

// poisson_solve  F:23462, 23471-23482: xi_a = (2 pi / n_a) * m, cos on the host with the libm call the reference makes per bin;
// built and uploaded by the first pressure accessor (the grid of a solver never changes)
PoissonTables Solver::poisson_tables() {
  const int len[3] = {g_.nx, g_.ny, g_.nz};
  for (int a = 0; a < 3; ++a) {
    if (poi_cs_[a]) continue;
    const int cnt = (a == 2) ? g_.nzc : len[a];
    std::vector<double> cs(cnt);
    const double xi_0 = 2.0 * M_PI / len[a];
    for (int m = 0; m < cnt; ++m) cs[m] = std::cos(xi_0 * m);
    FG_HIP_CHECK(hipMalloc(&poi_cs_[a], cnt * sizeof(double)));
    FG_HIP_CHECK(hipMemcpy(poi_cs_[a], cs.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
  }
  PoissonTables t;
  for (int a = 0; a < 3; ++a) t.cs[a] = poi_cs_[a];
  return t;
}

// get_raw_field("p")  F:15554-15573 / writeVTK F:23428-23434: laplace(p) = div(div(eta_0 (phi - phi_0) sigma_E)), solved by
// poisson_solve F:23454-23500.  The transforms are FFT3::forward / backward (F:7232-7244): FFTW's r2c and c2r, BOTH unnormalised,
// so the pair multiplies by nxyz and the symbol's c = 2 nxyz (F:23463) leaves p = L^-1 f with L the 7-point periodic Laplacian --
// restated as written: forward with scale 1, the division by c (...), inverse.
// The one-component forward / inverse pair of Fft3 is taken, not the fused chain of the loop: it leaves the spectrum in the
// canonical [nx][ny][nzc] layout on every route, which is what the symbol kernel indexes (an accessor, not the timed loop).
// Result: the first component of tau_, free once the divergence has consumed the polarisation.
void Solver::pressure() {
  viscosity_force("p");
  double* const p = tau_;
  launch_div_vector(g_, ptrs3(fu_), 1 / (2 * opt_.mu_0), p, stream_);   // (contains the multiplication with 2 eta_0  F:15564)
  const PoissonTables tb = poisson_tables();
  fft_->forward(p, 1, g_.n, 1.0);
  launch_poisson_symbol(g_, p, tb, stream_);
  fft_->inverse(p, 1, g_.n);
}

// get_raw_field  F:15396-15684 (epsilon, sigma, u, p, phi, normals) + raw stage buffers for the tests
void Solver::get_field(const std::string& name, double* out) {
  FG_HIP_CHECK(hipSetDevice(device_));
  if (name == "polarization" && opt_.mode != 1) {   // the raw state of method polarization between passes (fg_iterate); reading it keeps it
    if (!pol_state_) throw std::runtime_error("field 'polarization' exists only while method polarization holds its state (after fg_iterate)");
    download_unpadded(eps_, out, 6, g_.n);
    return;
  }
  if (name == "p") {   // the pressure exists in the dual Stokes scheme only (F:15554-15573 is written for mode viscosity)
    if (slab_layout_ && nranks_ > 1)   // (like "u": a lone slab holds the whole grid)
      throw std::runtime_error("field 'p' (a global Poisson solve) is not available on slab-decomposed solvers");
    if (opt_.mode != 2)
      throw std::runtime_error(std::string("field 'p' (the pressure) exists in mode viscosity only, not in mode ") +
                               (opt_.mode == 1 ? "heat / porous, whose potential is field 'u'" : "elasticity"));
  }
  ensure_eps();
  // fu_ is overwritten by the displacement reconstruction (scalar modes: by an equivalent potential, still valid;
  // displacement-space CG: the reconstruction goes to the free buffer fu_alt_, fu_ is the iterate itself)
  if (name == "u" && slab_layout_ && nranks_ > 1)
    throw std::runtime_error("field 'u' (a global reconstruction) is not available on slab-decomposed solvers");
  if ((name == "u" || name == "p") && opt_.mode != 1 && !cg_u_active_) u_valid_ = false;
  if (name == "sumsq") {  // the six sums of squares of the last norm sweep (device slot; the displacement loop keeps them there)
    FG_HIP_CHECK(hipMemcpyAsync(hscal_ + kSlotSumSq, dscal_ + kSlotSumSq, 6 * sizeof(double), hipMemcpyDeviceToHost, stream_));
    FG_HIP_CHECK(hipStreamSynchronize(stream_));
    for (int c = 0; c < 6; ++c) out[c] = sumsq_[c] = hscal_[kSlotSumSq + c];
    return;
  }
  if (name == "f_hat") {  // complex [3][nx][ny][nz/2+1], row padding stripped
    download_rows({RowBlock{fu_, out, (long)3 * g_.nx * g_.ny}}, 2 * g_.nzf, 2 * g_.nzc);
    return;
  }
  if (opt_.mode == 1 && name == "sigma") {  // calcStress with C0 = 0  F:15496-15508: the flux
    if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
    launch_sc_flux(g_, scalar_params(0.0, 1.0), ptrs3(eps_), phase_ptrs(), ptrs3(tau_), stream_);
    download_unpadded(tau_, out, 3, g_.n);
    return;
  }
  if (opt_.mode == 1 && name == "u") {  // potential T = G0 div(C0 : g), alpha = 1  F:15536-15541
    double* const tb = cg_u_active_ ? fu_alt_ : fu_;               // during CG fu_ is the iterate, fu_alt_ is free
    launch_sc_div(g_, ptrs3(eps_), 2 * opt_.mu_0, tb, stream_);    // calcStressConst + divOperatorStaggeredHeat
    const bool timing = timing_;
    timing_ = false;
    fft_g0_chain(tb, 1.0);
    timing_ = timing;
    download_unpadded(tb, out);
    return;
  }
  if (name == "sigma") {  // calcStress with C0 = 0  F:15496-15508
    if (pt_.n < 1) throw std::runtime_error(plan::kNoMaterials);
    stress_to_tau(stress_params(0.0, 0.0, 1.0), eps_);
    check_device_error("sigma");
    download_unpadded(tau_, out, 6, g_.n);
    return;
  }
  if (name == "p") {
    pressure();
    download_unpadded(tau_, out);
    return;
  }
  if (name == "u" && opt_.mode == 2) {
    // velocity  F:15528-15535: calcStressDiff, div, G0(1/(4 mu0), inf, alpha = 1/(2 mu0)): c10 = c20 = -alpha/mu = -2
    viscosity_force("u");
    const double a = 1 / (2 * opt_.mu_0), mu_g = 1 / (4 * opt_.mu_0);
    const double c12[2] = {-a / mu_g, -a / mu_g};
    const bool timing = timing_;
    timing_ = false;
    fft_g0_chain(fu_, a, c12);
    timing_ = timing;
    download_unpadded(fu_, out, 3, g_.n);
    return;
  }
  if (name == "u") {  // u = G0 div (C0 : eps), alpha = 1  F:15509-15521
    double* const ub = cg_u_active_ ? fu_alt_ : fu_;
    launch_stress_const(g_, opt_.mu_0, opt_.lambda_0, ptrs6(eps_), ptrs6(tau_), stream_);
    launch_div(g_, ptrs6(tau_), ptrs3(ub), kNoXHalo, stream_);
    fft_->forward(ub, 3, g_.n, 1 / (double)nglobal_);
    const double alpha = 1.0;
    const double c10 = -alpha / (opt_.mu_0);
    const double c20 = -alpha / (opt_.mu_0 * (1 + opt_.mu_0 / (opt_.lambda_0 + opt_.mu_0)));
    G0Tables tb;
    for (int a = 0; a < 3; ++a) {
      tb.kpm[a] = g0_kpm_[a];
      tb.kp[a] = g0_kp_[a];
    }
    launch_g0(g_, ptrs3(ub), tb, c10, c20, G0Layout{0, 0, 0}, stream_);
    fft_->inverse(ub, 3, g_.n);
    download_unpadded(ub, out, 3, g_.n);
    return;
  }
  const int nc = field_components(name);
  if (nc == 0) throw std::runtime_error("Unknown field '" + name + "'");
  std::vector<RowBlock> blocks;
  for (int c = 0; c < nc; ++c) {
    double* d = device_component(name, c);
    if (!d) throw std::runtime_error("field '" + name + "' is not available");
    blocks.push_back(RowBlock{d, out + (long)c * g_.nxyz, (long)g_.nx * g_.ny});
  }
  download_rows(blocks, g_.nz, g_.nzp);
}

void Solver::set_field(const std::string& name, const double* in) {
  FG_HIP_CHECK(hipSetDevice(device_));
  if (opt_.mode == 1) throw std::runtime_error("fields cannot be set in heat / porous mode");
  ensure_eps();
  u_valid_ = false;
  su_valid_ = false;   // slab driver: the strain field is the state again
  if (name == "f_hat") {
    upload_rows({RowBlock{fu_, const_cast<double*>(in), (long)3 * g_.nx * g_.ny}}, 2 * g_.nzf, 2 * g_.nzc);
    return;
  }
  if (name == "normals") {
    set_normals(in);
    return;
  }
  const int nc = field_components(name);
  if (nc == 0 || name == "sigma" || name == "sumsq" || name == "p") throw std::runtime_error("field '" + name + "' cannot be set");
  std::vector<RowBlock> blocks;
  for (int c = 0; c < nc; ++c) {
    double* d = device_component(name, c);
    if (!d) throw std::runtime_error("field '" + name + "' is not available");
    blocks.push_back(RowBlock{d, const_cast<double*>(in) + (long)c * g_.nxyz, (long)g_.nx * g_.ny});
  }
  upload_rows(blocks, g_.nz, g_.nzp);
}

}  // namespace fg
