// Configuration -> sweep: which combinations of mode, mixing rule, Green operator, method, phase laws and A/B switches the
// solver refuses (plan_error: every message once, in the order the entry points raise them) and which kernel each pass of an
// accepted one launches (plan_sweeps).  Host only, no HIP: Solver::plan_input fills a PlanInput, the launch sites switch on the
// plan.  tests/emulate/emu_sweep_plan.cpp walks both functions against tests/golden/sweep_plans.txt.gz, the decisions as they
// stood before this header existed (profiles/README.md says how the table was recorded).
#pragma once

namespace fg {
namespace plan {

// where the question is asked: Solver::iterate, Solver::run_one_step, one strain-state pass (basic_scheme), calc_ref_material,
// the slab driver (SlabGroup::check_members and the members' fast path)
enum class Entry { Iterate, Run, Pass, RefMaterial, Slab };

struct PlanInput {
  // SolverOptions
  int mode = 0;             // 0 elasticity, 1 heat / porous, 2 viscosity
  int mixing = 0;           // 0 voigt, 1 laminate, 2 reuss
  int gamma_scheme = 0;     // 0 staggered, 1 collocated, 2 full_staggered, 3 willot
  int method = 0;           // 0 basic, 1 cg, 2 polarization
  int error_estimator = 0;  // 0 epsilon, 1 residual, 2 sigma, 3 energy, 4 none
  int u_loop = 2;
  bool u_tile = true, fuse_stress_div = true, cg_fused = true, phi_sweep = true, aniso_tile = true, aniso_sc_tile = true,
       reuss_sweep = true;
  bool bc_relaxed = false;  // bc_relax != 1
  // phase table
  int n_phases = 2;
  bool general_phase = false, aniso_phase = false;
  bool reuss_invertible = true;   // 2 mu > 0 and 2 mu + 3 lambda > 0 (scalar modes: mu > 0) in every phase
  // geometry
  bool tiled = false;          // u_tile_supported(grid)
  bool complementary = false;  // two phases with phi_0 == 1 - phi_1 bit for bit; asked only where reads_complement says so
  bool normals = false;
  // solver
  bool slab = false;        // a slab layout or more than one rank
  bool multi_rank = false;  // more than one rank
  bool slab_ys = false;     // the slab has the y-slab transform
  bool mixed_bc = false;
  bool bc_identity = true;  // bc_projector = identity (Q = 0)
  // call
  Entry entry = Entry::Iterate;
  bool in_run = false;      // inside a run (Slab: under the run driver of method basic)
};

// ------------------------------------------------------------------------------------------------ the refusals, each once
constexpr const char* kNoMaterials = "No materials specified";
constexpr const char* kLaminateNormals = "laminate mixing needs interface normals";
constexpr const char* kPassSlab = "basic_scheme: slab solvers run under the slab driver (fg_slab.hip)";
constexpr const char* kCgSlab = "slab-decomposed solvers run method=cg under the slab driver (fg_slab.hip)";
constexpr const char* kViscScheme = "viscosity mode supports gamma_scheme staggered, full_staggered and willot only";
constexpr const char* kViscMixing = "viscosity mode supports Voigt and Reuss mixing only";
constexpr const char* kViscRelax = "viscosity mode supports bc_relax = 1 only";
constexpr const char* kHeatSlab = "heat / porous mode is not available on slab-decomposed solvers";
constexpr const char* kHeatMixing = "heat / porous mode supports Voigt and Reuss mixing only";
constexpr const char* kHeatRelax = "heat / porous mode does not support bc_relax != 1";
constexpr const char* kHeatMixedBc = "heat / porous mode: mixed boundary conditions run with method=basic (fg_run_load_case) only";
constexpr const char* kHeatEstimator = "heat / porous mode supports the error estimators epsilon and residual";
constexpr const char* kEstimatorMethod = "Selected error estimator is not compatible with the selected solution method";
constexpr const char* kAnisoMode = "aniso (3 x 3 conductivity) phases are available in heat / porous mode only";
constexpr const char* kAnisoSlab = "aniso (3 x 3 conductivity) phases are not available on slab-decomposed solvers";
constexpr const char* kGeneralMode = "general (anisotropic) phases are available in elasticity mode only";
constexpr const char* kGeneralMixing =
    "general (anisotropic) phases support Voigt mixing only (the laminate split is written for isotropic phases)";
constexpr const char* kGeneralDfg = "general (anisotropic) phases are not available with gamma_scheme full_staggered / half_staggered";
constexpr const char* kGeneralSlab = "general (anisotropic) phases are not available on slab-decomposed solvers";
constexpr const char* kReussAniso =
    "mixing_rule reuss is not available with aniso (3 x 3 conductivity) phases (the harmonic mean is written for isotropic phases)";
constexpr const char* kReussDfg =
    "mixing_rule reuss is not available with gamma_scheme full_staggered / half_staggered (the five moduli of the doubly fine "
    "grid are arithmetic means)";
constexpr const char* kReussEnergy =
    "error_estimator energy is not available with mixing_rule reuss (Reuss MaterialLaw energy not implemented)";
constexpr const char* kReussSlab = "mixing_rule reuss is not available on slab-decomposed solvers";
constexpr const char* kReussModuli =
    "mixing_rule reuss needs 2 mu > 0 and 2 mu + 3 lambda > 0 in every phase (the inversion of the phase stiffness fails otherwise)";
constexpr const char* kReussConstant =
    "mixing_rule reuss needs mu > 0 in every phase (the inversion of the phase constant fails otherwise)";
constexpr const char* kWillotHeat =
    "gamma_scheme willot is not available in heat / porous mode (the reference has no such operator)";
constexpr const char* kWillotSlab = "gamma_scheme willot is not available on slab-decomposed solvers";
constexpr const char* kDfgHeat =
    "gamma_scheme full_staggered is not available in heat / porous mode (the reference's 3-component prolongation uses another "
    "grid convention)";
constexpr const char* kDfgMixing =
    "gamma_scheme full_staggered supports Voigt mixing only (the laminate split is not linear in phi and needs normals on the "
    "fine grid)";
constexpr const char* kDfgSlab = "full_staggered is not available on slab-decomposed solvers";
constexpr const char* kPolarSlab = "method polarization is not available on slab-decomposed solvers";
constexpr const char* kPolarMode = "method polarization is available in mode elasticity only (not heat / porous / viscosity)";
constexpr const char* kPolarMixing = "method polarization supports mixing_rule voigt only (not laminate)";
constexpr const char* kPolarDfg = "method polarization is not available with gamma_scheme full_staggered / half_staggered";
constexpr const char* kPolarEstimator =
    "method polarization supports error_estimator epsilon and none only (not sigma / energy / residual: the loop's field is the "
    "polarisation, not the strain)";
constexpr const char* kPolarBc =
    "method polarization supports pure-strain boundary conditions only (bc_projector = identity; the reference switches the "
    "mixed check off)";
constexpr const char* kPolarRelax = "method polarization supports bc_relax = 1 only";
constexpr const char* kSlabScheme = "slab-decomposed solvers run the staggered Green operator";
constexpr const char* kSlabVisc = "viscosity mode supports Voigt mixing and bc_relax = 1 only";
constexpr const char* kSlabHeatFast =
    "heat / porous on slab-decomposed solvers: Voigt mixing, u_loop=2, bc_relax=1 (method=cg: prescribed mean gradients)";

constexpr const char* kMessages[] = {
    kNoMaterials, kLaminateNormals, kPassSlab,    kCgSlab,     kViscScheme,    kViscMixing,  kViscRelax,     kHeatSlab,
    kHeatMixing,  kHeatRelax,       kHeatMixedBc, kHeatEstimator, kEstimatorMethod, kAnisoMode, kAnisoSlab,  kGeneralMode,
    kGeneralMixing, kGeneralDfg,    kGeneralSlab, kReussAniso, kReussDfg,      kReussEnergy, kReussSlab,     kReussModuli,
    kReussConstant, kWillotHeat,    kWillotSlab,  kDfgHeat,    kDfgMixing,     kDfgSlab,     kPolarSlab,     kPolarMode,
    kPolarMixing, kPolarDfg,        kPolarEstimator, kPolarBc, kPolarRelax,    kSlabScheme,  kSlabVisc,      kSlabHeatFast};

constexpr bool dfg(const PlanInput& in) { return in.gamma_scheme == 2; }
constexpr bool willot(const PlanInput& in) { return in.gamma_scheme == 3; }
// mixed boundary conditions in a displacement / potential loop: <tau> of a pass corrects the prescribed mean of the next one
// on the host, which only the run of method basic does
constexpr bool mixed_bc_allowed(const PlanInput& in) {
  return in.entry == Entry::Run ? in.method == 0 : (in.entry == Entry::Slab && in.in_run);
}

// mixing_rule reuss: isotropic phases, staggered / collocated / willot, methods basic and cg, no energy estimator, one GPU
constexpr const char* reuss_refusal(const PlanInput& in) {
  return in.mixing != 2                              ? nullptr
         : in.general_phase                          ? kGeneralMixing
         : in.aniso_phase                            ? kReussAniso
         : dfg(in)                                   ? kReussDfg
         : in.method == 2                            ? kPolarMixing
         : in.error_estimator == 3                   ? kReussEnergy
         : in.slab                                   ? kReussSlab
         : in.reuss_invertible                       ? nullptr
         : in.mode == 0                              ? kReussModuli
                                                     : kReussConstant;
}
constexpr const char* dfg_refusal(const PlanInput& in) {
  return !dfg(in) ? nullptr : in.mode == 1 ? kDfgHeat : in.mixing != 0 ? kDfgMixing : in.slab ? kDfgSlab : nullptr;
}
constexpr const char* willot_refusal(const PlanInput& in) {
  return !willot(in) ? nullptr : in.mode == 1 ? kWillotHeat : in.slab ? kWillotSlab : nullptr;
}
// law "aniso": heat / porous, one GPU.  law "general": elasticity, Voigt mixing, staggered / collocated / willot, one GPU
constexpr const char* law_refusal(const PlanInput& in) {
  if (in.aniso_phase && in.mode != 1) return kAnisoMode;
  if (in.aniso_phase && in.slab) return kAnisoSlab;
  if (!in.general_phase) return nullptr;
  return in.mode != 0 ? kGeneralMode : in.mixing != 0 ? kGeneralMixing : dfg(in) ? kGeneralDfg : in.slab ? kGeneralSlab : nullptr;
}
constexpr const char* polar_refusal(const PlanInput& in) {
  return in.slab                                                 ? kPolarSlab
         : in.mode != 0                                          ? kPolarMode
         : in.mixing != 0                                        ? kPolarMixing
         : dfg(in)                                               ? kPolarDfg
         : (in.error_estimator != 0 && in.error_estimator != 4) ? kPolarEstimator
         : !in.bc_identity                                       ? kPolarBc
         : in.bc_relaxed                                         ? kPolarRelax
                                                                 : nullptr;
}
// the scalar modes only have the potential loop
constexpr const char* scalar_loop_refusal(const PlanInput& in) {
  return in.multi_rank                               ? kHeatSlab
         : in.mixing == 1                            ? kHeatMixing
         : in.bc_relaxed                             ? kHeatRelax
         : (in.mixed_bc && !mixed_bc_allowed(in))    ? kHeatMixedBc
                                                     : nullptr;
}

constexpr const char* slab_law_refusal(const PlanInput& in) { return in.general_phase ? kGeneralSlab : in.aniso_phase ? kAnisoSlab : nullptr; }

// The first refusal of the entry point, or nullptr.
inline const char* plan_error(const PlanInput& in) {
  const char* e = nullptr;
  if (in.entry == Entry::Slab) {   // (a group: SlabGroup::check_members asks the parts per member, with transport and sameness)
    if ((e = reuss_refusal(in))) return e;
    if (in.gamma_scheme != 0) return kSlabScheme;
    if (in.mode == 2 && (in.mixing != 0 || in.bc_relaxed)) return kSlabVisc;
    if (in.n_phases < 1) return kNoMaterials;
    return slab_law_refusal(in);
  }
  if (in.entry == Entry::RefMaterial) {
    if (in.n_phases < 1) return kNoMaterials;
    if ((e = reuss_refusal(in))) return e;
    return law_refusal(in);
  }
  if (in.entry == Entry::Pass) {
    if (in.multi_rank) return kPassSlab;
    if (in.n_phases < 1) return kNoMaterials;
    if (in.mixing == 1 && !in.normals) return kLaminateNormals;
  }
  if ((e = reuss_refusal(in)) || (e = dfg_refusal(in)) || (e = willot_refusal(in)) || (e = law_refusal(in))) return e;
  if (in.entry == Entry::Pass) {
    if (in.mode != 2) return nullptr;
    return in.gamma_scheme == 1 ? kViscScheme : in.mixing == 1 ? kViscMixing : in.bc_relaxed ? kViscRelax : nullptr;
  }
  if (in.method == 2 && (e = polar_refusal(in))) return e;
  if (in.entry == Entry::Run) {
    if (in.error_estimator >= 2 && in.mode == 1) return kHeatEstimator;
    if (in.method == 1 && in.mode != 1) return in.multi_rank ? kCgSlab : nullptr;
    if (in.method == 0 && in.error_estimator == 1) return kEstimatorMethod;
  }
  return in.method != 2 && in.mode == 1 ? scalar_loop_refusal(in) : nullptr;
}

// ------------------------------------------------------------------------------------------------ the sweeps
// one value per launch of Solver::u_pass_front (and of the direction sweep of the fused CG forms)
enum class Front {
  None = -1,
  ScFast,           // potential sweep on the precomputed conductivity (tiled where the grid fits)
  ScTileAniso,      // k_sc_tile_aniso: two complementary phases, either of them aniso
  ScExact,          // potential sweep in the exact order, per phase
  UStressThenDiv,   // laminate / Reuss, exact order: strain + polarisation stored, then its divergence
  UTileDfg,         // tiled sweep on the five moduli of full_staggered
  UTileAniso,       // tiled sweep, two complementary phases with a general one
  UTilePhi,         // tiled sweep reading phi_1 of two complementary phases
  UTilePhiReuss,    // ... forming the harmonic means
  UTileModuli,      // tiled sweep on the two moduli arrays
  UFastModuli,      // untiled sweep on the two moduli arrays
  UStressDivVoigt   // exact order, per phase
};
enum class Staggered { Tile, FusedVoigt, Stored };
enum class Viscosity { TileDfg, Tile, FusedVoigt, Stored };
enum class Cg { DisplacementSpace, Scalar, StrainSpace };

struct SweepPlan {
  bool u_loop = false;              // the displacement / potential loop carries the iteration
  Front front = Front::None;        // its sweep
  bool laminate_correction = false; // ... followed by the divergence of (tau_laminate - tau_voigt) on the interface voxels
  bool sum_tau = false;             // ... delivering the sums of tau (mixed boundary conditions)
  Staggered staggered = Staggered::Stored;   // polarisation + divergence of pass_staggered
  bool staggered_dfg = false;                //   on the five moduli
  Viscosity viscosity = Viscosity::Stored;   // ... of pass_viscosity
  Cg cg = Cg::StrainSpace;          // where method cg iterates (prescribed stresses send it to strain space at the call)
  bool cg_fused_wanted = false;     // the fused vector sweeps, before what only the call knows (memory, callback)
  bool cg_fused_dir = false;        // the direction update inside the operator's sweep
  Front cg_dir = Front::None;       // that sweep
  bool slab_fast = false;           // slab driver: the displacement / potential fast path
};

constexpr bool tile_sweeps(const PlanInput& in) { return in.u_loop >= 2 && in.u_tile && in.tiled; }
// general phases: the displacement loop exists as the tiled sweep's anisotropic form only
constexpr bool aniso_tile(const PlanInput& in) {
  return in.aniso_tile && in.mode == 0 && in.gamma_scheme == 0 && in.mixing == 0 && tile_sweeps(in) && !in.slab && in.complementary;
}
// aniso phases of the scalar modes: k_sc_tile_aniso has no sums of tau
constexpr bool sc_tile_aniso(const PlanInput& in, bool mixed) {
  return in.aniso_sc_tile && in.mode == 1 && in.aniso_phase && tile_sweeps(in) && !mixed && !in.slab && in.complementary;
}
// Reuss mixing: the tiled sweep of two complementary phases forms the harmonic means itself
constexpr bool reuss_sweep(const PlanInput& in) { return in.reuss_sweep && in.mixing == 2 && in.mode == 0 && in.complementary; }

constexpr bool u_loop(const PlanInput& in, bool allow_mixed_bc) {
  if (in.mode == 1) return in.n_phases >= 1;
  if (in.general_phase && !aniso_tile(in)) return false;
  // full_staggered: the displacement loop runs the tiled Voigt sweep only (the untiled sweep has no five-moduli form)
  const bool scheme_ok = in.gamma_scheme == 0 || (dfg(in) && in.mixing == 0 && tile_sweeps(in));
  if (!(in.u_loop && in.mode == 0 && scheme_ok && !in.multi_rank && in.n_phases >= 1 && (in.mixing != 1 || in.normals) && !in.bc_relaxed))
    return false;
  // mixed boundary conditions: the tiled sweep delivers <tau> with the norms
  return !in.mixed_bc || (allow_mixed_bc && tile_sweeps(in));
}

constexpr Front front_sweep(const PlanInput& in) {
  if (in.mode == 1) {
    if (in.u_loop >= 2 && !in.aniso_phase) return Front::ScFast;
    return sc_tile_aniso(in, in.mixed_bc && in.in_run) ? Front::ScTileAniso : Front::ScExact;
  }
  if (in.u_loop < 2) return in.mixing != 0 ? Front::UStressThenDiv : Front::UStressDivVoigt;
  if (!(in.u_tile && in.tiled)) return Front::UFastModuli;   // (never full_staggered: u_loop admits it on tiled grids only)
  if (dfg(in)) return Front::UTileDfg;
  if (in.general_phase) return Front::UTileAniso;
  if (in.mixing == 2) return reuss_sweep(in) ? Front::UTilePhiReuss : Front::UTileModuli;
  return in.complementary ? Front::UTilePhi : Front::UTileModuli;
}

// Whether the decisions read PlanInput::complementary (the caller then runs the device check, once per geometry).  The loop
// decision reads it for a general phase only; the sweeps (sweep = true) wherever a two-phase form is at stake.
constexpr bool reads_complement(const PlanInput& in, bool sweep) {
  if (in.n_phases != 2 || !in.phi_sweep || !tile_sweeps(in)) return false;
  if (in.mode == 1) return sweep && in.aniso_sc_tile && in.aniso_phase && !in.slab && !(in.mixed_bc && in.in_run);
  if (in.mode != 0) return false;
  if (in.general_phase) return in.aniso_tile && in.gamma_scheme == 0 && in.mixing == 0 && !in.slab;
  return sweep && !dfg(in) && (in.mixing != 2 || in.reuss_sweep);
}

constexpr SweepPlan plan_sweeps(const PlanInput& in) {
  SweepPlan p;
  p.u_loop = u_loop(in, mixed_bc_allowed(in));
  if (p.u_loop) {
    p.front = front_sweep(in);
    const bool tile = p.front >= Front::UTileDfg && p.front <= Front::UTileModuli;
    p.laminate_correction = in.mixing == 1 && (tile || p.front == Front::UFastModuli);
    p.sum_tau = tile ? in.mixed_bc : (p.front == Front::ScFast && in.mixed_bc && in.in_run);
  }
  const bool fast_tiled = in.u_loop >= 2 && in.tiled;   // (the strain-state passes do not ask for u_tile)
  // Voigt / Reuss: the tiled form on the moduli arrays; Voigt without mixed boundary conditions: polarisation and divergence in
  // one sweep; laminate (a Newton solve per voxel) and general phases: the stored polarisation
  p.staggered_dfg = dfg(in);
  p.staggered = in.fuse_stress_div && in.mixing != 1 && fast_tiled && !in.general_phase ? Staggered::Tile
                : in.fuse_stress_div && in.mixing == 0 && !in.mixed_bc && !dfg(in) && !in.general_phase ? Staggered::FusedVoigt
                                                                                                        : Staggered::Stored;
  // viscosity: the fused forms evaluate the Voigt rule; full_staggered has the tiled one only
  p.viscosity = !(in.fuse_stress_div && in.mixing != 2 && (!dfg(in) || fast_tiled)) ? Viscosity::Stored
                : dfg(in)                                                           ? Viscosity::TileDfg
                : fast_tiled                                                        ? Viscosity::Tile
                                                                                    : Viscosity::FusedVoigt;
  // (the estimators that measure a mean of the strain field run in strain space, where the iterate is a stored field)
  if (in.method == 1)
    p.cg = in.mode == 1 ? Cg::Scalar : in.u_loop >= 2 && u_loop(in, false) && in.error_estimator < 2 ? Cg::DisplacementSpace : Cg::StrainSpace;
  if (in.method != 1) {
  } else if (p.cg == Cg::DisplacementSpace) {
    p.cg_fused_wanted = in.cg_fused && in.u_tile && in.tiled && !in.slab;
    p.cg_fused_dir = p.cg_fused_wanted && in.mixing != 1;   // laminate mixing: the interface kernels read u_p as a stored field
    if (p.cg_fused_dir)   // (Reuss mixing: the CG sweep reads the moduli arrays)
      p.cg_dir = dfg(in) ? Front::UTileDfg : in.general_phase ? Front::UTileAniso : in.mixing != 2 && in.complementary ? Front::UTilePhi : Front::UTileModuli;
  } else if (p.cg == Cg::Scalar) {
    p.cg_fused_wanted = p.cg_fused_dir = in.cg_fused && fast_tiled && !in.slab && (!in.aniso_phase || sc_tile_aniso(in, false));
    if (p.cg_fused_dir) p.cg_dir = in.aniso_phase ? Front::ScTileAniso : Front::ScFast;
  } else {
    p.cg_fused_wanted = in.cg_fused;
  }
  const bool slab_common = in.u_loop >= 2 && in.gamma_scheme == 0 && in.n_phases >= 1 && !in.bc_relaxed && (!in.mixed_bc || mixed_bc_allowed(in));
  p.slab_fast = in.mode == 1   ? slab_common && in.mixing == 0 && in.slab_ys
                : in.mode == 0 ? slab_common && in.u_tile && in.tiled && (in.mixing == 0 || (in.mixing == 1 && in.normals))
                               : false;
  return p;
}

// full_staggered never reaches the untiled displacement sweep
constexpr PlanInput dfg_untiled() {
  PlanInput in;
  in.gamma_scheme = 2;
  return in;
}
static_assert(!plan_sweeps(dfg_untiled()).u_loop && plan_sweeps(dfg_untiled()).front == Front::None, "full_staggered, untiled grid");

}  // namespace plan
}  // namespace fg
