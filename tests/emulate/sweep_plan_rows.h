// The configurations of tests/golden/sweep_plans.txt.gz, in the table's order: for_each_row(f) calls f(key, input) per line;
// f returns whether it refused the row (the row set follows the answers of whoever walks it, not this header's).
// Primary cross: mode x mixing x gamma_scheme x method x u_loop x phase class; per primary row the full cross of
// {u_tile, tiled grid, mixed bc, entry iterate / run}, then every remaining factor changed singly from its default on both
// entries (estimators, bc_relax, normals, slab, the A/B switches, Reuss moduli, the projector) and the other entry points.
#pragma once
#include <cstdio>
#include <string>

#include "../../fibergen_amd/csrc/fg_sweep_plan.h"

namespace sweep_rows {
using fg::plan::Entry;
using fg::plan::PlanInput;

// phase classes: 1 iso; 2 iso complementary / not; 3 iso; 2 with a general phase, complementary / not; 2 with an aniso phase
struct PhaseClass {
  const char* name;
  int n;
  bool general, aniso, complementary;
};
static const PhaseClass kClasses[8] = {{"iso1", 1, false, false, false},    {"iso2c", 2, false, false, true},
                                       {"iso2", 2, false, false, false},    {"iso3", 3, false, false, false},
                                       {"general2c", 2, true, false, true}, {"general2", 2, true, false, false},
                                       {"aniso2c", 2, false, true, true},   {"aniso2", 2, false, true, false}};
static const char* kEntryName[] = {"iterate", "run", "pass", "ref", "slab"};

template <class F>
void for_each_row(F f) {
  char key[160];
  for (int mode = 0; mode < 3; ++mode)
    for (int mixing = 0; mixing < 3; ++mixing)
      for (int gs = 0; gs < 4; ++gs)
        for (int method = 0; method < 3; ++method)
          for (int ul = 0; ul < 3; ++ul)
            for (const PhaseClass& pc : kClasses) {
              PlanInput base;
              base.mode = mode, base.mixing = mixing, base.gamma_scheme = gs, base.method = method, base.u_loop = ul;
              base.n_phases = pc.n, base.general_phase = pc.general, base.aniso_phase = pc.aniso, base.complementary = pc.complementary;
              base.tiled = true, base.normals = true, base.slab_ys = true;
              auto row = [&](PlanInput in, const char* factor) {
                in.in_run = in.entry == Entry::Run || (in.entry == Entry::Slab && in.in_run);
                // the device check answers false wherever its preconditions fail (Solver::two_phase_complementary)
                in.complementary = in.complementary && in.phi_sweep && in.n_phases == 2 && in.mode != 2;
                snprintf(key, sizeof key, "%d %d %d %d %d %s %d %d %d %s %s:", mode, mixing, gs,
                         method, ul, pc.name, in.u_tile, in.tiled, in.mixed_bc, kEntryName[(int)in.entry], factor);
                return f(key, in);
              };
              bool refused[2] = {false, false};   // the primary row at the defaults of the cross, per entry
              for (int ut = 0; ut < 2; ++ut)
                for (int tiled = 0; tiled < 2; ++tiled)
                  for (int mixed = 0; mixed < 2; ++mixed)
                    for (Entry e : {Entry::Iterate, Entry::Run}) {
                      PlanInput in = base;
                      in.u_tile = ut, in.tiled = tiled, in.mixed_bc = mixed, in.bc_identity = !mixed, in.entry = e;
                      const bool r = row(in, "-");
                      if (ut && tiled && !mixed) refused[e == Entry::Run] = r;
                    }
              for (Entry e : {Entry::Iterate, Entry::Run}) {
                if (refused[e == Entry::Run]) continue;   // a primary row that is refused on this entry already: no single-factor rows
                auto single = [&](const char* factor, auto set) {
                  PlanInput in = base;
                  in.entry = e;
                  set(in);
                  row(in, factor);
                };
                single("estimator=residual", [](PlanInput& in) { in.error_estimator = 1; });
                single("estimator=sigma", [](PlanInput& in) { in.error_estimator = 2; });
                single("estimator=energy", [](PlanInput& in) { in.error_estimator = 3; });
                single("estimator=none", [](PlanInput& in) { in.error_estimator = 4; });
                single("bc_relax", [](PlanInput& in) { in.bc_relaxed = true; });
                single("no_normals", [](PlanInput& in) { in.normals = false; });
                single("slab_layout", [](PlanInput& in) { in.slab = true; });
                single("slab_ranks", [](PlanInput& in) { in.slab = in.multi_rank = true; });
                single("fuse_stress_div=0", [](PlanInput& in) { in.fuse_stress_div = false; });
                single("cg_fused=0", [](PlanInput& in) { in.cg_fused = false; });
                single("phi_sweep=0", [](PlanInput& in) { in.phi_sweep = false; });
                single("aniso_tile=0", [](PlanInput& in) { in.aniso_tile = false; });
                single("aniso_sc_tile=0", [](PlanInput& in) { in.aniso_sc_tile = false; });
                single("reuss_sweep=0", [](PlanInput& in) { in.reuss_sweep = false; });
                single("reuss_moduli", [](PlanInput& in) { in.reuss_invertible = false; });
                single("projector", [](PlanInput& in) { in.bc_identity = false; });
              }
              // the other entry points: a strain-state pass (with and without normals), calc_ref_material, the slab driver
              for (int k = 0; k < 8; ++k) {
                PlanInput in = base;
                in.entry = k < 2 ? Entry::Pass : k == 2 ? Entry::RefMaterial : Entry::Slab;
                if (k == 1) in.normals = false;
                if (k >= 3) in.slab = in.multi_rank = true, in.in_run = (k & 1) == 0;
                if (k >= 5) in.mixed_bc = true, in.bc_identity = false;
                if (k == 7) in.slab_ys = false, in.mixed_bc = false, in.bc_identity = true;
                row(in, k == 1 ? "no_normals" : k == 7 ? "no_ys" : in.in_run ? "in_run" : "-");
              }
            }
  // what the cross does not reach: no phases, a strain-state pass with bc_relax != 1 or on a rank of several
  for (int mode = 0; mode < 3; ++mode)
    for (int k = 0; k < 5; ++k) {
      PlanInput in;
      in.mode = mode, in.tiled = in.normals = in.slab_ys = true;
      in.entry = k == 1 ? Entry::RefMaterial : k == 2 ? Entry::Slab : Entry::Pass;
      if (k < 3) in.n_phases = 0;
      if (k == 2 || k == 4) in.slab = in.multi_rank = true;
      in.bc_relaxed = k == 3;
      snprintf(key, sizeof key, "%d 0 0 0 2 %s 1 1 0 %s %s:", mode, k < 3 ? "none" : "iso2", kEntryName[(int)in.entry],
               k == 3 ? "bc_relax" : k == 4 ? "slab_ranks" : "-");
      f(key, in);
    }
}

static const char* kFrontName[] = {"None",     "ScFast",        "ScTileAniso", "ScExact",     "UStressThenDiv", "UTileDfg", "UTileAniso",
                                   "UTilePhi", "UTilePhiReuss", "UTileModuli", "UFastModuli", "UStressDivVoigt"};
static const char* kStaggeredName[] = {"Tile", "FusedVoigt", "Stored"};
static const char* kViscosityName[] = {"TileDfg", "Tile", "FusedVoigt", "Stored"};
static const char* kCgName[] = {"DisplacementSpace", "Scalar", "StrainSpace"};

// the table's first line: the columns of a key and of a plan
static const char* kColumns =
    "# mode mixing gamma_scheme method u_loop phase_class u_tile tiled mixed_bc entry factor: ERR <message> | complement_check u_loop front "
    "laminate_correction sum_tau staggered staggered_dfg viscosity cg cg_fused_wanted cg_fused_dir cg_dir slab_fast";
// one line of the table for an accepted configuration (front, dir: Front values + 1, so that None = 0)
inline void print_plan(const char* key, int complement_check, bool u_loop, int front, bool lam, bool sum_tau, int stag, bool stag_dfg, int visc, int cg,
                       bool fused_wanted, bool fused_dir, int dir, bool slab_fast) {
  printf("%s %c %d %s %d %d %s %d %s %s %d %d %s %d\n", key, complement_check < 0 ? '-' : '0' + complement_check,
         u_loop, kFrontName[front], lam, sum_tau, kStaggeredName[stag], stag_dfg, kViscosityName[visc], kCgName[cg], fused_wanted, fused_dir,
         kFrontName[dir], slab_fast);
}

}  // namespace sweep_rows
