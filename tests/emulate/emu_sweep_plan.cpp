// Stand-alone driver of fibergen_amd/csrc/fg_sweep_plan.h (tests/test_sweep_plan.py): prints plan_error / plan_sweeps for every
// configuration of sweep_plan_rows.h in the format of tests/golden/sweep_plans.txt.gz, then the header's message constants
// (MSG lines), and checks the plans' invariants.  A FAIL line per broken property, OK as the last line.
#include <cstring>

#include "sweep_plan_rows.h"

using namespace fg::plan;

static bool same(const SweepPlan& a, const SweepPlan& b) {
  return a.u_loop == b.u_loop && a.front == b.front && a.laminate_correction == b.laminate_correction && a.sum_tau == b.sum_tau &&
         a.staggered == b.staggered && a.staggered_dfg == b.staggered_dfg && a.viscosity == b.viscosity && a.cg == b.cg &&
         a.cg_fused_wanted == b.cg_fused_wanted && a.cg_fused_dir == b.cg_fused_dir && a.cg_dir == b.cg_dir && a.slab_fast == b.slab_fast;
}

int main() {
  int fails = 0;
  printf("%s\n", sweep_rows::kColumns);
  sweep_rows::for_each_row([&](const char* key, const PlanInput& in) {
    auto check = [&](bool ok, const char* what) {
      if (!ok) printf("FAIL %s: %s\n", what, key), ++fails;
    };
    if (const char* e = plan_error(in)) {
      printf("%s ERR %s\n", key, e);
      return true;
    }
    const SweepPlan p = plan_sweeps(in);
    // where Solver asks plan_input for the complement check: the loop decision of iterate / run_one_step / run_cg (ask 1), the sweeps
    // (ask 2) of u_pass_front -- reached from iterate, the loop of method basic and the CG loops in displacement / potential space
    const bool walked = in.entry == Entry::Iterate || in.entry == Entry::Run;
    const bool loop_asked = in.method != 2 && !(in.entry == Entry::Run && in.method == 1 && in.mode == 1);
    const bool sweeps_reached = p.u_loop && in.method != 2 && (in.entry == Entry::Iterate || in.method == 0 || p.cg != Cg::StrainSpace);
    const int asked = !walked ? -1 : (loop_asked && reads_complement(in, false)) || (sweeps_reached && reads_complement(in, true));
    sweep_rows::print_plan(key, asked, p.u_loop, (int)p.front + 1, p.laminate_correction, p.sum_tau, (int)p.staggered, p.staggered_dfg, (int)p.viscosity,
                           (int)p.cg, p.cg_fused_wanted, p.cg_fused_dir, (int)p.cg_dir + 1, p.slab_fast);
    for (Front f : {p.front, p.cg_dir}) {
      const bool utile = f >= Front::UTileDfg && f <= Front::UTileModuli;
      check(!utile || (in.tiled && in.u_tile && in.u_loop >= 2), "a tiled sweep outside the tiled grids / u_tile / u_loop >= 2");
      check(!(f == Front::UTileAniso || f == Front::ScTileAniso || f == Front::UTilePhi || f == Front::UTilePhiReuss) || in.complementary,
            "a two-phase form without complementary phases");
      check(f != Front::UTileDfg || in.tiled, "full_staggered on the untiled displacement sweep");
    }
    check(p.u_loop || p.front == Front::None, "a front sweep without the loop");
    check(!dfg(in) || in.mode != 0 || p.front == Front::None || p.front == Front::UTileDfg, "full_staggered on a sweep without the five moduli");
    check(p.cg != Cg::DisplacementSpace || p.u_loop, "CG in displacement space without the loop");
    check(p.cg_fused_dir == (p.cg_dir != Front::None) && (!p.cg_fused_dir || p.cg_fused_wanted), "direction sweep and its switch disagree");
    check(!in.slab || !(in.general_phase || in.aniso_phase || in.mixing == 2 || willot(in) || dfg(in) ||
                        (in.method == 2 && in.entry != Entry::Slab)),
          "a slab solver accepted with a feature the slab driver lacks");
    // the plan reads the complement flag only where reads_complement says so
    PlanInput off = in;
    off.complementary = false;
    check(reads_complement(in, true) || same(p, plan_sweeps(off)), "the plan reads the complement check where it is not asked for");
    check(reads_complement(in, false) || p.u_loop == plan_sweeps(off).u_loop, "the loop decision reads the complement check where it is not asked for");
    return false;
  });
  for (const char* m : kMessages) {
    printf("MSG %s\n", m);
    int n = 0;
    for (const char* o : kMessages) n += strcmp(m, o) == 0;
    if (n != 1) printf("FAIL message listed %d times: %s\n", n, m), ++fails;
  }
  printf(fails ? "FAILED\n" : "OK\n");
  return fails ? 1 : 0;
}
