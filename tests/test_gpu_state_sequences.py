"""One LIVE solver through sequences of calls and option switches: the host-side state of fg_solver.h (u_valid_, eps_stale_,
E_cur_, pending_back_ / back_ready_, the moduli caches mod_dirty_ / smod_dirty_ / complement_dirty_ / mixed_dirty_, pol_state_,
cg_u_active_, su_valid_) decides which kernel runs on which buffer with which moduli, and a wrong transition does not fault.

Every script is played on the product and on tests/state_model.py (a freshly built oracle of the current configuration started
from the carried strain field -- never a product run) and after EVERY step the strain field is compared; after a whole run
also the iteration count, the residual history and the mean stress.

Bars (the project's, nothing new): a fixed count of passes against a NumPy oracle 1e-11 relative max-norm (test_gpu_parity.py,
test_gpu_bluestein.py), residual histories atol 1e-11 (test_gpu_dfg_state.py), iteration counts equal, product against product on
the same kernels bit for bit.  The runs use loose tolerances (a handful of iterations), so the pass-count bar holds for them.

Grids: (4, 16, 80) tiled sweep, (12, 10, 6) untiled, (16, 8, 64) the smallest grid x_layout accepts."""
import numpy as np
import pytest

import aniso_reference as ar
import general_reference as gr
import state_model as sm
from helpers import make_gpu_solver, rel_err, sphere_normals, sphere_phi, two_phase_setup
from oracle.ls_oracle import voigt_id4
from state_model import C, Step

pytestmark = pytest.mark.gpu

TOL = 1e-11
E1, E2 = sm.E_LOADS
TILED, UNTILED, XLAYOUT = ((4, 16, 80), (1.0, 1.5, 0.8)), ((12, 10, 6), (2.0, 1.0, 0.5)), ((16, 8, 64), (1.0, 1.0, 1.0))
IDS = {TILED: "4x16x80-tiled", UNTILED: "12x10x6-untiled", XLAYOUT: "16x8x64-xlayout"}


def play(s, m, steps, tag):
    """every step on the product and on the model, then the comparison; prints the measured error of every step"""
    worst = 0.0
    for i, st in enumerate(steps):
        got = want = None
        for c in st.calls:
            got, want = sm.call(s, *c), sm.call(m, *c)
        errs = {}
        if isinstance(want, bool):
            assert got is want, (tag, i, st.label)
        elif want is not None:
            assert np.shape(got) == np.shape(want), (tag, i, st.label)
            errs["value"] = rel_err(got, want)
        if st.full_run:
            assert s.iterations == m.iterations, (tag, i, st.label, s.iterations, m.iterations)
            np.testing.assert_allclose(s.residuals, m.residuals, rtol=0, atol=1e-11, err_msg="%s step %d %s" % (tag, i, st.label))
            errs["mean_stress"] = rel_err(s.mean_stress(), m.mean_stress())
        errs["epsilon"] = rel_err(s.get_field("epsilon"), m.get_field("epsilon"))
        print("STATE %s step %2d %-28s %s" % (tag, i, st.label, "  ".join("%s %.2e" % kv for kv in errs.items())))
        for k, v in errs.items():
            assert v <= TOL, (tag, i, st.label, k, v)
        worst = max([worst] + list(errs.values()))
    print("STATE-WORST %s %.2e" % (tag, worst))
    return worst


def pair(grid, dims, **opts):
    mats, phis, normals = two_phase_setup(grid)
    s = make_gpu_solver(grid, dims, **opts)
    m = sm.StateModel(grid, dims, mats=mats, phis=phis, normals=normals, **opts)
    return s, m, mats, phis


def prologue(grid, seed):
    return [Step("set_field", C("set_field", "epsilon", np.random.default_rng(seed).standard_normal((6,) + grid))),
            Step("calc_ref_material", C("calc_ref_material"))]


def options(*seq):
    """one pass after each switch"""
    out = []
    for kw in seq:
        label = ",".join("%s=%s" % kv for kv in kw.items())
        out += [Step(label, C("set_options", **kw)), Step("iterate 1", C("iterate", E2, 1))]
    return out


# ---------------------------------------------------------------------- A: the displacement state
@pytest.mark.parametrize("grid,dims", [TILED, UNTILED, XLAYOUT], ids=[IDS[TILED], IDS[UNTILED], IDS[XLAYOUT]])
def test_sequence_a_displacement_state(grid, dims):
    s, m, mats, phis = pair(grid, dims, u_loop=2)
    phi_b, phi_c = sphere_phi(grid, R=0.35, c=(0.45, 0.55, 0.5)), sphere_phi(grid, R=0.28, c=(0.55, 0.5, 0.45))
    steps = prologue(grid, 11) + [
        Step("A1 iterate 2", C("iterate", E1, 2)),
        Step("A2 get epsilon", C("get_field", "epsilon")),                  # reads must not perturb the state
        Step("A2 mean_stress", C("mean_stress")),
        Step("A2 get sigma", C("get_field", "sigma")),
        Step("A2 iterate 1", C("iterate", E1, 1)),
        Step("A3 iterate E2 2", C("iterate", E2, 2)),                       # E_cur_ handed over
        Step("A4 get u", C("get_field", "u")),                              # u_valid_ dropped: fu_ is overwritten
        Step("A4 iterate 1", C("iterate", E2, 1)),                          # ... so this is a strain-state pass
        # a field set while the displacement is the state: set_field drops u_valid_, the next pass starts from the new field
        Step("A4 set_field", C("set_field", "epsilon", np.random.default_rng(12).standard_normal((6,) + grid))),
        Step("A4 iterate 2", C("iterate", E2, 2)),
        Step("A5 set_phase moduli", C("set_phase", 0, 2.3, 1.1)),           # moduli caches rebuilt, state kept
        Step("A5 calc_ref_material", C("calc_ref_material")),
        Step("A5 iterate 2", C("iterate", E2, 2)),
        # both fractions replaced by fields that are NOT complementary: a stale complementary_ would form phi_0 as 1 - phi_1
        Step("A6 set_phase fractions", C("set_phase", 0, 2.3, 1.1, 0.9 * (1.0 - phi_b)), C("set_phase", 1, *mats[1], phi_b)),
        Step("A6 iterate 2", C("iterate", E2, 2)),
        Step("A6 complementary again", C("set_phase", 0, 2.3, 1.1, 1.0 - phi_c), C("set_phase", 1, *mats[1], phi_c)),
        Step("A6 iterate 1", C("iterate", E2, 1)),
        Step("A7 set_normals", C("set_normals", sphere_normals(grid, c=(0.55, 0.5, 0.45)))),
        Step("A7 laminate", C("set_options", mixing_rule="laminate")),
        Step("A7 iterate 2", C("iterate", E2, 2)),
        Step("A7 voigt", C("set_options", mixing_rule="voigt")),
        Step("A7 iterate 1", C("iterate", E2, 1)),
    ]
    steps += options(dict(gamma_scheme="collocated"), dict(gamma_scheme="staggered"), dict(gamma_scheme="willot"),
                     dict(gamma_scheme="staggered"))                                                         # A8
    steps += options(dict(u_loop=0), dict(u_loop=1), dict(u_loop=2), dict(u_tile=0), dict(u_tile=1))           # A9
    steps += options(dict(fuse_x=0), dict(fuse_x=1), dict(plane_fft=0), dict(plane_fft=1))                     # A10
    if (grid, dims) == XLAYOUT:
        steps += options(dict(x_layout=1), dict(x_layout=0), dict(pair_chunk=4), dict(pair_chunk=0))
    play(s, m, steps, "A-" + IDS[(grid, dims)])
    s.close()


# ---------------------------------------------------------------------- B: runs that stop, then continue
@pytest.mark.parametrize("grid,dims", [TILED, UNTILED], ids=[IDS[TILED], IDS[UNTILED]])
def test_sequence_b_runs_that_stop_then_continue(grid, dims):
    s, m, mats, phis = pair(grid, dims, tol=1e-3)
    tag = "B-" + IDS[(grid, dims)]
    play(s, m, [Step("B1 run", C("run", E1), full_run=True)], tag)            # converges: the enqueued chain is discarded
    first = s.get_field("epsilon"), s.iterations, s.residuals
    play(s, m, [
        Step("B1 iterate 1", C("iterate", E1, 1)),
        Step("B2 run maxiter 3", C("run_maxiter", E1, 3), full_run=True),
        Step("B2 iterate 2", C("iterate", E1, 2)),
        Step("B3 run stopped at 2", C("run_stopped", E1, 2), full_run=True),  # the break in run(): fu_alt_ was written, not adopted
        Step("B3 iterate 1", C("iterate", E1, 1)),
        Step("B4 run_load_steps", C("run_load_steps", E1, params=[0.0, 0.4, 1.0]), full_run=True),
        Step("B4 iterate 1", C("iterate", E1, 1)),
        Step("B4 run", C("run", E1), full_run=True),
    ], tag)
    # ... and that run is a first run (product against product: bit for bit)
    assert np.array_equal(s.get_field("epsilon"), first[0]) and s.iterations == first[1] and s.residuals == first[2]
    play(s, m, [
        Step("B5 cg", C("set_options", method="cg")),
        Step("B5 run cg", C("run", E1), full_run=True),
        Step("B5 basic", C("set_options", method="basic")),
        Step("B5 iterate 1", C("iterate", E1, 1)),
        Step("B5 polarization", C("set_options", method="polarization")),
        Step("B5 iterate 2", C("iterate", E1, 2)),
        Step("B5 basic", C("set_options", method="basic")),
        Step("B5 iterate 1", C("iterate", E1, 1)),
        Step("B5 cg", C("set_options", method="cg")),
        Step("B5 run cg", C("run", E1), full_run=True),
        Step("B6 uniaxial stress", C("set_options", method="basic"), C("set_bc_projector", sm.P_UNIAXIAL)),
        Step("B6 run mixed bc", C("run", sm.E_UNIAXIAL, np.zeros(6)), full_run=True),
        Step("B6 identity", C("set_bc_projector", voigt_id4())),
        Step("B6 iterate 2", C("iterate", E1, 2)),
    ], tag)
    s.close()


# ---------------------------------------------------------------------- C: laws and modes on one solver
def test_sequence_c1_general_law_enters_and_leaves_the_tiled_sweep():
    grid, dims = TILED
    s, m, mats, phis = pair(grid, dims, u_loop=2)
    tag = "C1-" + IDS[TILED]
    play(s, m, prologue(grid, 13) + [Step("C1 iterate 2 iso", C("iterate", E1, 2))], tag)
    assert s.counter("u_tile_aniso") == 0
    play(s, m, [Step("C1 set_phase_stiffness", C("set_phase_stiffness", 1, gr.distinct_stiffness(3.0))),
                Step("C1 iterate 2 general", C("iterate", E1, 2))], tag)
    n = s.counter("u_tile_aniso")
    assert n >= 1                                                           # the anisotropic form of the tiled sweep was entered
    play(s, m, [Step("C1 set_phase iso", C("set_phase", 1, *mats[1])), Step("C1 iterate 2 iso", C("iterate", E1, 2))], tag)
    assert s.counter("u_tile_aniso") == n                                   # ... and left
    s.close()


@pytest.mark.parametrize("grid,dims", [TILED, UNTILED], ids=[IDS[TILED], IDS[UNTILED]])
def test_sequence_c2_modes_on_one_solver(grid, dims):
    """the state across a mode switch is not defined (and set_field is refused in heat mode): every leg is a fresh run()"""
    s, m, mats, phis = pair(grid, dims, tol=1e-3)
    tag = "C2-" + IDS[(grid, dims)]
    K = ar.random_spd3(np.random.default_rng(5), 4.0)

    def phases(a, b):
        return C("set_phase", 0, *a), C("set_phase", 1, *b)

    play(s, m, [Step("C2 elasticity run", C("run", E1), full_run=True)], tag)
    first = s.get_field("epsilon"), s.iterations, s.residuals
    play(s, m, [
        Step("C2 heat run", C("set_options", mode="heat"), *phases((1.0, 0.0), (8.0, 0.0)), C("run", E1[:3]), full_run=True),
        Step("C2 heat aniso", C("set_phase_conductivity", 1, ar.k6(K))),
        Step("C2 heat iterate 2", C("iterate", E1[:3], 2)),
        Step("C2 heat iso again", C("set_phase", 1, 8.0, 0.0)),
        Step("C2 heat iterate 2", C("iterate", E1[:3], 2)),
        Step("C2 porous run", C("set_options", mode="porous"), C("run", E2[:3]), full_run=True),
        Step("C2 viscosity run", C("set_options", mode="viscosity"), *phases((1.0, 0.0), (0.05, 0.0)), C("run", E2), full_run=True),
        Step("C2 elasticity run", C("set_options", mode="elasticity"), *phases(*mats), C("run", E1), full_run=True),
    ], tag)
    assert np.array_equal(s.get_field("epsilon"), first[0]) and s.iterations == first[1] and s.residuals == first[2]
    s.close()


# ---------------------------------------------------------------------- D: slab group on one GPU
def test_sequence_d_slab_group():
    from fibergen_amd.distributed import SlabGroup
    grid, dims = (8, 16, 124), (1.0, 2.0, 1.5)
    mats, phis, normals = two_phase_setup(grid)
    g = SlabGroup(*grid, *dims, nranks=2)
    g.set_num_phases(2)
    for p in range(2):
        g.set_phase(p, mats[p][0], mats[p][1], phis[p])
    g.set_normals(normals)
    g.set_options(mixing_rule="voigt", tol=1e-3)
    m = sm.StateModel(grid, dims, mats=mats, phis=phis, normals=normals, tol=1e-3)
    phi_b, phi_c = sphere_phi(grid, R=0.35, c=(0.45, 0.55, 0.5)), sphere_phi(grid, R=0.28, c=(0.55, 0.5, 0.45))
    play(g, m, prologue(grid, 17) + [
        Step("D iterate 2", C("iterate", E1, 2)),                           # su_valid_
        Step("D get epsilon", C("get_field", "epsilon")),
        Step("D get sigma", C("get_field", "sigma")),
        Step("D iterate E2 1", C("iterate", E2, 1)),
        Step("D set_phase moduli", C("set_phase", 0, 2.3, 1.1)),            # complementary phases: the sweep reads phi_1 + the table
        Step("D iterate 1", C("iterate", E2, 1)),
        # fractions that are not complementary: the slabs' moduli buffer (smod_dirty_) now holds the effective moduli ...
        Step("D set_phase fractions", C("set_phase", 0, 2.3, 1.1, 0.9 * (1.0 - phi_b)), C("set_phase", 1, *mats[1], phi_b)),
        Step("D iterate 1", C("iterate", E2, 1)),
        Step("D set_phase moduli", C("set_phase", 1, 4.0, 2.0)),            # ... which new moduli alone have to rebuild
        Step("D iterate 1", C("iterate", E2, 1)),
        Step("D complementary again", C("set_phase", 0, 2.3, 1.1, 1.0 - phi_c), C("set_phase", 1, 4.0, 2.0, phi_c)),
        Step("D iterate 1", C("iterate", E2, 1)),
        Step("D set_normals", C("set_normals", sphere_normals(grid, c=(0.55, 0.5, 0.45)))),
        Step("D laminate", C("set_options", mixing_rule="laminate")),
        Step("D iterate 1", C("iterate", E2, 1)),
        Step("D cg", C("set_options", method="cg")),
        Step("D run cg", C("run", E1), full_run=True),                      # slab_reset_state
    ], "D-8x16x124-slab2")
    g.close()


# ---------------------------------------------------------------------- the seeded walk
@pytest.mark.parametrize("seed", list(sm.SEEDS))
def test_random_walks(seed):
    grid, dims, steps = sm.walk(seed)
    s, m, mats, phis = pair(grid, dims, tol=1e-3)
    play(s, m, prologue(grid, 100 + seed) + steps, "W-seed%d" % seed)
    s.close()
