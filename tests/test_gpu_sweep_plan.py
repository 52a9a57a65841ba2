"""Live solvers against tests/golden/sweep_plans.txt.gz: per value of plan::Front (fibergen_amd/csrc/fg_sweep_plan.h) one
configuration whose counter("front_sweep") / counter("cg_dir_sweep") -- set at the launch site -- must be the sweep the golden row
of that configuration names (looked up in the table, not computed), the three older counters, one refusal per message family
with its exact words, and one solver taken across a switch.  8 x 8 x 8: the untiled paths; 4 x 14 x 80: the smallest tiled grid."""
import numpy as np
import pytest

from test_sweep_plan import FRONT, golden_plan

pytestmark = pytest.mark.gpu

SMALL, TILED = (8, 8, 8), (4, 14, 80)
E6 = np.array([0.5, -0.2, 0.1, 0.05, -0.1, 0.3])
E3 = np.array([1.0, -0.5, 0.25])
MODE = {"elasticity": 0, "heat": 1, "viscosity": 2}
MIXING = {"voigt": 0, "laminate": 1, "reuss": 2}
SCHEME = {"staggered": 0, "collocated": 1, "full_staggered": 2, "willot": 3}
METHOD = {"basic": 0, "cg": 1, "polarization": 2}


def fields(grid, complementary=True):
    ax = [(np.arange(n) + 0.5) / n - 0.5 for n in grid]
    v = np.stack(np.broadcast_arrays(ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :])).astype(np.float64)
    r = np.sqrt((v * v).sum(axis=0))
    phi = np.clip(0.5 + (0.3 - r) * 6.0, 0.0, 1.0)
    other = 1.0 - phi if complementary else (1.0 - phi) * (1.0 - 2.0 ** -20)   # not 1 - phi bit for bit
    return other, phi, v / np.where(r == 0, 1.0, r)


def solver(grid, mode="elasticity", law="iso", complementary=True, **opts):
    from fibergen_amd import LSSolver
    f0, f1, nrm = fields(grid, complementary)
    s = LSSolver(*grid)
    s.set_options(mode=mode)
    if "gamma_scheme" in opts:
        s.set_options(gamma_scheme=opts.pop("gamma_scheme"))
    s.set_num_phases(2)
    mats = ((1.0, 0.0), (7.0, 0.0)) if mode == "heat" else ((0.4, 0.6), (4.0, 2.5))
    for p, f in enumerate((f0, f1)):
        s.set_phase(p, mats[p][0], mats[p][1], f)
    if law == "general":
        a = np.random.default_rng(11).standard_normal((6, 6))
        s.set_phase_stiffness(1, a @ a.T / 6 + 2.0 * np.eye(6))
    if law == "aniso":
        s.set_phase_conductivity(1, [3.0, 1.5, 0.7, 0.2, -0.1, 0.3])
    s.set_normals(nrm)
    s.set_options(tol=-1.0, abs_tol=-1.0, maxiter=3)
    s.set_options(**opts)
    return s


def golden(grid, call, mode="elasticity", law="iso", complementary=True, mixing_rule="voigt", gamma_scheme="staggered", method="basic",
           u_loop=2, factor="-", **_):
    cls = {"iso": "iso2", "general": "general2", "aniso": "aniso2"}[law] + ("c" if complementary else "")
    return golden_plan(MODE[mode], MIXING[mixing_rule], SCHEME[gamma_scheme], METHOD[method], u_loop, cls, 1, int(grid == TILED), 0, call, factor)


# (grid, call, configuration, the front sweep expected by name: a cross-check of the table look-up itself)
FRONTS = [
    (SMALL, "run", dict(mode="heat"), "ScFast"),
    (TILED, "run", dict(mode="heat", law="aniso"), "ScTileAniso"),
    (SMALL, "run", dict(mode="heat", law="aniso"), "ScExact"),
    (SMALL, "run", dict(mode="heat", u_loop=1), "ScExact"),
    (SMALL, "run", dict(mixing_rule="laminate", u_loop=1), "UStressThenDiv"),
    (SMALL, "iterate", dict(mixing_rule="reuss", u_loop=1), "UStressThenDiv"),
    (TILED, "run", dict(gamma_scheme="full_staggered"), "UTileDfg"),
    (TILED, "run", dict(law="general"), "UTileAniso"),
    (TILED, "run", dict(), "UTilePhi"),
    (TILED, "iterate", dict(mixing_rule="laminate"), "UTilePhi"),
    (TILED, "run", dict(mixing_rule="reuss"), "UTilePhiReuss"),
    (TILED, "run", dict(complementary=False), "UTileModuli"),
    (TILED, "run", dict(mixing_rule="reuss", complementary=False), "UTileModuli"),
    (SMALL, "run", dict(), "UFastModuli"),
    (SMALL, "run", dict(mixing_rule="laminate"), "UFastModuli"),
    (SMALL, "iterate", dict(u_loop=1), "UStressDivVoigt"),
    (SMALL, "run", dict(gamma_scheme="collocated"), "None"),
    (SMALL, "run", dict(gamma_scheme="full_staggered"), "None"),
]


@pytest.mark.parametrize("grid,call,cfg,name", FRONTS, ids=["%s-%s-%s" % (f[3], "x".join(map(str, f[0])), f[1]) for f in FRONTS])
def test_front_sweep_is_the_golden_row_s(grid, call, cfg, name):
    want = golden(grid, call, **cfg)
    assert want["front"] == name
    s = solver(grid, **cfg)
    E = E3 if cfg.get("mode") == "heat" else E6
    if call == "run":
        s.run(E)
    else:
        s.iterate(E, 3)
    assert s.counter("front_sweep") == (FRONT.index(name) if name != "None" else -1)
    assert (s.counter("u_tile_aniso") > 0) == (name == "UTileAniso")
    assert (s.counter("u_tile_reuss") > 0) == (name == "UTilePhiReuss")
    assert (s.counter("sc_tile_aniso") > 0) == (name == "ScTileAniso")
    assert s.counter("cg_dir_sweep") == -1
    assert s.counter("complement_checks") == int(want["complement_check"])   # the device check runs where it ran, and only there
    s.close()


DIRS = [
    (TILED, dict(gamma_scheme="full_staggered"), "UTileDfg"),
    (TILED, dict(law="general"), "UTileAniso"),
    (TILED, dict(), "UTilePhi"),
    (TILED, dict(complementary=False), "UTileModuli"),
    (TILED, dict(mixing_rule="reuss"), "UTileModuli"),
    (TILED, dict(mode="heat"), "ScFast"),
    (TILED, dict(mode="heat", law="aniso"), "ScTileAniso"),
    (TILED, dict(mixing_rule="laminate"), "None"),
    (SMALL, dict(), "None"),
]


@pytest.mark.parametrize("grid,cfg,name", DIRS, ids=["%s-%s" % (d[2], "x".join(map(str, d[0]))) for d in DIRS])
def test_cg_direction_sweep_is_the_golden_row_s(grid, cfg, name):
    want = golden(grid, "run", method="cg", **cfg)
    assert want["cg_dir"] == name and want["cg"] == ("Scalar" if cfg.get("mode") == "heat" else "DisplacementSpace")
    s = solver(grid, method="cg", **cfg)
    s.run(E3 if cfg.get("mode") == "heat" else E6)
    assert s.counter("cg_dir_sweep") == (FRONT.index(name) if name != "None" else -1)
    assert s.counter("front_sweep") == FRONT.index(want["front"])   # the operator of the first residual
    assert (s.counter("u_tile_aniso") > 0) == (name == "UTileAniso")
    assert (s.counter("sc_tile_aniso") > 0) == (name == "ScTileAniso")
    assert s.counter("complement_checks") == int(want["complement_check"])
    s.close()


# configurations that must not run the device complement check (the golden rows say 0), and their counterparts that do
NO_CHECK = [
    (TILED, "run", dict(gamma_scheme="full_staggered"), 0),
    (TILED, "run", dict(mixing_rule="reuss", reuss_sweep=0, factor="reuss_sweep=0"), 0),
    (TILED, "run", dict(phi_sweep=0, factor="phi_sweep=0"), 0),
    (TILED, "run", dict(law="general", aniso_tile=0, factor="aniso_tile=0"), 0),
    (TILED, "run", dict(mode="heat", law="aniso", aniso_sc_tile=0, factor="aniso_sc_tile=0"), 0),
    (SMALL, "run", dict(), 0),
    (SMALL, "run", dict(law="general"), 0),
    (TILED, "run", dict(mode="heat"), 0),
    (TILED, "run", dict(mode="viscosity"), 0),
    (TILED, "run", dict(method="cg", error_estimator="sigma", factor="estimator=sigma"), 0),
    (TILED, "run", dict(method="cg", mixing_rule="reuss", reuss_sweep=0, factor="reuss_sweep=0"), 0),
    (TILED, "run", dict(mixing_rule="reuss"), 1),
    (TILED, "run", dict(method="cg", mixing_rule="reuss"), 1),
    (TILED, "run", dict(law="general", complementary=False), 1),
    (TILED, "iterate", dict(complementary=False), 1),
]


@pytest.mark.parametrize("grid,call,cfg,checks", NO_CHECK, ids=["%d-%s-%s" % (c[3], "x".join(map(str, c[0])), "-".join("%s=%s" % kv for kv in c[2].items() if kv[0] != "factor") or "default") for c in NO_CHECK])
def test_complement_check_runs_where_the_golden_row_says(grid, call, cfg, checks):
    want = golden(grid, call, **cfg)
    assert int(want["complement_check"]) == checks
    s = solver(grid, **{k: v for k, v in cfg.items() if k != "factor"})
    E = E3 if cfg.get("mode") == "heat" else E6
    s.run(E) if call == "run" else s.iterate(E, 3)
    assert s.counter("complement_checks") == checks
    s.close()


REFUSED = [
    (dict(mixing_rule="reuss", error_estimator="energy"), "run", dict(mixing_rule="reuss", factor="estimator=energy"),
     "error_estimator energy is not available with mixing_rule reuss (Reuss MaterialLaw energy not implemented)"),
    (dict(law="general", mixing_rule="laminate"), "iterate", dict(law="general", mixing_rule="laminate"),
     "general (anisotropic) phases support Voigt mixing only (the laminate split is written for isotropic phases)"),
    (dict(mode="heat", gamma_scheme="willot"), "iterate", dict(mode="heat", gamma_scheme="willot"),
     "gamma_scheme willot is not available in heat / porous mode (the reference has no such operator)"),
    (dict(method="polarization", error_estimator="sigma"), "run", dict(method="polarization", factor="estimator=sigma"),
     "method polarization supports error_estimator epsilon and none only (not sigma / energy / residual: the loop's field is the "
     "polarisation, not the strain)"),
]


@pytest.mark.parametrize("cfg,call,row,message", REFUSED, ids=["reuss-energy", "general-laminate", "willot-heat", "polarization-sigma"])
def test_refusals_in_the_golden_row_s_words(cfg, call, row, message):
    assert golden(TILED, call, **row) == "ERR " + message
    s = solver(TILED, **cfg)   # (LSSolver hands the options to the library as they are: the refusal is the entry point's)
    E = E3 if cfg.get("mode") == "heat" else E6
    with pytest.raises(RuntimeError) as err:
        s.run(E) if call == "run" else s.iterate(E, 2)
    assert message in str(err.value)
    assert s.counter("front_sweep") == -1
    s.close()


def test_a_live_solver_across_the_switches():
    """phi_sweep 1 -> 0, then a phase field that is not the complement of the other: UTilePhi -> UTileModuli, and it stays"""
    s = solver(TILED)
    s.iterate(E6, 3)
    assert s.counter("front_sweep") == FRONT.index(golden(TILED, "iterate")["front"]) == FRONT.index("UTilePhi")
    s.set_options(phi_sweep=0)
    s.iterate(E6, 2)
    assert s.counter("front_sweep") == FRONT.index(golden(TILED, "iterate", factor="phi_sweep=0")["front"]) == FRONT.index("UTileModuli")
    s.set_options(phi_sweep=1)
    f0, _, _ = fields(TILED, complementary=False)
    s.set_phase(0, 0.4, 0.6, f0)
    s.iterate(E6, 2)
    assert s.counter("front_sweep") == FRONT.index(golden(TILED, "iterate", complementary=False)["front"]) == FRONT.index("UTileModuli")
    s.iterate(E6, 2)
    assert s.counter("front_sweep") == FRONT.index("UTileModuli")
    s.close()
