"""tests/state_model.py checked without a GPU: for every oracle the model wraps, n chained single passes are the oracle's own
n-pass run, and a reconfiguration followed by a pass is a fresh oracle of the new configuration started from the same field;
the six seeded walks cover the alphabet and the written list of ordered pairs, and the model can play every one of them."""
import numpy as np
import pytest

import aniso_reference as ar
import general_reference as gr
import polarization_reference as pr
import state_model as sm
from helpers import INCLUSION, MATRIX, lame, rel_err, sphere_normals, sphere_phi
from oracle.ls_oracle import LSOracle
from oracle.viscosity_oracle import ViscosityOracle
from willot_reference import WillotLSOracle, WillotViscosityOracle

GRID, DIMS = (6, 5, 8), (1.0, 1.5, 0.8)
E6 = np.array([1.0, 0, 0, 0, 0, 0.5])
PHI = sphere_phi(GRID, R=0.33)
PHIS = [1.0 - PHI, PHI]
ISO = [lame(**MATRIX), lame(**INCLUSION)]
FIXED = dict(tol=-1.0, abs_tol=-1.0)      # the oracle's own n-pass run: no tolerance ends it, maxiter = n does

# name -> (mode, model mats, options, oracle factory)
CASES = {
    "staggered": ("elasticity", ISO, {}, lambda kw: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, **kw)),
    "collocated": ("elasticity", ISO, dict(gamma_scheme="collocated"),
                   lambda kw: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, gamma_scheme="collocated", **kw)),
    "willot": ("elasticity", ISO, dict(gamma_scheme="willot"), lambda kw: WillotLSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, **kw)),
    "laminate": ("elasticity", ISO, dict(mixing_rule="laminate"),
                 lambda kw: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, normals=sphere_normals(GRID), mixing_rule="laminate", **kw)),
    "laminate-willot": ("elasticity", ISO, dict(mixing_rule="laminate", gamma_scheme="willot"),
                        lambda kw: WillotLSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, normals=sphere_normals(GRID),
                                                  mixing_rule="laminate", **kw)),
    "general": ("elasticity", [ISO[0], gr.distinct_stiffness(3.0)], {},
                lambda kw: gr.GeneralLSOracle(*GRID, *DIMS, mats=[ISO[0], gr.distinct_stiffness(3.0)], phis=PHIS, **kw)),
    "viscosity": ("viscosity", [(1.0, 0.0), (0.05, 0.0)], {},
                  lambda kw: ViscosityOracle(*GRID, *DIMS, mats=[(1.0, 0.0), (0.05, 0.0)], phis=PHIS, **kw)),
    "viscosity-willot": ("viscosity", [(1.0, 0.0), (0.05, 0.0)], dict(gamma_scheme="willot"),
                         lambda kw: WillotViscosityOracle(*GRID, *DIMS, mats=[(1.0, 0.0), (0.05, 0.0)], phis=PHIS,
                                                          gamma_scheme="willot", **kw)),
    "heat": ("heat", [(1.0, 0.0), (8.0, 0.0)], {},
             lambda kw: ar.AnisoScalarOracle(*GRID, mus=[1.0, 8.0], phis=PHIS, dx=DIMS[0], dy=DIMS[1], dz=DIMS[2], **kw)),
}
K3 = ar.random_spd3(np.random.default_rng(5), 4.0)


def model(name, **opts):
    mode, mats, o, _ = CASES[name]
    m = sm.StateModel(GRID, DIMS, mats=mats, phis=PHIS, normals=sphere_normals(GRID))
    m.set_options(mode=mode, **o)
    m.set_options(**opts)
    return m


def load(name):
    return E6[:3] if CASES[name][0] == "heat" else E6


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [1, 4])
def test_chained_passes_are_the_oracle_s_own_run(name, n):
    o = CASES[name][3](dict(maxiter=n, **FIXED))
    assert o.run(load(name)) is False and o.iterations == n
    m = model(name)
    m.calc_ref_material()
    assert m.mu_0 == o.mu_0
    for _ in range(n):
        m.iterate(load(name), 1)
    assert rel_err(m.eps, o.eps) <= 1e-13
    assert rel_err(m.mean_stress(), o.mean_stress()) <= 1e-13
    # and the model's run is that run
    r = model(name, maxiter=n, **FIXED)
    assert r.run(load(name)) is False and r.iterations == n
    assert np.array_equal(r.eps, o.eps) and r.residuals == list(o.residuals) and r.mu_0 == o.mu_0


def test_chained_passes_heat_aniso():
    mus = [1.0, K3]
    o = ar.AnisoScalarOracle(*GRID, mus=mus, phis=PHIS, dx=DIMS[0], dy=DIMS[1], dz=DIMS[2], maxiter=3, **FIXED)
    assert o.run(E6[:3]) is False
    m = model("heat")
    m.set_phase_conductivity(1, ar.k6(K3))
    m.calc_ref_material()
    for _ in range(3):
        m.iterate(E6[:3], 1)
    assert rel_err(m.eps, o.eps) <= 1e-13


@pytest.mark.parametrize("scheme", ["staggered", "collocated", "willot"])
@pytest.mark.parametrize("held", [True, False])
def test_chained_polarization_passes(scheme, held):
    """fg_iterate under method polarization: calls with nothing between them continue from the held polarisation and are the
    oracle's own run; a read between them settles the state, and the next call starts from 4 mu_0 E again"""
    mats = [ISO[0], gr.distinct_stiffness(3.0)]
    o = pr.PolarizationOracle(*GRID, *DIMS, mats=mats, phis=PHIS, gamma_scheme=scheme, maxiter=3, **FIXED)
    assert o.run_polarization(E6) is False and o.iterations == 3
    m = sm.StateModel(GRID, DIMS, mats=mats, phis=PHIS, gamma_scheme=scheme, method="polarization")
    m.calc_ref_material()
    assert m.mu_0 == o.mu_0
    for _ in range(3):
        m.iterate(E6, 1)
        if not held:
            m.get_field("epsilon")
    if held:
        assert rel_err(m.eps, o.eps) <= 1e-13
        r = sm.StateModel(GRID, DIMS, mats=mats, phis=PHIS, gamma_scheme=scheme, method="polarization", maxiter=3, **FIXED)
        assert r.run(E6) is False and r.iterations == 3 and np.array_equal(r.eps, o.eps)
    else:
        one = pr.PolarizationOracle(*GRID, *DIMS, mats=mats, phis=PHIS, gamma_scheme=scheme, maxiter=1, **FIXED)
        one.run_polarization(E6)
        assert rel_err(m.eps, one.eps) <= 1e-13


@pytest.mark.parametrize("method", ["basic", "cg", "polarization"])
def test_a_callback_stops_the_model_s_run_like_maxiter(method):
    name = "staggered"
    a, b = model(name, method=method, tol=1e-12), model(name, method=method, tol=1e-12)
    assert sm.run_stopped(a, E6, 3) is False
    # the basic and the polarisation loop count from 1, the CG loop from 0 (F:21716-21805, F:23153-23247)
    assert sm.run_maxiter(b, E6, 2 if method == "cg" else 3) is False
    assert a.iterations == b.iterations and np.array_equal(a.eps, b.eps) and a.residuals == b.residuals


RECONFIGURATIONS = {
    # name -> (start case, calls on the model, the fresh oracle of the new configuration given (mu_0))
    "moduli": ("staggered", [sm.C("set_phase", 0, 2.3, 1.1)],
               lambda mu_0: LSOracle(*GRID, *DIMS, mats=[(2.3, 1.1), ISO[1]], phis=PHIS, mu_0=mu_0)),
    "fractions": ("staggered", [sm.C("set_phase", 1, *ISO[1], 0.5 * PHI)],
                  lambda mu_0: LSOracle(*GRID, *DIMS, mats=ISO, phis=[PHIS[0], 0.5 * PHI], mu_0=mu_0)),
    "laminate": ("staggered", [sm.C("set_options", mixing_rule="laminate")],
                 lambda mu_0: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, normals=sphere_normals(GRID), mixing_rule="laminate", mu_0=mu_0)),
    "collocated": ("staggered", [sm.C("set_options", gamma_scheme="collocated")],
                   lambda mu_0: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, gamma_scheme="collocated", mu_0=mu_0)),
    "willot": ("collocated", [sm.C("set_options", gamma_scheme="willot")],
               lambda mu_0: WillotLSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, mu_0=mu_0)),
    "general": ("staggered", [sm.C("set_phase_stiffness", 1, gr.distinct_stiffness(3.0))],
                lambda mu_0: gr.GeneralLSOracle(*GRID, *DIMS, mats=[ISO[0], gr.distinct_stiffness(3.0)], phis=PHIS, mu_0=mu_0)),
    "iso-again": ("general", [sm.C("set_phase", 1, *ISO[1])], lambda mu_0: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, mu_0=mu_0)),
    "kernel-options": ("staggered", [sm.C("set_options", u_loop=0, u_tile=0, fuse_x=0, plane_fft=0, x_layout=1, pair_chunk=4)],
                       lambda mu_0: LSOracle(*GRID, *DIMS, mats=ISO, phis=PHIS, mu_0=mu_0)),
    "conductivity": ("heat", [sm.C("set_phase_conductivity", 1, ar.k6(K3))],
                     lambda mu_0: ar.AnisoScalarOracle(*GRID, mus=[1.0, K3], phis=PHIS, dx=DIMS[0], dy=DIMS[1], dz=DIMS[2], mu_0=mu_0)),
    "viscosity-moduli": ("viscosity", [sm.C("set_phase", 1, 0.2, 0.0)],
                         lambda mu_0: ViscosityOracle(*GRID, *DIMS, mats=[(1.0, 0.0), (0.2, 0.0)], phis=PHIS, mu_0=mu_0)),
}


@pytest.mark.parametrize("name", sorted(RECONFIGURATIONS))
def test_reconfiguration_then_a_pass_is_a_fresh_oracle_from_the_same_field(name):
    start, calls, fresh = RECONFIGURATIONS[name]
    m = model(start)
    m.calc_ref_material()
    m.iterate(load(start), 2)
    field = m.eps.copy()
    for c in calls:
        sm.call(m, *c)
    assert np.array_equal(m.eps, field)            # a reconfiguration leaves the state alone
    E2 = np.array([0.2, -0.5, 0.3, 0.1, 0.4, -0.2])[:m.ncomp]
    m.iterate(E2, 1)
    o = fresh(m.mu_0)
    assert rel_err(m.eps, o.basic_scheme(E2, field)) <= 1e-13
    assert np.array_equal(field, m.get_field("epsilon")) is False


def test_reads_and_switches_leave_the_state_alone():
    m = model("staggered")
    m.calc_ref_material()
    m.iterate(E6, 2)
    field = m.eps.copy()
    assert m.get_field("sigma").shape == (6,) + GRID and m.get_field("u").shape == (3,) + GRID and m.mean_stress().shape == (6,)
    m.set_normals(sphere_normals(GRID))
    m.set_bc_projector(sm.P_UNIAXIAL)
    m.set_options(method="cg", mixing_rule="laminate", gamma_scheme="willot", u_loop=1)
    assert np.array_equal(m.eps, field)
    with pytest.raises(KeyError):
        m.set_options(no_such_option=1)


# ---------------------------------------------------------------------- the walk
def walks():
    return [sm.walk(seed) for seed in sm.SEEDS]


def test_walks_cover_the_alphabet_and_the_required_pairs():
    ops, pairs, values = set(), set(), set()
    for grid, dims, steps in walks():
        assert len(steps) == sm.WALK_LENGTH
        names = [s.op for s in steps]
        ops.update(names)
        pairs.update(zip(names, names[1:]))
        for s in steps:
            for name, args, kw in s.calls:
                values.update("%s=%s" % kv for kv in kw.items() if name == "set_options" and not isinstance(kv[1], list))
    assert ops == set(sm.ALPHABET)
    missing = [p for p in sm.required_pairs() if p not in pairs]
    assert not missing, missing
    assert len(sm.required_pairs()) == 2 * len(sm.ALPHABET)
    # what the draws of the option steps reached over the six seeds (a change of the seeds must not lose these)
    keys = {v.split("=")[0] for v in values}
    assert keys >= {"mixing_rule", "gamma_scheme", "method", "mode", "u_loop", "u_tile", "fuse_x", "plane_fft", "x_layout", "pair_chunk"}
    assert "mixing_rule=laminate" in values and "method=cg" in values
    assert any(v.startswith("gamma_scheme=") and v != "gamma_scheme=staggered" for v in values)
    assert any(v.startswith("u_loop=") and v != "u_loop=2" for v in values)
    assert {g for g, _, _ in walks()} == {g for g, _ in sm.WALK_GRIDS}


def test_walks_are_reproducible():
    a, b = sm.walk(3), sm.walk(3)
    assert [s.op for s in a[2]] == [s.op for s in b[2]]
    assert all(np.array_equal(x.calls[0][1][-1], y.calls[0][1][-1]) for x, y in zip(a[2], b[2]) if x.op == "set_field")


@pytest.mark.parametrize("seed", list(sm.SEEDS))
def test_the_model_plays_every_walk(seed):
    """every legal draw is one the oracle set can model: the model runs the whole script (on a small grid of the same kind of
    configuration the values do not matter here, the calls do)"""
    grid, dims, steps = sm.walk(seed)
    from helpers import two_phase_setup
    mats, phis, normals = two_phase_setup(grid)
    m = sm.StateModel(grid, dims, mats=mats, phis=phis, normals=normals, tol=1e-3)
    m.set_field("epsilon", np.random.default_rng(seed).standard_normal((6,) + grid))
    m.calc_ref_material()
    for s in steps:
        for c in s.calls:
            sm.call(m, *c)
        assert np.isfinite(m.eps).all(), s.label
        assert m.eps.shape == (m.ncomp,) + grid
