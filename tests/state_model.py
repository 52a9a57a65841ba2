"""Host model of ONE solver taken through a sequence of calls (test infrastructure only, no GPU, no product import).

The reference's state is the strain field eps (the gradient field in the scalar modes); everything else is configuration.
`StateModel` carries the expected eps, the configuration (materials, fractions, normals, options, projector, mu_0) and has
one method per call of LSSolver that the sequences of tests/test_gpu_state_sequences.py use, under LSSolver's names and
signatures, so that one script drives the product and the model alike (`play`).

  * solve calls advance eps with a FRESHLY built oracle of the current configuration started from the carried eps
    (`oracle()`): n chained `basic_scheme` passes for iterate, the oracle's own run / run_cg / run_load_steps /
    run_polarization for whole runs (which zero the field first, as LSSolver::run does, F:21379);
  * every other call (reads, option switches, material changes) leaves eps alone;
  * no expected value ever comes from a product run.

Entry points the oracles lack, added here without touching their numerics: a polarisation run that a convergence callback
stops (`_run_polarization`), and the polarisation passes of fg_iterate (`_iterate_polarization`: from P = 4 mu_0 E, or from
the polarisation the last such call left when nothing has read or changed the state since -- what Solver::iterate does).

The second half is the seeded walk over the same alphabet (`walk`, `ALPHABET`, `required_pairs`).
"""
from __future__ import annotations

import numpy as np

import aniso_reference as ar
import general_reference as gr
import polarization_reference as pr
from oracle.ls_oracle import LSOracle, voigt_id4
from oracle.viscosity_oracle import ViscosityOracle
from willot_reference import WillotLSOracle, WillotViscosityOracle

SCALAR_MODES = ("heat", "porous")
# options that choose kernels, buffers or launch shapes, never values: the model records them and nothing else
KERNEL_OPTIONS = ("u_loop", "u_tile", "fuse_x", "plane_fft", "x_layout", "pair_chunk", "slab_split", "cg_fused",
                  "fuse_stress_div", "phi_sweep", "aniso_tile", "laminate_overlap")
NUMERIC_OPTIONS = ("tol", "abs_tol", "bc_tol", "maxiter", "error_estimator", "mu_0", "ref_scale")


class _Stop(Exception):
    pass


class StateModel:
    def __init__(self, grid, dims=(1.0, 1.0, 1.0), mats=(), phis=(), normals=None, **options):
        self.grid, self.dims = tuple(grid), tuple(dims)
        self.mats = [self._mat(m) for m in mats]           # (mu, lam), a 6 x 6 stiffness or a 3 x 3 conductivity per phase
        self.phis = [np.array(p, dtype=np.float64) for p in phis]
        self.normals = None if normals is None else np.array(normals, dtype=np.float64)
        self.mode = "elasticity"
        self.mixing_rule, self.gamma_scheme, self.method = "voigt", "staggered", "basic"
        self.numeric = {}                                  # tol, maxiter, ... as handed to the oracle
        self.kernel = {}
        self.mu_0 = float("nan")
        self.P = voigt_id4()
        self.callback = None
        self.eps = np.zeros((6,) + self.grid)
        self.E_last = None
        self.held = None                                   # (P, mu_0) of method polarization between two fg_iterate calls
        self.iterations, self.residuals = 0, []
        self.set_options(**options)

    # ------------------------------------------------------------------ configuration
    @staticmethod
    def _mat(m):
        return np.array(m, dtype=np.float64) if np.ndim(m) == 2 else (float(m[0]), float(m[1]))

    @property
    def scalar(self):
        return self.mode in SCALAR_MODES

    @property
    def ncomp(self):
        return 3 if self.scalar else 6

    def _settle(self):
        """whatever reads or changes the state first turns a held polarisation into the strain (ensure_eps, polar_settle);
        eps already is that strain"""
        self.held = None

    def set_phase(self, p, mu, lam, phi=None):
        self._settle()
        self.mats[p] = (float(mu), float(lam))
        if phi is not None:
            self.phis[p] = np.array(phi, dtype=np.float64)

    def set_phase_stiffness(self, p, C):
        self._settle()
        self.mats[p] = np.array(C, dtype=np.float64).reshape(6, 6)

    def set_phase_conductivity(self, p, K, phi=None):
        K = np.asarray(K, dtype=np.float64)
        if K.shape == (6,):
            K = np.array([[K[0], K[5], K[4]], [K[5], K[1], K[3]], [K[4], K[3], K[2]]])
        self.mats[p] = K.copy()
        if phi is not None:
            self.phis[p] = np.array(phi, dtype=np.float64)

    def set_normals(self, normals):
        self.normals = np.array(normals, dtype=np.float64)

    def set_bc_projector(self, P):
        self.P = np.array(P, dtype=np.float64)

    def set_convergence_callback(self, fn):
        self.callback = fn

    def set_options(self, **kw):
        for k, v in kw.items():
            if k == "mode":
                if (v in SCALAR_MODES) != self.scalar:     # the field changes its shape; its content is not defined
                    self.eps = np.zeros((3 if v in SCALAR_MODES else 6,) + self.grid)
                    self.held = None
                self.mode = v
            elif k in ("mixing_rule", "gamma_scheme", "method"):
                setattr(self, k, v)
            elif k in NUMERIC_OPTIONS:
                if k == "mu_0":
                    self.mu_0 = float(v)
                else:
                    self.numeric[k] = v
            elif k in KERNEL_OPTIONS:
                self.kernel[k] = v
            else:
                raise KeyError("StateModel does not know option %r" % k)

    # ------------------------------------------------------------------ the oracle of the current configuration
    def oracle(self):
        kw = {k: v for k, v in self.numeric.items() if k != "error_estimator"}
        kw["mu_0"] = self.mu_0
        phis = [p.copy() for p in self.phis]
        if self.scalar:
            mus = [m.copy() if np.ndim(m) == 2 else m[0] for m in self.mats]
            d = dict(zip(("dx", "dy", "dz"), self.dims))
            o = ar.AnisoScalarOracle(*self.grid, mus=mus, phis=phis, **d, **kw)
            if not np.array_equal(self.P[:3, :3], np.eye(3)):
                o.set_bc_projector(self.P[:3, :3])
        else:
            if "error_estimator" in self.numeric:
                kw["error_estimator"] = self.numeric["error_estimator"]
            mats = [m.copy() if np.ndim(m) == 2 else m for m in self.mats]
            normals = None if self.normals is None else self.normals.copy()
            kw.update(mats=mats, phis=phis, normals=normals, mixing_rule=self.mixing_rule, gamma_scheme=self.gamma_scheme)
            willot = self.gamma_scheme == "willot"
            if self.mode == "viscosity":
                cls = WillotViscosityOracle if willot else ViscosityOracle
            elif self.mixing_rule == "voigt":
                cls = pr.PolarizationOracle     # iso and general phases, staggered / collocated / willot, both loops
            else:
                cls = WillotLSOracle if willot else LSOracle
            o = cls(*self.grid, *self.dims, **kw)
            o.set_bc_projector(self.P)
        o.callback = self.callback
        o.eps = self.eps.copy()
        return o

    def _load(self, E):
        E = np.asarray(E, dtype=np.float64).ravel()
        return E[:3].copy() if self.scalar else E.copy()

    # ------------------------------------------------------------------ reads
    def get_field(self, name):
        self._settle()
        o = self.oracle()
        if name == "epsilon":
            return self.eps.copy()
        if name == "sigma":
            return o.calc_stress(0.0, o.eps) if self.scalar else o.calc_stress(0.0, 0.0, o.eps)
        if name == "u":
            if self.scalar:
                return o.potential()[None]
            return o.velocity() if self.mode == "viscosity" else o.get_field("u")
        raise KeyError(name)

    def mean_stress(self):
        self._settle()
        return self.oracle().mean_stress()

    @property
    def ref_material(self):
        return self.mu_0, 0.0

    # ------------------------------------------------------------------ state
    def set_field(self, name, value):
        if self.scalar:
            raise RuntimeError("fields cannot be set in heat / porous mode")
        if name != "epsilon":
            raise KeyError(name)
        self._settle()
        self.eps = np.array(value, dtype=np.float64)

    def calc_ref_material(self):
        o = self.oracle()
        if self.method == "polarization":
            o.calc_ref_material_polarization()
        else:
            o.calc_ref_material()
        self.mu_0 = o.mu_0
        return self.ref_material

    # ------------------------------------------------------------------ solves
    def iterate(self, E, n):
        E = self._load(E)
        o = self.oracle()
        if self.method == "polarization":
            self._iterate_polarization(o, E, n)
        else:
            self._settle()
            for _ in range(n):
                self.eps = o.basic_scheme(E, self.eps)
        self.E_last = E

    def _iterate_polarization(self, o, E, n):
        if self.held is not None and self.held[1] != self.mu_0:
            self.held = None
        P0 = 4 * self.mu_0 * E
        if self.held is None:
            P = np.empty_like(self.eps)
            P[:] = P0[:, None, None, None]               # polar_start: epsilon.setConstant(4 mu_0 E)  F:21828
        else:
            P = self.held[0]
        for _ in range(n):
            P = o.polarization_scheme(P0, P)
        self.held = (P, self.mu_0)
        self.eps = o.calc_polarization(P, inv=True)

    def _run_polarization(self, o, E):
        """PolarizationOracle.run_polarization, which hands every pass to a callback but cannot be stopped by it: the model's
        convergence callback ends it by an exception, and the strain is converted from the polarisation of that pass"""
        seen = {}

        def cb(it, P):
            seen["it"], seen["P"] = it, P
            if self.callback is not None and self.callback():
                raise _Stop

        try:
            return o.run_polarization(E, callback=cb)
        except _Stop:
            o.iterations = seen["it"]
            o.eps = o.calc_polarization(seen["P"], inv=True)
            return False

    def _adopt(self, o, failed, E):
        self.eps = o.eps.copy()
        self.mu_0 = o.mu_0
        self.iterations = int(o.iterations)
        self.residuals = list(o.residuals)
        self.held = None
        self.E_last = E
        return bool(failed)

    def run(self, E, S=None):
        E = self._load(E)
        o = self.oracle()
        if self.scalar:
            S3 = None if S is None else np.asarray(S, dtype=np.float64).ravel()[:3]
            failed = o.run_cg(E) if self.method == "cg" else o.run(E, S3)
        elif self.method == "polarization":
            o.eps = np.zeros_like(o.eps)                  # LSSolver::run zeroes the field  F:21379
            failed = self._run_polarization(o, E)
        elif self.method == "cg":
            failed = o.run_cg(E, S)
        else:
            failed = o.run(E, S)
        return self._adopt(o, failed, E)

    def run_load_steps(self, E, S=None, params=(0.0, 1.0)):
        if self.scalar or self.method == "polarization":
            raise RuntimeError("StateModel: load steps are modelled for the strain loops of elasticity / viscosity")
        E = self._load(E)
        o = self.oracle()
        failed = o.run_load_steps(E, S, params=list(params), method=self.method)
        return self._adopt(o, failed, E)


def run_stopped(target, E, k):
    """run(E) ended by the convergence callback in iteration k; the same code for the product and the model"""
    n = [0]

    def cb():
        n[0] += 1
        return n[0] >= k

    target.set_convergence_callback(cb)
    try:
        return target.run(E)
    finally:
        target.set_convergence_callback(None)


def run_maxiter(target, E, maxiter, restore=10000):
    target.set_options(maxiter=maxiter)
    try:
        return target.run(E)
    finally:
        target.set_options(maxiter=restore)


# ---------------------------------------------------------------------- scripts
class Step:
    """one step of a script: calls (name, args, kwargs) made on the product and on the model alike; `full_run` marks a whole
    run, after which iterations, residual history and mean stress are compared too.  Names without a method of that name are
    the functions of this module taking the target first (run_stopped, run_maxiter)."""

    def __init__(self, label, *calls, full_run=False, op=None):
        self.label, self.calls, self.full_run, self.op = label, calls, full_run, op or label


def call(target, name, args=(), kw=None):
    fn = getattr(target, name, None)
    if fn is None:
        return globals()[name](target, *args, **(kw or {}))
    return fn(*args, **(kw or {}))


def C(name, *args, **kw):
    return (name, args, kw)


# ---------------------------------------------------------------------- the seeded walk
# One solver, 12 operations, compared with the model after each.  A pure random draw of 72 operations cannot promise the
# pairs below, so the draw is steered: every operation X of the alphabet is dealt once to one of the six seeds (a fixed
# shuffle), a seed plays its X as "run_stopped, X, iterate" -- which covers "run-stopped-early then X" and "X then iterate" --
# and the seed decides the order, the remaining slots (free legal draws) and every parameter.
# The legality rules of fg_solver.hip's refusals are the `legal` function; what is illegal at its turn moves to a later slot
# of the same seed, and `walk` fails (here, on the CPU) rather than drop it.
#
# Not in the alphabet, on purpose:
#   * x_layout / pair_chunk as operations of their own: only the (16, 8, 64) walks accept them; chain_option sets them there.
#   * run_load_steps under method polarization and in heat: PolarizationOracle's load steps and ScalarOracle have no
#     callback / S / first arguments to match LSSolver::run_load_steps call for call; sequence B.4 covers the strain loops.
#   * gamma_scheme full_staggered: needs fine phase fields; tests/test_gpu_dfg_state.py walks that state.
ALPHABET = ("iterate", "run", "run_stopped", "run_maxiter", "run_load_steps", "get_epsilon", "get_sigma", "get_u", "mean_stress",
            "set_field", "calc_ref_material", "set_moduli", "set_fractions", "set_stiffness", "set_normals", "mixing_rule",
            "gamma_scheme", "method", "sweep_option", "chain_option", "bc_projector", "mode")
SEEDS = range(6)
WALK_LENGTH = 12
WALK_GRIDS = [((4, 16, 80), (1.0, 1.5, 0.8)), ((16, 8, 64), (1.0, 1.0, 1.0))]   # tiled sweep / untiled, x_layout accepted
DEAL_SEED = 2026

E_LOADS = [np.array([1.0, 0, 0, 0, 0, 0.5]), np.array([0.2, -0.5, 0.3, 0.1, 0.4, -0.2])]
E_UNIAXIAL = np.array([0.01, 0, 0, 0, 0, 0])
P_UNIAXIAL = np.zeros((6, 6))
P_UNIAXIAL[0, 0] = 1.0


def required_pairs():
    return [(x, "iterate") for x in ALPHABET] + [("run_stopped", x) for x in ALPHABET]


def deal():
    """which seed plays which operation: a fixed shuffle of the alphabet dealt round the seeds, `mode` last in its hand (the
    state across a mode switch is not defined: its step ends in a fresh run and only the closing iterate follows)"""
    rng = np.random.default_rng(DEAL_SEED)
    ops = list(ALPHABET)
    rng.shuffle(ops)
    hands = [[] for _ in SEEDS]
    for i, x in enumerate(ops):
        hands[i % len(hands)].append(x)
    return hands


class _Config:
    """what the generator knows about the solver it is writing a script for"""

    def __init__(self, grid):
        self.grid = grid
        self.mode, self.mixing, self.method, self.scheme = "elasticity", "voigt", "basic", "staggered"
        self.general = False          # phase 1 is a general phase
        self.mixed_bc = False
        self.complementary = True     # phi_0 == 1 - phi_1
        self.x_layout_grid = grid == (16, 8, 64)


def legal(x, c):
    el = c.mode == "elasticity"
    if x == "set_field":
        return c.mode not in SCALAR_MODES                                   # "fields cannot be set in heat / porous mode"
    if x == "set_stiffness":
        return el and c.mixing == "voigt"                                    # law_refusal (fg_sweep_plan.h)
    if x == "run_load_steps":
        return c.mode not in SCALAR_MODES and c.method != "polarization"    # (see above: not modelled)
    if x == "bc_projector":
        return el and c.method != "polarization"                            # polar_refusal (fg_sweep_plan.h): pure strain only
    # the switches (mixing_rule, gamma_scheme, method, mode) are always legal: _draw picks among the values the
    # configuration admits (laminate: two isotropic complementary phases, not under polarization; polarization: Voigt, pure
    # strain, elasticity; collocated: not in viscosity; heat: staggered only)
    return True


def _sphere(grid, rng):
    from helpers import sphere_normals, sphere_phi
    c = tuple(0.5 + 0.1 * (rng.random(3) - 0.5))
    R = 0.25 + 0.1 * rng.random()
    return sphere_phi(grid, R=R, c=c), sphere_normals(grid, c=c)


def _draw(x, c, rng):
    """the step of operation x in configuration c (updated in place)"""
    E = E_UNIAXIAL if c.mixed_bc else E_LOADS[int(rng.integers(2))]
    if c.mode in SCALAR_MODES:
        E = E[:3] if not c.mixed_bc else E
    if x == "iterate":
        return Step(x, C("iterate", E, int(rng.integers(1, 3))))
    if x == "run":
        return Step(x, C("run", E), full_run=True)
    if x == "run_stopped":
        return Step(x, C("run_stopped", E, 2), full_run=True)
    if x == "run_maxiter":
        return Step(x, C("run_maxiter", E, 3), full_run=True)
    if x == "run_load_steps":
        return Step(x, C("run_load_steps", E, params=[0.0, 0.4, 1.0]), full_run=True)
    if x == "get_epsilon":
        return Step(x, C("get_field", "epsilon"))
    if x == "get_sigma":
        return Step(x, C("get_field", "sigma"))
    if x == "get_u":
        return Step(x, C("get_field", "u"))
    if x == "mean_stress":
        return Step(x, C("mean_stress"))
    if x == "set_field":
        return Step(x, C("set_field", "epsilon", rng.standard_normal((6,) + c.grid)))
    if x == "calc_ref_material":
        return Step(x, C("calc_ref_material"))
    if x == "set_moduli":
        p = 1 if c.general else int(rng.integers(2))
        c.general = False
        mu = float(0.5 + 4 * rng.random())
        lam = 0.0 if c.mode != "elasticity" else float(0.5 + 2 * rng.random())
        c.mats[p] = (mu, lam)
        return Step(x, C("set_phase", p, mu, lam))
    if x == "set_fractions":
        phi, _ = _sphere(c.grid, rng)
        # complementary or not (two_phase_complementary has to notice either way); the laminate rule defines c2 := 1 - c1,
        # so it keeps complementary fractions
        c.complementary = c.mixing == "laminate" or bool(rng.integers(2))
        phi0 = 1.0 - phi if c.complementary else 0.9 * (1.0 - phi)
        c.general = False             # set_phase is the only call that takes a field: phase 1 is isotropic again
        return Step(x, C("set_phase", 0, *c.mats[0], phi0), C("set_phase", 1, *c.mats[1], phi))
    if x == "set_stiffness":
        c.general = True
        return Step(x, C("set_phase_stiffness", 1, gr.random_spd(rng)))
    if x == "set_normals":
        return Step(x, C("set_normals", _sphere(c.grid, rng)[1]))
    if x == "mixing_rule":
        ok = c.mode == "elasticity" and not c.general and c.method != "polarization" and c.complementary
        c.mixing = "laminate" if ok and c.mixing == "voigt" else "voigt"
        return Step(x, C("set_options", mixing_rule=c.mixing))
    if x == "gamma_scheme":
        pool = {"elasticity": ["staggered", "collocated", "willot"], "viscosity": ["staggered", "willot"]}.get(c.mode, ["staggered"])
        pool = [s for s in pool if s != c.scheme] or pool
        c.scheme = pool[int(rng.integers(len(pool)))]
        return Step(x, C("set_options", gamma_scheme=c.scheme))
    if x == "method":
        pool = ["basic", "cg"]
        if c.mode == "elasticity" and c.mixing == "voigt" and not c.mixed_bc:
            pool.append("polarization")
        pool = [m for m in pool if m != c.method]
        c.method = pool[int(rng.integers(len(pool)))]
        return Step(x, C("set_options", method=c.method))
    if x == "sweep_option":
        return Step(x, C("set_options", u_loop=int(rng.integers(3)), u_tile=int(rng.integers(2))))
    if x == "chain_option":
        kw = dict(fuse_x=int(rng.integers(2)), plane_fft=int(rng.integers(2)))
        if c.x_layout_grid:
            kw.update(x_layout=int(rng.integers(2)), pair_chunk=4 * int(rng.integers(2)))
        return Step(x, C("set_options", **kw))
    if x == "bc_projector":
        c.mixed_bc = not c.mixed_bc
        return Step(x, C("set_bc_projector", P_UNIAXIAL if c.mixed_bc else voigt_id4()))
    if x == "mode":
        c.mode = ["heat", "viscosity"][int(rng.integers(2))]
        c.mixing, c.scheme, c.general, c.mixed_bc = "voigt", "staggered", False, False
        if c.method == "polarization":
            c.method = "basic"
        mus = [1.0, 0.05] if c.mode == "viscosity" else [1.0, 8.0]
        c.mats = [(mus[0], 0.0), (mus[1], 0.0)]
        El = E_LOADS[0][:3] if c.mode in SCALAR_MODES else E_LOADS[0]
        return Step(x, C("set_options", mode=c.mode, mixing_rule="voigt", gamma_scheme="staggered", method=c.method),
                    C("set_bc_projector", voigt_id4()), C("set_phase", 0, *c.mats[0]), C("set_phase", 1, *c.mats[1]),
                    C("run", El), full_run=True)
    raise KeyError(x)


def walk(seed):
    """(grid, dims, steps) of one seed: WALK_LENGTH operations as triples "run_stopped, X, iterate" """
    from helpers import INCLUSION, MATRIX, lame
    rng = np.random.default_rng(1000 + seed)
    grid, dims = WALK_GRIDS[seed % len(WALK_GRIDS)]
    c = _Config(grid)
    c.mats = [lame(**MATRIX), lame(**INCLUSION)]
    hand = list(deal()[seed])
    rng.shuffle(hand)
    if "mode" in hand:
        hand.remove("mode")
        hand.append("mode")
    free = [x for x in ALPHABET if x != "mode"]
    while len(hand) < WALK_LENGTH // 3:       # the remaining slots: free draws
        hand.insert(int(rng.integers(len(hand) + 1 - ("mode" in hand))), free[int(rng.integers(len(free)))])
    # operations with a precondition go before the switches that could take it away (a stable sort: the seed's order otherwise)
    hand.sort(key=lambda h: 0 if h in ("set_stiffness", "bc_projector", "run_load_steps", "set_field") else (2 if h == "mode" else 1))
    steps = []
    while hand:
        x = next((h for h in hand if legal(h, c)), None)
        if x is None:
            raise RuntimeError("walk %d: no legal order for %r" % (seed, hand))
        hand.remove(x)
        for op in ("run_stopped", x, "iterate"):
            steps.append(_draw(op, c, rng))
    assert len(steps) == WALK_LENGTH
    return grid, dims, steps
