"""SHA-256 of the residual history and of the final epsilon field for a fixed list of short runs (tol = abs_tol = -1,
maxiter = 5: every run makes the same five passes whatever it computes).  Two builds that print the same lines enqueue the same
arithmetic on every path the list reaches: the check for a change that must leave every iterate bit-identical.

    python tools/pass_digest.py > profiles/pass_digest_<build>.txt
    python tools/pass_digest.py tiles > profiles/pass_digest_tiles_<build>.txt     (a second list: the tiled marching sweeps)
    python tools/pass_digest.py fft > profiles/pass_digest_fft_<build>.txt         (a third: every transform family per axis)
    python tools/pass_digest.py reuss > profiles/pass_digest_reuss_<build>.txt     (a fourth: mixing_rule reuss on every sweep)
    python tools/pass_digest.py slab > profiles/pass_digest_slab_<build>.txt       (a fifth: groups of 1, 2 and 4 slabs on one GPU)
    python tools/pass_digest.py steps > profiles/pass_digest_steps_<build>.txt     (a sixth: load paths on the lone solver)

One line per run: grid, name, the digest of the residuals, the digest of the field and the iteration count -- or the solver's
error text where a combination is refused (a refusal is part of the behaviour that is compared)."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from fibergen_amd import LSSolver  # noqa: E402

FIXED = dict(tol=-1.0, abs_tol=-1.0, maxiter=5)
E6 = np.array([0.5, -0.2, 0.1, 0.05, -0.1, 0.3])
E3 = np.array([1.0, -0.5, 0.25])
# sigma_11 prescribed, the other five strains prescribed
P_MIXED = np.diag([0.0, 1.0, 1.0, 0.5, 0.5, 0.5])
E_MIXED = np.array([0.0, -0.2, 0.1, 0.05, -0.1, 0.3])
S_MIXED = np.array([0.1, 0, 0, 0, 0, 0.0])
P3_MIXED = np.diag([0.0, 1.0, 1.0, 0.5, 0.5, 0.5])   # heat: flux component 1 prescribed
E3_MIXED = np.array([0.0, -0.5, 0.25])
S3_MIXED = np.array([0.2, 0.0, 0.0])
COUNTERS = ()   # solver counters printed behind a line where they are non-zero (the tiles list: the anisotropic tile kernels)


def geometry(grid):
    """a blurred sphere (fractions strictly between 0 and 1 on its surface, so laminate mixing has work) and its normals"""
    ax = [(np.arange(n) + 0.5) / n - 0.5 for n in grid]
    v = np.stack(np.broadcast_arrays(ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :])).astype(np.float64)
    r = np.sqrt((v * v).sum(axis=0))
    phi = np.clip(0.5 + (0.3 - r) * 6.0, 0.0, 1.0)
    rr = np.where(r == 0, 1.0, r)
    return phi, v / rr


def general_stiffness():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((6, 6))
    return a @ a.T / 6 + 2.0 * np.eye(6)


def solver(grid, mode="elasticity", mats=((0.4, 0.6), (4.0, 2.5)), normals=False, general=False, aniso=False, fine=False, group=0,
           **opts):
    phi, nrm = geometry(grid)
    if group:   # all slabs of the problem on this GPU, below the C ABI
        from fibergen_amd.distributed import SlabGroup
        s = SlabGroup(*grid, nranks=group)
    else:
        s = LSSolver(*grid)
    s.set_options(mode=mode)
    if "gamma_scheme" in opts:
        s.set_options(gamma_scheme=opts.pop("gamma_scheme"))
    s.set_num_phases(2)
    for p, f in enumerate((1.0 - phi, phi)):
        s.set_phase(p, mats[p][0], mats[p][1], f)
        if fine:
            s.set_phase_fine(p, np.repeat(np.repeat(np.repeat(f, 2, 0), 2, 1), 2, 2))
    if general:
        s.set_phase_stiffness(1, general_stiffness())
    if aniso:
        s.set_phase_conductivity(1, [3.0, 1.5, 0.7, 0.2, -0.1, 0.3])
    if normals:
        s.set_normals(nrm)
    s.set_options(**FIXED)
    s.set_options(**opts)
    return s


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def report(name, grid, E=E6, mixed=False, params=None, callback=False, **kw):
    """params: a load path (run_load_steps from its first entry) instead of one run; callback: a convergence callback that never
    asks to stop (a group of several slabs then votes after every pass)"""
    tag = "%s %s" % ("x".join(map(str, grid)), name)
    try:
        s = solver(grid, **kw)
        if mixed:
            s.set_bc_projector(P_MIXED)
            E = E3_MIXED if len(E) == 3 else E_MIXED
        if callback:
            s.set_convergence_callback(lambda: False)
        S = (S3_MIXED if len(E) == 3 else S_MIXED) if mixed else None
        if params:
            s.run_load_steps(E, S, params=params, first=0)
        else:
            s.run(E, S)
        reached = "".join(" %s=%d" % (c, s.counter(c)) for c in COUNTERS if s.counter(c) > 0)
        print("%s: %s %s %d%s" % (tag, digest(s.residuals), digest(s.get_field("epsilon")), s.iterations, reached))
        s.close()
    except Exception as exc:   # noqa: BLE001
        print("%s: ERROR %s" % (tag, str(exc).splitlines()[0] if str(exc) else type(exc).__name__))
    sys.stdout.flush()


def opts(o):
    return " ".join("%s=%s" % kv for kv in o.items()) or "defaults"


# the schedules of the transform chain; the plane kernel needs ny >= 16, the x layout rows of 64 points
CHAIN = [dict(fuse_x=0, plane_fft=0), dict(plane_fft=0), dict(), dict(fuse_x=0), dict(plane_fft=0, pair_chunk=4),
         dict(fuse_x=0, plane_fft=0, pair_chunk=4), dict(plane_fft=0, x_layout=1), dict(plane_fft=0, x_layout=1, pair_chunk=4)]
G16, G64, GODD, G32 = (16, 8, 16), (16, 16, 64), (12, 10, 7), (32, 32, 32)
VISC = dict(mode="viscosity", mats=((1.0, 0.0), (0.05, 0.0)))
HEAT = dict(mode="heat", mats=((1.0, 0.0), (7.0, 0.0)), E=E3)
LAM = dict(normals=True, mixing_rule="laminate")


def features(grid, full):
    """every operator and loop on one grid; full: with each of its variants, else its default form"""
    for ul in (0, 1, 2) if full else (2,):
        report("laminate u_loop=%d" % ul, grid, u_loop=ul, **LAM)
    report("laminate mixed bc", grid, mixed=True, **LAM)
    # mixed boundary conditions and bc_relax on the three schemes, full_staggered
    for scheme, ul in (("staggered", 0), ("staggered", 2), ("collocated", 2), ("willot", 2)):
        o = dict(gamma_scheme=scheme, u_loop=ul)
        report("%s u_loop=%d mixed bc" % (scheme, ul), grid, mixed=True, **o)
        if ul == 2:
            report("%s mixed bc bc_relax=0.5" % scheme, grid, mixed=True, bc_relax=0.5, **o)
        if full and scheme != "willot":
            report("%s u_loop=%d bc_relax=0.5" % (scheme, ul), grid, bc_relax=0.5, **o)
        if scheme != "staggered":
            report(scheme, grid, gamma_scheme=scheme)
    for ul in (0, 2) if full else (2,):
        report("full_staggered u_loop=%d" % ul, grid, gamma_scheme="full_staggered", fine=True, u_loop=ul)
    report("full_staggered mixed bc", grid, mixed=True, gamma_scheme="full_staggered", fine=True)
    # viscosity: fused, unfused, mixed boundary conditions, willot, full_staggered
    for sd in (0, 1):
        report("viscosity fuse_stress_div=%d" % sd, grid, fuse_stress_div=sd, **VISC)
        report("viscosity fuse_stress_div=%d mixed bc" % sd, grid, mixed=True, fuse_stress_div=sd, **VISC)
        if full:
            report("viscosity fuse_stress_div=%d u_loop=0" % sd, grid, fuse_stress_div=sd, u_loop=0, **VISC)
            report("viscosity full_staggered fuse_stress_div=%d" % sd, grid, gamma_scheme="full_staggered", fine=True, fuse_stress_div=sd,
                   **VISC)
    report("viscosity willot", grid, gamma_scheme="willot", **VISC)
    report("viscosity willot mixed bc", grid, mixed=True, gamma_scheme="willot", **VISC)
    # heat, with and without an aniso phase
    for an in (0, 1):
        for ul in (1, 2) if full else (2,):
            for c in CHAIN[:6] if full and not an else CHAIN[:2]:
                report("heat aniso=%d u_loop=%d %s" % (an, ul, opts(c)), grid, aniso=an, u_loop=ul, **c, **HEAT)
        report("heat aniso=%d mixed bc" % an, grid, mixed=True, aniso=an, **HEAT)
        report("heat aniso=%d cg" % an, grid, aniso=an, method="cg", **HEAT)
    # a general phase
    for scheme, ul in (("staggered", 0), ("staggered", 2), ("collocated", 2), ("willot", 2)):
        report("general %s u_loop=%d" % (scheme, ul), grid, general=True, gamma_scheme=scheme, u_loop=ul)
    if full:
        report("general aniso_tile=0", grid, general=True, aniso_tile=0)
        report("general mixed bc", grid, mixed=True, general=True)
    # conjugate gradients: strain space, displacement space (four kernels / fused sweeps); the scalar form is above
    report("cg u_loop=0", grid, method="cg", u_loop=0)
    for cf in (0, 1):
        report("cg cg_fused=%d" % cf, grid, method="cg", cg_fused=cf)
        if full:
            report("cg laminate cg_fused=%d" % cf, grid, method="cg", cg_fused=cf, **LAM)
    if full:
        report("cg x_layout=1 plane_fft=0", grid, method="cg", x_layout=1, plane_fft=0)
        report("cg mixed bc", grid, mixed=True, method="cg")
        report("cg collocated", grid, method="cg", gamma_scheme="collocated")
        report("cg general", grid, method="cg", general=True)
    # method polarization on the three schemes
    for scheme in ("staggered", "collocated", "willot"):
        for gen in (0, 1) if full else (0,):
            report("polarization %s general=%d" % (scheme, gen), grid, method="polarization", gamma_scheme=scheme, general=gen)


def main():
    # elasticity, staggered: the sweeps (u_loop, fuse_stress_div) against every schedule of the chain
    for ul in (0, 1, 2):
        for c in CHAIN:
            report("stag u_loop=%d %s" % (ul, opts(c)), G64, u_loop=ul, **c)
        for grid in (G16, G64, GODD):
            report("stag u_loop=%d fuse_stress_div=0" % ul, grid, u_loop=ul, fuse_stress_div=0)
        for grid in (G16, GODD):
            for fx in (0, 1):
                report("stag u_loop=%d fuse_x=%d plane_fft=0" % (ul, fx), grid, u_loop=ul, fuse_x=fx, plane_fft=0)
    for c in CHAIN[4:]:   # options the small grid does not take: the chain falls back
        report("stag %s" % opts(c), G16, **c)
    for grid in ((1, 8, 16), (1, 1, 16)):   # no x pass / neither x nor y pass
        for fx in (0, 1):
            report("stag fuse_x=%d" % fx, grid, fuse_x=fx)
            report("heat fuse_x=%d" % fx, grid, fuse_x=fx, **HEAT)
    features(G64, True)
    features(G16, False)
    # the untiled sweeps and the generic transforms once more per operator; 32^3: two waves per row, more than one block everywhere
    for grid in (GODD, G32):
        for name, o in (("laminate", LAM), ("collocated mixed bc bc_relax=0.5", dict(gamma_scheme="collocated", mixed=True, bc_relax=0.5)),
                        ("willot", dict(gamma_scheme="willot")), ("viscosity mixed bc", dict(mixed=True, **VISC)), ("heat", HEAT),
                        ("cg", dict(method="cg")), ("polarization collocated", dict(method="polarization", gamma_scheme="collocated"))):
            report(name, grid, **o)


def tiles():
    """the tiled marching sweeps (grids with nz/2 >= 40, ny >= 14, nx >= 4), which the list above does not reach: every one of
    the six kernels on the three tile shapes -- general tiles of 62 pairs, one wave per row, two waves per row"""
    global COUNTERS
    COUNTERS = ("u_tile_aniso", "sc_tile_aniso")
    for grid in ((4, 16, 80), (6, 14, 128), (4, 14, 256)):
        report("default", grid)                                   # k_u_tile PHI2
        report("laminate", grid, **LAM)
        report("mixed bc", grid, mixed=True)                      # SUMT
        report("phi_sweep=0", grid, phi_sweep=0)                  # the precomputed moduli instead of PHI2
        for ul in (0, 2):                                         # NMOD = 5; u_loop 0: k_eps_tile
            report("full_staggered u_loop=%d" % ul, grid, gamma_scheme="full_staggered", fine=True, u_loop=ul)
        report("viscosity", grid, **VISC)                         # k_eps_tile, NMOD = 2
        report("general", grid, general=True)                     # ANISO (4x14x256: the general tiles)
        report("general mixed bc", grid, mixed=True, general=True)
        for cf in (0, 1):                                         # CGP, k_cgu_tile modes 0 and 1
            report("cg cg_fused=%d" % cf, grid, method="cg", cg_fused=cf)
            report("cg general cg_fused=%d" % cf, grid, method="cg", cg_fused=cf, general=True)
        report("cg full_staggered", grid, method="cg", gamma_scheme="full_staggered", fine=True)
        # k_sc_tile (plain, SUMT, CGP), k_sc_tile_aniso, k_sc_cgu_tile.  (aniso=1 with mixed bc does not reach k_sc_tile_aniso
        # -- that kernel has no sums of tau and the solver takes another sweep: those lines show no sc_tile_aniso counter)
        for an in (0, 1):
            report("heat aniso=%d" % an, grid, aniso=an, **HEAT)
            report("heat aniso=%d mixed bc" % an, grid, mixed=True, aniso=an, **HEAT)
            report("heat aniso=%d cg" % an, grid, aniso=an, method="cg", **HEAT)


def fft():
    """every transform family on every axis (fg_fft_route.h): per axis the shortest length of each family and both sides of the
    thresholds (tests/helpers.py fft_route_grids), thin on the other axes.  Three components with the fused x pass, without
    it (the x passes on their own), and one component (heat); Bluestein against the O(n^2) sums on a prime length, the joint
    and the per-component image of the tile kernels' fused x pass"""
    from helpers import fft_route_grids
    global COUNTERS
    COUNTERS = ("fft_path_x", "fft_path_y", "fft_path_z")
    for grid in sorted({g[0] for g in fft_route_grids()}):
        report("stag", grid)
        report("stag fuse_x=0", grid, fuse_x=0)
        report("heat", grid, **HEAT)
    for b in (0, 1):
        for grid in ((67, 8, 16), (8, 67, 16), (8, 8, 134)):
            report("stag bluestein=%d" % b, grid, bluestein=b)
    for j in (0, 1):
        report("stag joint_x=%d" % j, (100, 8, 16), joint_x=j)
        report("heat joint_x=%d" % j, (100, 8, 16), joint_x=j, **HEAT)


def reuss():
    """mixing_rule reuss on the untiled and the tiled grids, methods basic and cg: the exact-order sweep (u_loop 0 / 1), the moduli
    arrays, the in-sweep harmonic form of two complementary phases and its switch (reuss_sweep, phi_sweep), mixed boundary
    conditions, heat and viscosity.  These are digests of RESULTS (residuals, final field), not of the launches; behind a line the
    counter of the in-sweep form"""
    global COUNTERS
    COUNTERS = ("u_tile_reuss",)
    R = dict(mixing_rule="reuss")
    for grid in (G16, GODD, (4, 16, 80), (6, 14, 128)):
        for method in ("basic", "cg"):
            for ul in (0, 1, 2):
                report("reuss %s u_loop=%d" % (method, ul), grid, method=method, u_loop=ul, **R)
            for o in (dict(reuss_sweep=0), dict(phi_sweep=0), dict(u_tile=0), dict(cg_fused=0), dict(fuse_stress_div=0)):
                report("reuss %s %s" % (method, opts(o)), grid, method=method, **o, **R)
        report("reuss mixed bc", grid, mixed=True, **R)
        report("reuss collocated", grid, gamma_scheme="collocated", **R)
        report("reuss heat", grid, **R, **HEAT)
        report("reuss heat cg", grid, method="cg", **R, **HEAT)
        report("reuss viscosity", grid, **R, **VISC)


GSLAB = ((8, 16, 128), (16, 16, 16), (12, 10, 6))   # the displacement loop of the slabs; the strain-state pipeline; its generic transforms


def slab():
    """the slab driver (SlabGroup::run_step, run_cg and the collective measurements) in groups of 1, 2 and 4 members on one GPU.
    A group the grid cannot be cut into, or a feature the slabs refuse, prints its refusal"""
    for grid in GSLAB:
        for P in (1, 2, 4):
            def rep(name, **kw):
                report("P=%d %s" % (P, name), grid, group=P, **kw)
            for method in ("basic", "cg"):
                rep(method, method=method)
                rep("%s laminate" % method, method=method, **LAM)
            rep("heat", **HEAT)
            rep("viscosity", **VISC)
            rep("mixed bc", mixed=True)
            rep("laminate mixed bc", mixed=True, **LAM)
            rep("heat mixed bc", mixed=True, **HEAT)
            rep("two steps", params=(0.5, 1.0))
            rep("three steps laminate", params=(0.25, 0.5, 1.0), **LAM)
            rep("two steps mixed bc", mixed=True, params=(0.5, 1.0))
            rep("update_ref", update_ref=1)
            rep("update_ref mixed bc two steps", mixed=True, update_ref=1, params=(0.5, 1.0))
            for est in ("sigma", "energy"):
                rep("estimator %s" % est, error_estimator=est)
                rep("estimator %s cg" % est, error_estimator=est, method="cg")
            rep("callback", callback=True)
            rep("callback two steps", callback=True, params=(0.5, 1.0))


def steps():
    """load paths on the lone solver (Solver::run_load_steps, the carry pass of a continuing step, the polynomial extrapolation)"""
    PATHS = ((0.5, 1.0), (0.25, 0.5, 1.0), (0.1, 0.3, 0.6, 1.0))
    for grid in (G16, GODD, (4, 16, 80)):
        for path in PATHS:
            for order in (0, 1, 2):
                report("%d steps order=%d" % (len(path), order), grid, params=path, loadstep_extrapolation_order=order)
        report("3 steps laminate order=1", grid, params=PATHS[1], loadstep_extrapolation_order=1, **LAM)
        report("3 steps u_loop=0", grid, params=PATHS[1], u_loop=0)
        report("3 steps cg", grid, params=PATHS[1], method="cg")
        report("3 steps mixed bc", grid, mixed=True, params=PATHS[1])
        report("3 steps laminate mixed bc", grid, mixed=True, params=PATHS[1], **LAM)
        report("3 steps update_ref", grid, params=PATHS[1], update_ref=1)
        report("3 steps update_ref mixed bc", grid, mixed=True, params=PATHS[1], update_ref=1)
        for est in ("sigma", "energy"):
            report("3 steps estimator %s" % est, grid, params=PATHS[1], error_estimator=est)
        # heat with mixed boundary conditions: on G16 and GODD the tiled sweep does not fit and <tau> comes from the flux-mean sweep
        report("3 steps heat", grid, params=PATHS[1], **HEAT)
        report("3 steps heat mixed bc", grid, mixed=True, params=PATHS[1], **HEAT)
        report("equal parameters order=1", grid, params=(0.5, 0.5, 1.0), loadstep_extrapolation_order=1)


if __name__ == "__main__":
    {"tiles": tiles, "fft": fft, "reuss": reuss, "slab": slab, "steps": steps}.get((sys.argv[1:] or [""])[0], main)()
