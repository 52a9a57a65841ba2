"""Where the set-up time of FG.run() goes: a <place_fiber> project run four times in one process.
    python tools/setup_cost.py [n=64] [--device-geometry 0|1] [--project hashin|capsules] [--skip-create]
Prints per run: wall time of run(), the solver's own solve time (six load cases), and the difference = set-up (project layer,
voxeliser, fg_create, phase upload), then its breakdown: parse (set_xml), create (settings + fg_create), voxelise, normalise,
upload (clocks this tool wraps around geometry.voxelize, _normalize_phi, LSSolver.set_phase / set_phase_fine / set_normals
and LSSolver.voxelize_into; with --device-geometry 1 the three are that one call, booked under voxelise), solve, rest.
--project capsules places the 126 capsules of bench_rve_parameters(n).  Then the cost of fg_create + fg_destroy alone for a
few grids (first and later calls)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def project(n):
    return """<settings><solver nx="%d" ny="%d" nz="%d"><tol>1e-5</tol><method>cg</method><mixing_rule>voigt</mixing_rule>
      <materials><matrix E="1" nu="0.3" /><coating E="5" nu="0.25" /><inclusion E="10" nu="0.2" /></materials></solver>
      <actions><select_material name="coating" /><place_fiber R="0.4" /><select_material name="inclusion" /><place_fiber R="0.2" />
      <calc_effective_properties /></actions></settings>""" % (n, n, n)


def capsule_project(n):
    """the capsules of the benchmark family (bench_rve_parameters) as <place_fiber> actions; L is the equal-volume length"""
    from fibergen_amd.rve import bench_rve_parameters, place_capsules
    par = bench_rve_parameters(n)
    centres, axes = place_capsules(par["K"], par["R"], par["L"])
    L = par["L"] - 2 * par["R"] + 4 / 3 * par["R"]
    fibers = "".join('<place_fiber type="capsule" cx="%r" cy="%r" cz="%r" ax="%r" ay="%r" az="%r" L="%r" R="%r" />'
                     % (*[float(v) for v in c], *[float(v) for v in a], float(L), float(par["R"])) for c, a in zip(centres, axes))
    return """<settings><solver nx="%d" ny="%d" nz="%d"><tol>1e-5</tol><method>cg</method><mixing_rule>voigt</mixing_rule>
      <materials><matrix E="1" nu="0.3" /><fiber E="10" nu="0.2" /></materials></solver>
      <actions><select_material name="fiber" />%s<calc_effective_properties /></actions></settings>""" % (n, n, n, fibers)


CLOCKS = {"voxelise": 0.0, "normalise": 0.0, "upload": 0.0}


def clocked(fn, key):
    def wrapper(*a, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*a, **kw)
        finally:
            CLOCKS[key] += time.perf_counter() - t0
    return wrapper


def install_clocks():
    """the pieces of FG.init_phase, timed from outside"""
    from fibergen_amd import LSSolver, geometry
    from fibergen_amd import fg as fg_module
    geometry.voxelize = clocked(geometry.voxelize, "voxelise")
    fg_module._normalize_phi = clocked(fg_module._normalize_phi, "normalise")
    LSSolver.voxelize_into = clocked(LSSolver.voxelize_into, "voxelise")
    for name in ("set_phase", "set_phase_fine", "set_normals"):
        setattr(LSSolver, name, clocked(getattr(LSSolver, name), "upload"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=64)
    ap.add_argument("--device-geometry", type=int, choices=(0, 1), default=1)
    ap.add_argument("--project", choices=("hashin", "capsules"), default="hashin")
    ap.add_argument("--skip-create", action="store_true", help="only the FG.run() part")
    args = ap.parse_args()
    n = args.n
    from fibergen_amd import FG, LSSolver
    xml = project(n) if args.project == "hashin" else capsule_project(n)
    install_clocks()
    fg = FG()
    fg.device_geometry = bool(args.device_geometry)
    for i in range(4):
        t0 = time.perf_counter()
        fg.set_xml(xml)
        t1 = time.perf_counter()
        fg.init_lss()
        for k in CLOCKS:   # (set_phase without a field, inside "create", is no upload)
            CLOCKS[k] = 0.0
        t2 = time.perf_counter()
        rc = fg.run()
        t3 = time.perf_counter()
        wall, solve = t3 - t0, fg.get_solve_time()
        print("FG.run #%d %s at %d^3, device_geometry %d: rc %s, wall %.1f ms, solver %.1f ms, set-up %.1f ms" %
              (i, args.project, n, args.device_geometry, rc, 1e3 * wall, 1e3 * solve, 1e3 * (wall - solve)), flush=True)
        parts = [("parse", t1 - t0), ("create", t2 - t1), ("voxelise", CLOCKS["voxelise"]), ("normalise", CLOCKS["normalise"]),
                 ("upload", CLOCKS["upload"]), ("solve", solve)]
        parts.append(("rest", wall - sum(v for _, v in parts)))
        print("    " + ", ".join("%s %.1f" % (k, 1e3 * v) for k, v in parts) + " ms; phase_uploads %d"
              % fg._lss.counter("phase_uploads"), flush=True)
        fg.reset()
    if args.skip_create:
        return
    for g in (32, 64, 128, 256):
        ts = []
        for i in range(4):
            t0 = time.perf_counter()
            s = LSSolver(g, g, g)
            t1 = time.perf_counter()
            s.close()
            t2 = time.perf_counter()
            ts.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
        print("%d^3: create / close ms: %s" % (g, ", ".join("%.1f / %.1f" % t for t in ts)), flush=True)
    # pieces of a run at 64^3 on a live solver
    g = 64
    from helpers import INCLUSION, MATRIX, lame, sphere_phi
    phi = sphere_phi((g, g, g), 0.3)
    s = LSSolver(g, g, g)
    s.set_num_phases(2)
    t0 = time.perf_counter()
    s.set_phase(0, *lame(**MATRIX), 1 - phi)
    s.set_phase(1, *lame(**INCLUSION), phi)
    t1 = time.perf_counter()
    s.set_options(tol=1e-5, method="cg")
    for i in range(3):
        t2 = time.perf_counter()
        s.run(np.array([1.0, 0, 0, 0, 0, 0]))
        t3 = time.perf_counter()
        print("64^3 run #%d: wall %.2f ms, solver-reported %.2f ms, %d iterations" % (i, 1e3 * (t3 - t2), 1e3 * s.solve_time, s.iterations))
    print("64^3 set_phase x2: %.2f ms" % (1e3 * (t1 - t0)))
    s.close()


if __name__ == "__main__":
    main()
