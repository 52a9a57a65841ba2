"""Cost of gamma_scheme full_staggered (the doubly fine grid) against staggered: iterations per second of the same
geometry on both schemes, and the set-up time of the fine voxelisation.  One JSON line per case on stdout.

    python tools/dfg_ab.py [--steps K] [--sizes 128,256] [--out FILE]

Cases: viscosity (basic scheme, CG) at each size, Voigt elasticity (basic scheme) at the largest; a sphere of radius 0.3.
basic: fg_time_iterations (HIP events around K passes); cg: a run of K iterations (tol 0), solve time / iterations.
set-up: <place_fiber> voxelised at n^3 (staggered) against (2n)^3 + the device reduction to the staggered fractions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fibergen_amd import LSSolver, geometry  # noqa: E402
from fibergen_amd.fg import _Fiber, _normalize_phi  # noqa: E402

MATS = {"elasticity": [(0.3846153846153846, 0.5769230769230769), (4.166666666666667, 2.7777777777777777)],
        "viscosity": [(1.0, 0.0), (0.05, 0.0)]}
E = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


def voxelize(n):
    f = _Fiber("capsule", (0.5, 0.5, 0.5), (1.0, 0.0, 0.0), 0.0, 0.3, 1)
    t = time.perf_counter()
    phi, _, _ = geometry.voxelize([f], (n, n, n), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 2, 0)
    phi = _normalize_phi(phi)
    return phi, time.perf_counter() - t


def solver(n, mode, scheme, phi):
    s = LSSolver(n, n, n)
    s.set_options(mode=mode, gamma_scheme=scheme)
    s.set_num_phases(2)
    for p, (mu, lam) in enumerate(MATS[mode]):
        if scheme == "staggered":
            s.set_phase(p, mu, lam, phi[p])
        else:
            s.set_phase(p, mu, lam)
            s.set_phase_fine(p, phi[p])
    return s


def measure(n, mode, method, scheme, phi, steps):
    s = solver(n, mode, scheme, phi)
    if method == "basic":
        s.time_iterations(E, 3)
        best = min(s.time_iterations(E, steps) for _ in range(3))
        its = steps / (best * 1e-3)
    else:
        s.set_options(method="cg", tol=0.0, abs_tol=0.0, maxiter=steps)
        s.run(E)
        s.set_options(maxiter=steps)
        best = None
        for _ in range(3):
            s.run(E)
            r = s.iterations / s.solve_time
            best = r if best is None else max(best, r)
        its = best
    s.close()
    return its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    lines = []
    for n in sizes:
        coarse, t_c = voxelize(n)
        fine, t_f = voxelize(2 * n)
        t = time.perf_counter()
        s = solver(n, "viscosity", "full_staggered", fine)
        s.mean_strain()
        t_up = time.perf_counter() - t
        s.close()
        lines.append({"case": "setup", "n": n, "voxelize_coarse_s": round(t_c, 4), "voxelize_fine_s": round(t_f, 4),
                      "fine_upload_and_reduce_s": round(t_up, 4)})
        print(json.dumps(lines[-1]), flush=True)
        cases = [("viscosity", "basic"), ("viscosity", "cg")]
        if n == max(sizes):
            cases.append(("elasticity", "basic"))
        for mode, method in cases:
            r = {"case": mode, "method": method, "n": n, "steps": a.steps}
            for scheme, phi in (("staggered", coarse), ("full_staggered", fine)):
                r[scheme + "_it_s"] = round(measure(n, mode, method, scheme, phi, a.steps), 1)
            r["time_ratio"] = round(r["staggered_it_s"] / r["full_staggered_it_s"], 3)
            lines.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
