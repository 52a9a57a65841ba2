"""Basic scheme against method "polarization" on the benchmark RVE, at contrast 10 and 1000.  One JSON line per (size, contrast).

    python tools/polarization_ab.py [--window S] [--sizes 128,256] [--contrasts 10,1000] [--scheme staggered] [--out FILE]

Per line and method: passes per second (fg_time_iterations after one iteration of a run has set the reference medium; the pass
count of a timed window is scaled from a short probe so that a window lasts about --window seconds, five windows per method,
the two methods alternating; median and min / max spread), iterations to tol = 1e-6 (maxiter 20000) and the wall time of that
run (three runs, median and spread).  The two estimators watch different fields (the
strain, the polarisation), so the iteration counts are what a user of either method sees, not a like-for-like accuracy.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fibergen_amd import LSSolver  # noqa: E402
from fibergen_amd.rve import bench_rve  # noqa: E402

MATRIX = (0.3846153846153846, 0.5769230769230769)
E = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


def solver(n, phi, contrast, method, scheme, **opts):
    s = LSSolver(n, n, n)
    s.set_options(method=method, gamma_scheme=scheme, **opts)
    s.set_num_phases(2)
    s.set_phase(0, *MATRIX, 1.0 - phi)
    s.set_phase(1, contrast * MATRIX[0], contrast * MATRIX[1], phi)
    return s


def rate_solver(n, phi, contrast, method, scheme, window):
    s = solver(n, phi, contrast, method, scheme, maxiter=1)
    s.run(E)
    s.time_iterations(E, 3)
    per_pass = s.time_iterations(E, 10) * 1e-4            # seconds per pass, probe
    return s, max(10, int(window / per_pass))


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def measure_pair(n, phi, contrast, scheme, window):
    methods = ("basic", "polarization")
    sv = {m: rate_solver(n, phi, contrast, m, scheme, window) for m in methods}
    rates = {m: [] for m in methods}
    for _ in range(5):                                      # alternate the two methods
        for m in methods:
            s, steps = sv[m]
            rates[m].append(steps / (s.time_iterations(E, steps) * 1e-3))
    out = {}
    for m in methods:
        sv[m][0].close()
        walls, its, failed = [], 0, False
        for _ in range(3):
            s = solver(n, phi, contrast, m, scheme, tol=1e-6, maxiter=20000)
            failed = bool(s.run(E)) or failed
            walls.append(s.solve_time)
            its = s.iterations
            s.close()
        out[m] = {"passes_per_s": {k: round(v, 1) for k, v in spread(rates[m]).items()}, "window_passes": sv[m][1],
                  "iterations": its, "wall_s": {k: round(v, 4) for k, v in spread(walls).items()}, "failed": failed}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.4, help="seconds per timed window")
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--contrasts", default="10,1000")
    ap.add_argument("--scheme", default="staggered")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        phi = bench_rve(n)[0]
        phi = np.ascontiguousarray(phi[1] if np.ndim(phi) == 4 else phi)
        for contrast in [float(x) for x in a.contrasts.split(",")]:
            r = {"n": n, "contrast": contrast, "scheme": a.scheme, "window_s": a.window}
            r.update(measure_pair(n, phi, contrast, a.scheme, a.window))
            lines.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
