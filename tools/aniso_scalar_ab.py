"""Cost of law="aniso" on the benchmark RVE in porous mode: the fibre phase as a 3x3 permeability (the isotropic fibre's own
constant times the identity, so the runs solve the same problem; --oblique: a seeded oblique SPD matrix at contrast 10 instead,
where only the two aniso forms solve the same problem) on the tiled sweep's aniso form (aniso_sc_tile 1), on the exact-order
13-point sweep (aniso_sc_tile 0), and the isotropic run on the tiled sweep.  One JSON line per size on stdout.

    python tools/aniso_scalar_ab.py [--steps K] [--sizes 128,256] [--oblique] [--out FILE]

Per size: iterations per second of the basic scheme (fg_time_iterations, median of five after a warm-up) once one iteration
of a run has set the reference medium, the launches the counter "sc_tile_aniso" reports, and how far the residual histories
of a short run (tol 1e-6) agree.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fibergen_amd import LSSolver  # noqa: E402
from fibergen_amd.rve import bench_rve  # noqa: E402

MUS = [1.0, 10.0]
E = np.array([1.0, -0.5, 0.25])


def oblique_K():
    B = np.random.default_rng(7).standard_normal((3, 3))
    K = B @ B.T + 1.5 * np.eye(3)
    return 10.0 * 3.0 * K / np.trace(K)


def make(n, phi, K, aniso_sc_tile, **kw):
    s = LSSolver(n, n, n)
    s.set_options(mode="porous", method="basic", aniso_sc_tile=aniso_sc_tile, **kw)
    s.set_num_phases(2)
    s.set_phase(0, MUS[0], 0.0, 1.0 - phi)
    if K is not None:
        s.set_phase_conductivity(1, K, phi)
    else:
        s.set_phase(1, MUS[1], 0.0, phi)
    return s


def measure(n, phi, steps, K, aniso_sc_tile):
    s = make(n, phi, K, aniso_sc_tile, maxiter=1)
    s.run(E)
    s.time_iterations(E, 3)
    rate = steps / (float(np.median([s.time_iterations(E, steps) for _ in range(5)])) * 1e-3)
    launches = s.counter("sc_tile_aniso")
    s.close()
    s = make(n, phi, K, aniso_sc_tile, tol=1e-6, maxiter=200)
    s.run(E)
    res = np.array(s.residuals)
    s.close()
    return rate, launches, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--oblique", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K = oblique_K() if a.oblique else MUS[1] * np.eye(3)
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        phi = bench_rve(n)[0]
        phi = np.ascontiguousarray(phi[1] if np.ndim(phi) == 4 else phi)
        r = {"n": n, "steps": a.steps, "oblique": bool(a.oblique)}
        iso, _, h0 = measure(n, phi, a.steps, None, 1)
        tile, r["aniso_tile_launches"], h1 = measure(n, phi, a.steps, K, 1)
        exact, r["aniso_exact_launches"], h2 = measure(n, phi, a.steps, K, 0)
        r["isotropic_it_s"], r["aniso_tile_it_s"], r["aniso_exact_it_s"] = round(iso, 1), round(tile, 1), round(exact, 1)
        r["tile_over_exact"] = round(tile / exact, 3)
        r["tile_over_isotropic"] = round(tile / iso, 3)
        r["iterations"] = [len(h0), len(h1), len(h2)]
        m = min(len(h1), len(h2))
        r["residual_max_diff_tile_exact"] = float(np.abs(h1[:m] - h2[:m]).max())
        if not a.oblique:
            m = min(len(h0), len(h1))
            r["residual_max_diff_tile_isotropic"] = float(np.abs(h0[:m] - h1[:m]).max())
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
