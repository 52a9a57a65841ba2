"""Cost of law="general" on the benchmark RVE: the fibre phase as a 6x6 stiffness (the isotropic fibre's own constants, so the
three runs solve the same problem) with the tiled sweep's anisotropic form (aniso_tile 1), on the strain-state pass
(aniso_tile 0), and the isotropic run (the PHI2 sweep).  One JSON line per size on stdout.

    python tools/general_ab.py [--steps K] [--sizes 128,256] [--out FILE]

Per size: iterations per second of the basic scheme (fg_time_iterations, best of three) after one iteration of a run has set
the reference medium, and the launches the counter "u_tile_aniso" reports.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fibergen_amd import LSSolver  # noqa: E402
from fibergen_amd.rve import bench_rve  # noqa: E402

MATS = [(0.3846153846153846, 0.5769230769230769), (4.166666666666667, 2.7777777777777777)]
E = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


def iso_stiffness(mu, lam):
    C = np.zeros((6, 6))
    C[:3, :3] = lam
    for i in range(3):
        C[i, i] = 2 * mu + lam
        C[3 + i, 3 + i] = mu
    return C


def measure(n, phi, steps, general, aniso_tile):
    s = LSSolver(n, n, n)
    s.set_options(method="basic", maxiter=1, aniso_tile=aniso_tile)
    s.set_num_phases(2)
    s.set_phase(0, *MATS[0], 1.0 - phi)
    s.set_phase(1, *MATS[1], phi)
    if general:
        s.set_phase_stiffness(1, iso_stiffness(*MATS[1]))
    s.run(E)
    s.time_iterations(E, 3)
    best = min(s.time_iterations(E, steps) for _ in range(3))
    launches = s.counter("u_tile_aniso")
    s.close()
    return steps / (best * 1e-3), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        phi = bench_rve(n)[0]
        phi = np.ascontiguousarray(phi[1] if np.ndim(phi) == 4 else phi)
        r = {"n": n, "steps": a.steps}
        r["isotropic_it_s"], _ = measure(n, phi, a.steps, False, 1)
        r["general_tile_it_s"], r["general_tile_launches"] = measure(n, phi, a.steps, True, 1)
        r["general_strain_state_it_s"], r["general_strain_state_launches"] = measure(n, phi, a.steps, True, 0)
        for k in ("isotropic_it_s", "general_tile_it_s", "general_strain_state_it_s"):
            r[k] = round(r[k], 1)
        r["tile_over_strain_state"] = round(r["general_tile_it_s"] / r["general_strain_state_it_s"], 3)
        r["tile_over_isotropic"] = round(r["general_tile_it_s"] / r["isotropic_it_s"], 3)
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
