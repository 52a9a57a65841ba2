"""fft_images = 1 (one exchange plane in LDS per workgroup of the power-of-two y / x / z transform passes) against 2 (both
planes), alternating inside one process on the bench RVE.  One JSON line per workload on stdout.

    python tools/fft_images_ab.py [--steps K] [--rounds R] [--cases 128:voigt,256:voigt,512:voigt,256:voigt:porous] [--out FILE]

Per workload and setting: iterations per second of the basic scheme (fg_time_iterations, stage timing off, best of the rounds)
and the transform passes' times per step from the stage timing of whole steps (HIP events around each launch inside the step).
The two solvers exist side by side and are timed in turn, R rounds, so that both see the same clocks and the same box.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402
from fibergen_amd import LSSolver  # noqa: E402
from fibergen_amd.rve import bench_rve  # noqa: E402

PASSES = ["r2c_z", "c2c_y_fwd", "c2c_x_fwd", "g0", "c2c_x_inv", "c2c_y_inv", "c2r_z"]


def make(n, mixing, mode, images, phi, normals):
    s = LSSolver(n, n, n)
    bench.configure(s, phi, normals, mixing, mode)
    s.set_options(fft_images=images)
    s.calc_ref_material()
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="128:voigt,256:voigt,512:voigt,256:voigt:porous")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for case in a.cases.split(","):
        parts = case.split(":")
        n, mixing, mode = int(parts[0]), parts[1], (parts[2] if len(parts) > 2 else "elasticity")
        phi, normals, _ = bench_rve(n, mixing)
        E = np.zeros(3 if mode in ("porous", "heat") else 6)
        E[0] = 1.0
        solvers = {im: make(n, mixing, mode, im, phi, normals) for im in (2, 1)}
        ms = {2: [], 1: []}
        for s in solvers.values():
            s.time_iterations(E, 5)
        for _ in range(a.rounds):
            for im in (2, 1):
                ms[im].append(solvers[im].time_iterations(E, a.steps) / a.steps)
        r = {"n": n, "mixing": mixing, "mode": mode, "steps": a.steps, "rounds": a.rounds}
        for im in (2, 1):
            s = solvers[im]
            r["images%d_ms_per_step" % im] = [round(x, 5) for x in ms[im]]
            r["images%d_it_s" % im] = round(1e3 / min(ms[im]), 1)
            s.enable_stage_timing(True)
            s.iterate(E, a.steps)
            t, cnt = s.stage_times()
            r["images%d_pass_us" % im] = {k: round(t[k] / cnt * 1e3, 1) for k in PASSES if t.get(k, 0.0) > 0.0}
            s.close()
        r["one_plane_faster"] = max(ms[1]) < min(ms[2])
        lines.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
