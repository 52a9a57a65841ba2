"""Cost of gamma_scheme willot against collocated: both run the same pipeline (polarisation, six forward transforms, one
Fourier-space kernel that moves 192 B per frequency, six inverse transforms, copy + norms), so the collocated kernel is the
yardstick of k_gamma_willot.  One JSON line per size on stdout.

    python tools/willot_ab.py [--steps K] [--sizes 128,256] [--out FILE]

Per size and scheme: the Fourier kernel's time per pass, taken from the stage timing of whole passes (HIP events around the
launch inside the pass, slot "g0"; not a stand-alone launch), and the iterations per second of the basic scheme
(fg_time_iterations, stage timing off, best of three); a sphere of radius 0.3, Voigt mixing, the reference medium the
solver takes from the phases.  Elasticity times k_gamma_willot<false>
(finite lambda_0) against k_gamma_collocated; a viscosity line times k_gamma_willot<true> (lambda_0 = infinity, the Stokes
form) and the willot pass against the staggered Delta operator's pass -- the collocated scheme has no viscosity mode.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fibergen_amd import LSSolver  # noqa: E402

MATS = [(0.3846153846153846, 0.5769230769230769), (4.166666666666667, 2.7777777777777777)]
E = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


def sphere(n, R=0.3):
    x = (np.arange(n) + 0.5) / n - 0.5
    d2 = x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2
    return (d2 <= R * R).astype(np.float64)


VISC = [(1.0, 0.0), (0.05, 0.0)]


def measure(n, scheme, phi, steps, mode="elasticity"):
    s = LSSolver(n, n, n)
    mats = MATS
    if mode == "viscosity":
        mats = VISC
    s.set_options(mode=mode, gamma_scheme=scheme, maxiter=1)
    s.set_num_phases(2)
    s.set_phase(0, *mats[0], 1.0 - phi)
    s.set_phase(1, *mats[1], phi)
    s.run(E)   # one iteration of a run: the reference medium from the phases (lambda_0 = 0), as a user gets it
    s.time_iterations(E, 3)
    best = min(s.time_iterations(E, steps) for _ in range(3))
    its = steps / (best * 1e-3)
    s.enable_stage_timing(True)
    s.iterate(E, steps)
    ms, cnt = s.stage_times()
    s.close()
    return its, ms["g0"] / cnt * 1e3, sum(ms.values()) / cnt * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for n in [int(x) for x in a.sizes.split(",")]:
        phi = sphere(n)
        r = {"case": "elasticity", "method": "basic", "n": n, "steps": a.steps,
             "bytes_per_pass_MB": round(192 * n * n * (n // 2 + 1) / 1e6, 1)}
        for scheme in ("collocated", "willot"):
            its, k_us, all_us = measure(n, scheme, phi, a.steps)
            r[scheme + "_it_s"] = round(its, 1)
            r[scheme + "_fourier_kernel_us_in_pass"] = round(k_us, 1)
            r[scheme + "_all_kernels_us_in_pass"] = round(all_us, 1)
        r["fourier_kernel_time_ratio"] = round(r["willot_fourier_kernel_us_in_pass"] / r["collocated_fourier_kernel_us_in_pass"], 3)
        r["pass_time_ratio"] = round(r["collocated_it_s"] / r["willot_it_s"], 3)
        lines.append(r)
        print(json.dumps(r), flush=True)
        v = {"case": "viscosity", "method": "basic", "n": n, "steps": a.steps}
        for scheme in ("staggered", "willot"):
            its, k_us, all_us = measure(n, scheme, phi, a.steps, "viscosity")
            v[scheme + "_it_s"] = round(its, 1)
            if scheme == "willot":
                v["willot_inf_lambda_fourier_kernel_us_in_pass"] = round(k_us, 1)
            v[scheme + "_all_kernels_us_in_pass"] = round(all_us, 1)
        v["pass_time_ratio"] = round(v["staggered_it_s"] / v["willot_it_s"], 3)
        lines.append(v)
        print(json.dumps(v), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
