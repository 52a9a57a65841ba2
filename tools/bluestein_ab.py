"""Bluestein tile kernels against the O(n^2) sums and against the 13-smooth neighbour sizes, inside one process:
    python tools/bluestein_ab.py [--sizes 68:72,97:96,170:168,190:192,340:336] [--out profiles/bluestein_ab.jsonl]
Per pair n:m the cubes n^3 with bluestein = 0 / 1 (one solver, the option switched between timed windows, alternating twice) and
m^3 (a length the tile / sub-line kernels take).  Rates from fg_time_iterations (HIP events around K passes of the basic scheme,
stage timing off), K chosen so that a window lasts about `--window` seconds; the best of the windows of a variant is reported
beside all of them.  Two-phase sphere, Voigt mixing.  One JSON line per cube."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def make(n):
    from fibergen_amd import LSSolver
    from helpers import INCLUSION, MATRIX, lame
    x = (np.arange(n) + 0.5) / n - 0.5
    r = np.sqrt(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2)
    phi1 = np.clip((0.3 - r) * n + 0.5, 0.0, 1.0)
    s = LSSolver(n, n, n)
    s.set_num_phases(2)
    s.set_phase(0, *lame(**MATRIX), 1.0 - phi1)
    s.set_phase(1, *lame(**INCLUSION), phi1)
    s.calc_ref_material()
    return s


def rate(s, E, window):
    """it/s of one timed window of about `window` seconds (at least 2 passes), after a warm-up of the same kernels"""
    ms = s.time_iterations(E, 2)
    k = max(2, min(2000, int(window * 1e3 / max(ms / 2, 1e-3))))
    ms = s.time_iterations(E, k)
    return k / (ms * 1e-3), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="68:72,97:96,170:168,190:192,340:336")
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    lines = []
    for pair in a.sizes.split(","):
        n, m = (int(v) for v in pair.split(":"))
        s = make(n)
        rec = {"grid": [n] * 3, "paths": None, "padded": None, "it_s": {"bluestein=0": [], "bluestein=1": []}, "passes": {}}
        for flag in (0, 1, 0, 1):
            s.set_options(bluestein=flag)
            if flag:
                rec["paths"] = [s.counter("fft_path_" + c) for c in "xyz"]
                rec["padded"] = [s.counter("fft_bluestein_m_" + c) for c in "xyz"]
            r, k = rate(s, E, a.window)
            rec["it_s"]["bluestein=%d" % flag].append(round(r, 2))
            rec["passes"]["bluestein=%d" % flag] = k
        s.close()
        rec["best_it_s"] = {k: max(v) for k, v in rec["it_s"].items()}
        rec["speedup"] = round(rec["best_it_s"]["bluestein=1"] / rec["best_it_s"]["bluestein=0"], 2)
        s = make(m)
        nb = {"grid": [m] * 3, "paths": [s.counter("fft_path_" + c) for c in "xyz"], "it_s": []}
        for _ in range(2):
            r, k = rate(s, E, a.window)
            nb["it_s"].append(round(r, 2))
            nb["passes"] = k
        s.close()
        nb["best_it_s"] = max(nb["it_s"])
        # per voxel: the neighbour's rate scaled to the same number of voxels
        rec["neighbour"] = nb
        rec["voxel_rate_vs_neighbour"] = round((rec["best_it_s"]["bluestein=1"] * n ** 3) / (nb["best_it_s"] * m ** 3), 3)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
