"""Which transform family runs an axis (fibergen_amd/csrc/fg_fft_route.h: route_axis, route_fused_x, the resource predicates of
the one-kernel sub-line launchers) against tests/golden/fft_routes.txt.gz: the decisions of Fft3's constructor, can_fuse() and
path() as they stood before the header existed, recorded for every length 1 ... 2048 on each axis (profiles/README.md says how).
tests/emulate/emu_fft_route.cpp prints the header's answers in the table's format and checks every route against the launchers'
limits.  Built and run twice: plain, and with AddressSanitizer + UBSan (a plain executable: no preloaded runtime).  CPU only."""
import gzip
import os
import subprocess

import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fft_routes.txt.gz")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FAMILIES = ["len1", "pow2", "sub_one", "sub_lds", "sub_scratch", "tile", "bluestein", "quadratic"]
# Fft3::path(): 0 length 1, 1 power of two, 2 sub-lines p * 2^k, 3 tile kernels, 4 Bluestein, 5 O(n^2)
PATH = dict(len1=0, pow2=1, sub_one=2, sub_lds=2, sub_scratch=2, tile=3, bluestein=4, quadratic=5)


def golden_routes():
    """{(axis, length): the fields of its line}"""
    rows = [ln.split() for ln in gzip.open(GOLDEN, "rt") if not ln.startswith("#")]
    return {(int(r[0]), int(r[1])): r[2:] for r in rows}


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_fft_route(tmp_path, sanitized):
    flags = [f for f in emulation_build_flags() if f not in ("-shared", "-fPIC")]
    if sanitized:
        flags = SANITIZE + [f for f in flags if not f.startswith("-O")]
    exe = str(tmp_path / "emu_fft_route")
    subprocess.check_call(["g++"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emulate", "emu_fft_route.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(ln.startswith("FAIL") for ln in lines)
    want = gzip.open(GOLDEN, "rt").read().splitlines()
    assert len(want) == 1 + 3 * 2048
    # every entry: family, path, p, m, the plan, the Bluestein length, zodd, the fused routes and their plans
    assert lines[:-1] == want, next((a, b) for a, b in zip(lines, want) if a != b)


def test_golden_table_reaches_every_family():
    routes = golden_routes()
    seen = {a: {f[0] for (ax, _), f in routes.items() if ax == a} for a in range(3)}
    assert seen[0] | seen[1] | seen[2] == set(FAMILIES)
    assert seen[0] == seen[1] == set(FAMILIES)
    assert seen[2] == set(FAMILIES) - {"sub_scratch"}   # the z sweeps always combine in place
    # the six-way summary is a map of the family
    assert all(int(f[1]) == PATH[f[0]] for f in routes.values())
    # both sides of the thresholds, the fused-x override and its neighbour on y
    assert [routes[k][0] for k in ((0, 96), (0, 100), (1, 96), (1, 100), (2, 112), (2, 144))] == ["sub_one", "tile"] * 3
    assert routes[(0, 384)][0] == "sub_one" and routes[(1, 384)][0] == "tile"
    assert routes[(0, 1152)][0] == "tile" and routes[(0, 1216)][0] == "sub_scratch" and routes[(0, 136)][0] == "sub_lds"
