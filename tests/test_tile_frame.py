"""The frame of the six tiled marching sweeps (fibergen_amd/csrc/fg_tile_frame.h: tile shape, launch plan, the place of a thread)
driven by a stand-alone program, tests/emulate/emu_tile_frame.cpp, which walks every workgroup and thread of every plan and
checks ownership (each voxel pair exactly once), offsets inside the field under both x wraps on whole grids and x-slabs,
neighbour rows, surplus workgroups and the XCD remap.  The plans it prints are compared here with the figures of the
launchers' arithmetic as it stood before the header existed -- literals, not produced by the header: the balanced plans at
256 and 2 CUs are the figures of a Python transcription of the old launchers; the plans of the fixed rule and of the general
tiles on rows of 128 pairs were worked out by hand from the old launcher text (the arithmetic stands next to them).  Built and run twice: plain, and with AddressSanitizer + UBSan (a plain executable: no preloaded runtime).  CPU only."""
import os
import subprocess

import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# (grid, tile shape, CUs, rule) -> (nty, ntz, LX, ntx, nb)
PLANS = {
    ("4x14x80", "<8,0>", 256, "balanced"): (3, 1, 4, 1, 3),      # a row shorter than a tile, kp0 < 0
    ("8x14x124", "<8,0>", 256, "balanced"): (3, 1, 4, 2, 6),     # exactly one 62-pair tile, two marches
    ("4x14x200", "<8,0>", 256, "balanced"): (3, 2, 4, 1, 6),     # two z tiles, the last one overlapping
    ("6x20x130", "<8,0>", 256, "balanced"): (4, 2, 4, 2, 16),
    ("6x14x128", "<8,1>", 256, "balanced"): (3, 1, 4, 2, 6),     # a last march of 2 planes; nb < 8: no rounding, no remap
    ("16x16x128", "<8,1>", 256, "balanced"): (3, 1, 4, 4, 16),   # remapped
    ("4x14x256", "<6,2>", 256, "balanced"): (4, 1, 4, 1, 4),
    ("5x20x256", "<6,2>", 256, "balanced"): (5, 1, 4, 2, 16),    # surplus workgroups
    ("9x14x80", "<8,0>", 256, "balanced"): (3, 1, 4, 3, 16),
    ("16x16x128", "<8,1>", 2, "balanced"): (3, 1, 8, 2, 6),      # LX > 4
    ("9x14x80", "<8,0>", 2, "balanced"): (3, 1, 9, 1, 3),
    # the strain sweep's fixed rule, by hand from the old launch_eps_tile_t: LX = 32, 16 if tiles * ceil(nx / 32) < CUs, then
    # at most nx -- nx <= 16 here, so LX = nx, ntx = 1; nty = ceil(ny / (TYR - 2)), ntz = ceil(nz/2 / (64 ZS or 62)),
    # nb = nty * ntz rounded up to a multiple of 8 from 8 on: 14/6 -> 3; 16/6 -> 3; 20/6 -> 4, 65/62 -> 2, nb 8; 20/4 -> 5
    ("4x14x80", "<8,0>", 256, "fixed"): (3, 1, 4, 1, 3),
    ("16x16x128", "<8,1>", 256, "fixed"): (3, 1, 16, 1, 3),
    ("6x20x130", "<8,0>", 256, "fixed"): (4, 2, 6, 1, 8),
    ("5x20x256", "<6,2>", 256, "fixed"): (5, 1, 5, 1, 5),
}


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_tile_frame(tmp_path, sanitized):
    flags = [f for f in emulation_build_flags() if f not in ("-shared", "-fPIC")]
    if sanitized:
        flags = SANITIZE + [f for f in flags if not f.startswith("-O")]
    exe = str(tmp_path / "emu_tile_frame")
    subprocess.check_call(["g++"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emulate", "emu_tile_frame.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(ln.startswith("FAIL") for ln in lines)
    plans = {}
    for ln in lines:
        if ln.startswith("PLAN "):
            _, grid, shape, cus, rest = ln.split(" ", 4)
            rule, figures = rest.split(": ")
            plans[(grid, shape, int(cus[4:]), rule)] = tuple(int(v) for v in figures.split())
    # nine grids x three CU counts (the three rows of 128 pairs also with the general tiles) + the fixed rule
    assert len(plans) == 9 * 3 + 2 * 3 + 9
    for key, want in PLANS.items():
        assert plans[key] == want, key
    # callers without a <6, 2> form: rows of 128 pairs take the general tiles.  By hand: nty = ceil(14 / 6) = 3,
    # ntz = ceil(128 / 62) = 3, nx = 4 -> LX = 4, ntx = 1, nb = 9 -> 16
    assert plans[("4x14x256", "<8,0>", 256, "balanced")] == (3, 3, 4, 1, 16)
