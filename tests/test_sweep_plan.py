"""Configuration -> refusal or sweeps (fibergen_amd/csrc/fg_sweep_plan.h: plan_error, plan_sweeps) against
tests/golden/sweep_plans.txt.gz: the decisions of the solver's check members, u_loop_eligible, the ladder of u_pass_front and its
copies as they stood before the header existed, recorded per configuration (profiles/README.md says how).
tests/emulate/emu_sweep_plan.cpp prints the header's answers in the table's format, its message constants, and checks the plans'
invariants.  Built and run twice: plain, and with AddressSanitizer + UBSan (a plain executable: no preloaded runtime).  CPU only."""
import glob
import gzip
import os
import re
import subprocess

import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sweep_plans.txt.gz")
CSRC = os.path.join(ROOT, "fibergen_amd", "csrc")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FRONT = ["ScFast", "ScTileAniso", "ScExact", "UStressThenDiv", "UTileDfg", "UTileAniso", "UTilePhi", "UTilePhiReuss", "UTileModuli",
         "UFastModuli", "UStressDivVoigt"]   # plan::Front, in the order of its values 0 ... 10 (None = -1)
KEY = ["mode", "mixing", "gamma_scheme", "method", "u_loop", "phase_class", "u_tile", "tiled", "mixed_bc", "entry", "factor"]
PLAN = ["complement_check", "u_loop", "front", "laminate_correction", "sum_tau", "staggered", "staggered_dfg", "viscosity", "cg", "cg_fused_wanted",
        "cg_fused_dir", "cg_dir", "slab_fast"]


def golden_rows():
    """{key tuple: "ERR <message>" or {plan field: text}}"""
    rows = {}
    for ln in gzip.open(GOLDEN, "rt"):
        if ln.startswith("#"):
            continue
        key, _, rest = ln.rstrip("\n").partition(": ")
        rows[tuple(key.split())] = rest if rest.startswith("ERR ") else dict(zip(PLAN, rest.split()))
    return rows


def golden_plan(mode=0, mixing=0, gamma_scheme=0, method=0, u_loop=2, phase_class="iso2c", u_tile=1, tiled=1, mixed_bc=0, entry="run",
                factor="-"):
    key = (mode, mixing, gamma_scheme, method, u_loop, phase_class, u_tile, tiled, mixed_bc, entry, factor)
    return golden_rows_cached()[tuple(str(k) for k in key)]


_ROWS = []


def golden_rows_cached():
    if not _ROWS:
        _ROWS.append(golden_rows())
    return _ROWS[0]


def run_driver(tmp_path, sanitized):
    flags = [f for f in emulation_build_flags() if f not in ("-shared", "-fPIC")]
    if sanitized:
        flags = SANITIZE + [f for f in flags if not f.startswith("-O")]
    exe = str(tmp_path / "emu_sweep_plan")
    subprocess.check_call(["g++"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "emulate", "emu_sweep_plan.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "OK" and not any(ln.startswith("FAIL") for ln in lines)
    return [ln for ln in lines[:-1] if not ln.startswith("MSG ")], [ln[4:] for ln in lines if ln.startswith("MSG ")]


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_sweep_plan(tmp_path, sanitized):
    table, _ = run_driver(tmp_path, sanitized)
    want = gzip.open(GOLDEN, "rt").read().splitlines()
    assert len(want) > 80000
    assert table == want, next((a, b) for a, b in zip(table, want) if a != b)


def test_golden_reaches_every_value(tmp_path):
    rows = golden_rows_cached()
    plans = [r for r in rows.values() if isinstance(r, dict)]
    assert {p["front"] for p in plans} == set(FRONT) | {"None"}
    assert {p["cg_dir"] for p in plans} == {"None", "UTileDfg", "UTileAniso", "UTilePhi", "UTileModuli", "ScFast", "ScTileAniso"}
    assert {p["staggered"] for p in plans} == {"Tile", "FusedVoigt", "Stored"}
    assert {p["viscosity"] for p in plans} == {"TileDfg", "Tile", "FusedVoigt", "Stored"}
    assert {p["cg"] for p in plans} == {"DisplacementSpace", "Scalar", "StrainSpace"}
    # every message of the header is some row's refusal -- but for the one the slab driver raises after its own preparation
    _, messages = run_driver(tmp_path, False)
    refused = {r[4:] for r in rows.values() if not isinstance(r, dict)}
    assert refused <= set(messages)
    assert set(messages) - refused == {m for m in messages if m.startswith("heat / porous on slab-decomposed solvers")}
    # both sides of each A/B switch, with differing plans
    for factor in ("fuse_stress_div=0", "cg_fused=0", "phi_sweep=0", "aniso_tile=0", "aniso_sc_tile=0", "reuss_sweep=0"):
        differ = 0
        for key, r in rows.items():
            if key[-1] == factor:
                differ += rows[key[:6] + ("1", "1", "0", key[9], "-")] != r
        assert differ > 0, factor
    # the device complement check: asked on some rows, not asked on others, recorded for the entries whose path is walked
    asked = {(k[9], p["complement_check"]) for k, p in rows.items() if isinstance(p, dict)}
    assert asked == {("iterate", "0"), ("iterate", "1"), ("run", "0"), ("run", "1"), ("pass", "-"), ("ref", "-"), ("slab", "-")}
    for col in (6, 7):   # u_tile, the tiled grid
        assert any(rows[k[:col] + ("0",) + k[col + 1:]] != r for k, r in rows.items() if k[col] == "1" and k[-1] == "-" and k[9] in ("iterate", "run"))


def test_python_layers_speak_the_header_s_words(tmp_path):
    """every refusal the Python layers raise before a solver exists is a message constant of the header, character for character"""
    from fibergen_amd import materials
    from fibergen_amd.solver import POLARIZATION_ERRORS, REUSS_ERRORS
    _, messages = run_driver(tmp_path, False)
    for key, msg in list(POLARIZATION_ERRORS.items()) + list(REUSS_ERRORS.items()):
        assert msg in messages, key
    fg_py = open(os.path.join(ROOT, "fibergen_amd", "fg.py")).read()
    assert 'raise RuntimeError("No materials specified")' in fg_py and "No materials specified" in messages
    for name in ("GENERAL_MODE_ERROR", "GENERAL_MIXING_ERROR", "GENERAL_DFG_ERROR", "GENERAL_SLAB_ERROR", "ANISO_SLAB_ERROR"):
        assert getattr(materials, name) in messages, name


def test_every_message_once_in_the_sources(tmp_path):
    _, messages = run_driver(tmp_path, False)
    text = ""
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h*"))):
        text += re.sub(r'"\s*\n\s*"', "", open(path).read())
    for msg in messages:
        assert text.count('"%s"' % msg) == 1, msg
    # the decisions live in the header: the solver asks the grid predicate in plan_input and in the slab code that passes gu_
    hits = [ln for path in glob.glob(os.path.join(CSRC, "fg_s*.hip")) for ln in open(path) if "u_tile_supported(g_)" in ln]
    assert len(hits) == 1 and "in.tiled" in hits[0], hits
