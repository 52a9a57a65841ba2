"""Parity at BASELINE.json's full sizes (256^3 default config, 512^3 roofline config) through size-independent
properties: the oracle cannot run there in seconds, so the fast pipeline is checked against the exact-order
pipeline of the same library (itself bit-exact against the oracle at small sizes, tests/test_gpu_parity.py),
and against analytic facts: mean strain = prescribed strain after every pass, homogeneous medium, the
staggered eps-G0-div identity (F:24129-24151), linearity of the pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lattice_phi(n, R=0.31):
    """periodic lattice of 4^3 spheres, voxel-centre sampling with a smooth rim (values in [0, 1])"""
    c = ((np.arange(n) + 0.5) / n * 4) % 1.0 - 0.5
    d = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    return np.clip((R - d) * n / 4 + 0.5, 0.0, 1.0)


def _solver(n, **kw):
    from fibergen_amd import LSSolver
    from helpers import INCLUSION, MATRIX, lame
    phi = _lattice_phi(n)
    s = LSSolver(n, n, n)
    s.set_num_phases(2)
    m0, m1 = lame(**MATRIX), lame(**INCLUSION)
    s.set_phase(0, m0[0], m0[1], 1.0 - phi)
    s.set_phase(1, m1[0], m1[1], phi)
    s.set_options(**kw)
    return s


@pytest.mark.parametrize("n", [256, 512])
def test_fast_pipeline_equals_exact_pipeline_at_full_size(n):
    """k iterations of the default pipeline (tiled sweep, fused x pass) against the exact-order displacement loop and
    the strain-state pipeline: same residual norms to rounding, same mean stress, mean strain = E."""
    E = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.5])
    res = {}
    for name, opts in (("fast", {}), ("exact", dict(u_loop=1)), ("plain", dict(u_loop=0, fuse_x=0, fuse_stress_div=0))):
        s = _solver(n, **opts)
        s.calc_ref_material()
        if name == "plain":
            # the displacement loop's norm sweep belongs to the strain of the previous pass: compare like with like
            s.iterate(E, 5)
            ss = s.get_field("sumsq")
            s.iterate(E, 1)
        else:
            s.iterate(E, 6)
            ss = s.get_field("sumsq")
        res[name] = (ss, s.mean_stress(), s.mean_strain(), s.ref_material)
        s.close()
    for other in ("exact", "plain"):
        assert res["fast"][3] == res[other][3]
        np.testing.assert_allclose(res["fast"][0], res[other][0], rtol=1e-11)
        np.testing.assert_allclose(res["fast"][1], res[other][1], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(res["fast"][2], E, atol=1e-12)
    assert np.array_equal(res["exact"][0], res["plain"][0]) or np.allclose(res["exact"][0], res["plain"][0], rtol=1e-13)


@pytest.mark.parametrize("n", [256, 192, 320])   # 192 = 3*64, 320 = 5*64: the single-kernel p*2^k FFT passes at size
def test_homogeneous_medium_and_identity_at_256(n):
    """(i) one phase everywhere: eps == E after one pass for any start; (ii) staggered epsG0div identity on a random
    displacement field: eps(G0(div(C0 : eps(u)))) == eps(u)  (F:24129-24151) at 256^3 (and at two p*2^k sizes)."""
    from fibergen_amd import LSSolver
    s = LSSolver(n, n, n)
    s.set_num_phases(1)
    s.set_phase(0, 0.7, 1.1, np.ones((n, n, n)))
    s.set_options(mu_0=0.7, lambda_0=1.1, update_ref="never")
    E = np.array([0.3, -0.2, 0.1, 0.05, 0.0, 0.4])
    s.iterate(E, 3)
    ss = s.get_field("sumsq")
    np.testing.assert_allclose(ss / n ** 3, E * E, rtol=1e-12, atol=1e-26)
    np.testing.assert_allclose(s.mean_strain(), E, atol=1e-14)
    # identity: u random -> eps0 = grad_s u ; tau = C0 : eps0 ; f = div tau ; u' = G0 f (alpha = 1) ; eps1 = grad_s u'
    rng = np.random.default_rng(0)
    u = rng.standard_normal((3, n, n, n))
    s.set_field("u", u)
    s.run_stage("eps", np.zeros(6))
    e0 = s.get_field("epsilon")
    s.run_stage("stress_const", None)
    s.run_stage("div", None)
    s.run_stage("fft_forward", None)
    s.run_stage("g0", np.array([1.0, 0, 0, 0, 0, 0]))
    s.run_stage("fft_inverse", None)
    s.run_stage("eps", np.zeros(6))
    e1 = s.get_field("epsilon")
    assert np.abs(e1 - e0).max() <= 1.5e-8 * max(1.0, np.abs(e0).max())   # the reference's tolerance sqrt(eps)
    assert np.abs(e1 - e0).max() <= 1e-9 * np.abs(e0).max()
    s.close()


def test_pass_is_affine_at_256():
    """One pass is affine in the strain: B(a e1 + (1-a) e2) == a B(e1) + (1-a) B(e2)."""
    n = 256
    s = _solver(n, u_loop=0, mu_0=0.9, lambda_0=0.2, update_ref="never")
    rng = np.random.default_rng(1)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    e1 = rng.standard_normal((6, n, n, n))
    e2 = rng.standard_normal((6, n, n, n))
    out = []
    for e in (e1, e2, 0.25 * e1 + 0.75 * e2):
        s.set_field("epsilon", e)
        s.run_stage("iteration", E)
        out.append(s.get_field("epsilon"))
    s.close()
    ref = 0.25 * out[0] + 0.75 * out[1]
    assert np.abs(out[2] - ref).max() <= 1e-11 * np.abs(ref).max()


def test_hbm_stream_helper():
    """fg_hbm_stream (the measured roofline bench.py reports): plausible copy / triad rates on an MI355X."""
    import ctypes
    from fibergen_amd import _lib
    lib = _lib.load()
    c, t = ctypes.c_double(0.0), ctypes.c_double(0.0)
    assert lib.fg_hbm_stream(0, 512, 2, ctypes.byref(c), ctypes.byref(t)) == 0
    assert 1000.0 < c.value < 8000.0 and 1000.0 < t.value < 8000.0
    assert lib.fg_hbm_stream(0, 0, 1, ctypes.byref(c), ctypes.byref(t)) != 0   # bad size: error code, no exception


def test_runs_are_reproducible_bit_for_bit():
    """The reductions of the loop are fixed-order (DPP folds inside a wave, fixed fold over the workgroups, no float atomics) and
    the laminate correction has one writer per voxel: two runs of the same problem on fresh solvers give the same residual
    history, strain field and mean stress bit for bit -- basic scheme and CG, Voigt and laminate mixing."""
    from helpers import make_gpu_solver
    E = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.5])
    for mixing, method in (("voigt", "basic"), ("laminate", "basic"), ("laminate", "cg")):
        out = []
        for _ in range(2):
            s = make_gpu_solver((64, 48, 128), mixing=mixing, tol=1e-7, method=method)
            assert s.run(E) is False
            out.append((np.array(s.residuals), s.get_field("epsilon"), s.mean_stress().copy()))
            s.close()
        assert np.array_equal(out[0][0], out[1][0]), (mixing, method)
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2]), (mixing, method)


def test_bench_line_of_the_default_command_on_a_small_grid():
    """`python bench.py --full` (the driver's N = 1 command with every leg) on 64^3 with short budgets: the one JSON line keeps the
    contract's keys --
    metric / value / unit / steps / warmup / ms_per_step, `roofline` with the traffic measured in the run by the two counter
    passes, `cpu_baseline` from the C loop nests on this host, the per-kernel table, one `also` leg."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--size", "64", "--steps", "6", "--warmup", "2", "--repeats",
           "3", "--sustain-s", "0.3", "--cpu-budget", "3", "--also", "32:laminate"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1   # ONE line
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["steps"] == 6 and line["warmup"] == 2 and line["unit"] == "it/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["vs_baseline"] is None and line["data"] == "synthetic"
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-3 and "workload" in line["config"]
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["traffic"] is None or rf["traffic"] > 0.5 * rf["alg_bytes_per_launch"]
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "it/s" and "sample" in cb
    assert line["also"]["32^3 laminate"]["it_s"] > 0 and len(line["kernels"]) >= 4
    # what the line measures, said in the line: one GPU has no scaling mode; `value` is fg_iterate, the loop under
    # the stop rule sits beside it -- top level and inside `config`, which the driver's record keeps whole; a Green-operator
    # figure on a grid whose spectrum (3 x 16 B x 64 x 64 x 33 = 6.5 MB) lives in the Infinity Cache is flagged as such
    assert line["scaling"] is None and "fg_iterate" in line["metric"] and "fg_iterate" in line["config"]["timed_call"]
    assert line["run_load_case_it_s"] > 0 and line["config"]["run_load_case_it_s"] == line["run_load_case_it_s"]
    assert line["gamma0_apply_standalone"]["cache_assisted"] is True
    pc = line["pcie_inclusive"]
    assert pc["upload_ms"] > 0 and pc["download_ms"] > 0 and pc["it_s_inclusive"] > 0


def test_plain_bench_run_and_its_outputs(tmp_path):
    """`python bench.py` without --full: the headline only -- ONE region of exactly --steps timed steps, none of the --full
    legs -- and --dump-outputs writes what the timed path computed: the strain and stress fields (64^3 = 2^18 voxels: all of
    them) and their means, float64, consistent with each other."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--size", "64", "--steps", "7", "--warmup", "2",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert key in line, key
    assert line["steps"] == 7 and line["warmup"] == 2 and line["repeats"] == 1 and line["unit"] == "it/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-3
    assert "fg_iterate" in line["metric"] and line["config"]["grid"] == [64, 64, 64]
    for key in ("kernels", "roofline", "cpu_baseline", "also", "sustained_it_s", "cg_method", "slab_forced"):
        assert key not in line, key
    d = {name: np.load(tmp_path / "out" / (name + ".npy")) for name in ("epsilon", "sigma", "mean_stress", "mean_strain")}
    assert d["epsilon"].shape == d["sigma"].shape == (6, 64 ** 3) and d["mean_stress"].shape == d["mean_strain"].shape == (6,)
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in d.values())
    assert np.abs(d["epsilon"].mean(axis=1) - d["mean_strain"]).max() < 1e-10
    assert np.abs(d["sigma"].mean(axis=1) - d["mean_stress"]).max() < 1e-9 * np.abs(d["mean_stress"]).max()
    assert np.abs(d["epsilon"][0].mean() - 1.0) < 1e-10   # the prescribed mean strain E = e_xx


def test_driver_smoke_entry(capsys):
    """__graft_entry__.smoke(): the invocation the driver runs before the bench."""
    import __graft_entry__
    __graft_entry__.smoke()
    out = capsys.readouterr().out
    assert "smoke voigt" in out and "smoke laminate" in out
