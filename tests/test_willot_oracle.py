"""CPU pins of the willot restatement (tests/willot_reference.py) and of the arithmetic the kernel k_gamma_willot runs
(fibergen_amd/csrc/fg_willot_math.h, built for the host)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import emulation_build_flags
from oracle.ls_oracle import isotropic_laminate_ceff, material_from_pair
from willot_reference import (VI, VJ, WillotLSOracle, willot_apply_hat, willot_axis_tables, willot_gamma_hat, willot_r)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQRT_EPS = math.sqrt(np.finfo(np.float64).eps)   # check_tol's default bar, 1.49e-8
MU_0 = 0.9
IDENTITY_GRIDS = [((2, 1, 1), (1, 1, 1)),              # F:27261
                  ((41, 33, 11), (1, 1, 1)),           # F:27266
                  ((41, 33, 11), (41, 33, 11)),        # F:27271
                  ((41, 33, 11), (0.7, 1.3, 2.1)),
                  ((8, 6, 4), (1, 1, 1)),              # Nyquist index on every axis (q = -pi)
                  ((7, 6, 5), (1, 1, 1))]


@pytest.mark.parametrize("lam", [0.0, 1.7])
@pytest.mark.parametrize("grid,dims", IDENTITY_GRIDS)
def test_willot_epsG0div_identity(grid, dims, lam):
    """'WillotR epsG0div identity'  F:24107-24126: eta = Gamma(tau) with alpha = 1, E = 0 is compatible, and
    Gamma(C0 : eta) gives it back; bar: the reference's norm_2(max |.|) <= sqrt(eps) on N(0, 1) input."""
    o = WillotLSOracle(*grid, *dims)
    rng = np.random.default_rng(3)
    tau = rng.standard_normal((6,) + grid)
    Z = np.zeros(6)
    org = o.gamma_willot(Z, MU_0, lam, tau, 1.0)
    back = o.gamma_willot(Z, MU_0, lam, o.calc_stress_const(MU_0, lam, org), 1.0)
    assert np.isfinite(org).all() and np.isfinite(back).all()
    diff = np.abs(back - org).reshape(6, -1).max(axis=1)
    assert np.linalg.norm(diff) <= SQRT_EPS
    assert np.abs(org.reshape(6, -1).mean(axis=1)).max() < 1e-12   # zero frequency = E = 0
    if max(grid) > 2:
        assert np.abs(org).max() > 1e-3                                # (not the trivial fixed point)


def _layers(shape, fr):
    edges = np.round(np.cumsum([0.0] + fr) * shape[0]).astype(int)
    phis = []
    for a, b in zip(edges[:-1], edges[1:]):
        p = np.zeros(shape)
        p[a:b] = 1.0
        phis.append(p)
    return phis


@pytest.mark.parametrize("shape,fr", [((11, 1, 1), [4 / 11, 7 / 11]), ((12, 1, 1), [5 / 12, 7 / 12]),
                                      ((10, 4, 6), [0.3, 0.7])])
def test_willot_scheme_reproduces_the_closed_form_laminate(shape, fr):
    """x-layered two-phase medium: at k_y = k_z = 0 the operator reduces to the exact one-dimensional one, so the scheme
    converges to calc_isotropic_laminate F:26405-26446 like the collocated and staggered ones
    (test_collocated_scheme_same_laminate_as_staggered, same bar)."""
    ms = [material_from_pair(E=100.0, nu=0.4), material_from_pair(E=25.0, nu=0.25)]
    o = WillotLSOracle(*shape, mats=[(m["mu"], m["lambda"]) for m in ms], phis=_layers(shape, fr), tol=1e-12)
    C = o.calc_effective_properties()
    Cl = isotropic_laminate_ceff([(f, m["mu"], m["lambda"]) for f, m in zip(fr, ms)])
    assert np.abs(C - Cl).max() / np.abs(Cl).max() < 1e-8


@pytest.mark.parametrize("grid,dims", [((8, 6, 4), (1, 1, 1)), ((7, 6, 5), (0.7, 1.3, 2.1)), ((16, 16, 16), (1, 1, 1))])
def test_willot_two_algebraic_forms_agree(grid, dims):
    """lambda_0 = 1.7: the reference's active form (in mu_0 / lambda_0, F:19233-19240) and the multiplied-through one
    (F:19243-19250) the library uses for finite lambda_0 agree to 1e-13, entry by entry (|entries| = O(1 / mu_0))."""
    r = willot_r(grid, dims)
    a = willot_gamma_hat(r, MU_0, 1.7, "active")
    b = willot_gamma_hat(r, MU_0, 1.7, "multiplied")
    nz = np.ones(r[0].shape, dtype=bool)
    nz[0, 0, 0] = False
    assert max(np.abs(a[k] - b[k])[nz].max() for k in a) <= 1e-13
    # and lambda_0 = 0 is finite in the multiplied-through form only
    with np.errstate(divide="ignore", invalid="ignore"):
        assert not np.isfinite(willot_gamma_hat(r, MU_0, 0.0, "active")[0, 0][nz]).any()
    assert all(np.isfinite(v[nz]).all() for v in willot_gamma_hat(r, MU_0, 0.0).values())


@pytest.mark.parametrize("lam", [0.0, 1.7, math.inf])
@pytest.mark.parametrize("grid,dims", [((8, 6, 4), (1, 1, 1)), ((7, 6, 5), (0.7, 1.3, 2.1))])
def test_willot_gamma_hat_is_hermitian_and_projects(grid, dims, lam):
    """Gamma_hat straight from the formula is Hermitian (the reference mirrors the upper triangle, F:19255); it annihilates
    equilibrated fields (tau . conj(r) = 0), and for finite lambda_0 gives compatible fields sym(r (x) a) back from
    C0 : sym(r (x) a)."""
    r = willot_r(grid, dims)
    nz = np.ones(r[0].shape, dtype=bool)
    nz[0, 0, 0] = False
    pairs = [(i, j) for i in range(6) for j in range(6)]
    G = willot_gamma_hat(r, MU_0, lam, pairs=pairs)
    scale = 1 / MU_0
    for i, j in pairs:
        assert np.abs(G[i, j] - np.conj(G[j, i]))[nz].max() <= 1e-13 * scale
    up = willot_gamma_hat(r, MU_0, lam)
    rng = np.random.default_rng(7)
    cplx = lambda: rng.standard_normal((3,) + r[0].shape) + 1j * rng.standard_normal((3,) + r[0].shape)
    rr = np.array(r)
    sym = lambda a, b: np.array([0.5 * (a[VI[v]] * b[VJ[v]] + a[VJ[v]] * b[VI[v]]) for v in range(6)])
    # equilibrated: tau = sym(v1 (x) v2) with v . conj(r) = 0
    v = [x - (x * np.conj(rr)).sum(axis=0) * rr for x in (cplx(), cplx())]
    out = willot_apply_hat(up, sym(v[0], v[1]), 1.0, 0.0)
    assert np.abs(out[:, nz]).max() <= 1e-13 * scale
    if not math.isinf(lam):
        e = sym(rr, cplx())
        tr = e[0] + e[1] + e[2]
        s = 2 * MU_0 * e
        s[:3] += lam * tr
        back = willot_apply_hat(up, s, 1.0, 0.0)
        assert np.abs(back - e)[:, nz].max() <= 1e-13 * np.abs(e).max()


def test_willot_nyquist_tables():
    """an even axis: the Nyquist index maps to q = -pi, tan(q / 2) is huge and 1 + e^{iq} tiny, their product finite"""
    (q, tn, e, w), = willot_axis_tables((8,), (1.0,))
    assert q[4] == -math.pi and abs(tn[4]) > 1e15 and e[4].real == 0.0 and 0 < abs(e[4].imag) < 1e-15
    assert abs(abs(0.25 * tn[4] * e[4] / w) - 4.0) < 1e-12   # |i tan(q/2) (1 + e^{iq}) / (4 w)| -> 2 / (4 w) ... = 4 for w = 1/8


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_willot.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, os.path.join(ROOT, "tests", "emulate", "emu_willot.cpp")])
    lib = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_willot_apply.restype = None
    lib.emu_willot_apply.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 7 + [dp, dp]
    return lib


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.7, math.inf])
@pytest.mark.parametrize("grid,dims", [((2, 1, 1), (1, 1, 1)), ((8, 6, 4), (1, 1, 1)), ((7, 6, 5), (1, 1, 1)),
                                       ((12, 10, 6), (2.0, 1.0, 0.5)), ((41, 33, 11), (0.7, 1.3, 2.1))])
def test_kernel_arithmetic_matches_restatement(emu, grid, dims, lam):
    """willot_point / willot_axis_table of fg_willot_math.h (what k_gamma_willot runs per frequency, host tables included)
    against the restatement on a random spectrum.  The two differ in association only (tables with 1 / w folded in, one
    reciprocal of the denominator, r_i r_j conj(r_k r_l) from shared products): bar 1e-13 relative to the largest value,
    > 40x the 2.3e-15 measured."""
    rng = np.random.default_rng(0)
    nzc = grid[2] // 2 + 1
    shp = (6,) + grid[:2] + (nzc,)
    th = rng.standard_normal(shp) + 1j * rng.standard_normal(shp)
    E = rng.standard_normal(6)
    mu = -0.7 if math.isinf(lam) else MU_0   # (the Delta operator hands over a negative mu)
    ref = willot_apply_hat(willot_gamma_hat(willot_r(grid, dims), mu, lam), th, -1.0, 0.3)
    ref[:, 0, 0, 0] = E
    buf = np.ascontiguousarray(th).copy()
    dp = ctypes.POINTER(ctypes.c_double)
    emu.emu_willot_apply(*grid, *map(float, dims), mu, lam, -1.0, 0.3, E.ctypes.data_as(dp),
                         buf.view(np.float64).ctypes.data_as(dp))
    assert np.isfinite(buf).all()
    assert np.abs(buf - ref).max() <= 1e-13 * np.abs(ref).max()
