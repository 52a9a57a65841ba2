"""mixing_rule "reuss" on the host: the model's own pin (the closed form of reuss_reference.py against the literal restatement
of ReussMixedMaterialLaw::PK1 F:12663-12689 with numpy.linalg.inv), and stress_voxel / tangent_eigs of fg_stage_math.h with
kMixReuss compiled for the host against the model.

Tolerances.  The closed form and the literal 6 x 6 inversions differ by the rounding of two LU inversions of well-conditioned
matrices (cond = 3 K / 2 mu of a phase, at most ~30 in the draws): the pin holds 1e-14 of max |P| and prints the worst figure,
which reuss_reference.py quotes (CLOSED_FORM_VS_LITERAL).  The host code evaluates the same closed form as the model in the
same order (sums of phi / 2 mu and phi / 3 K in phase order, two reciprocals, hooke): 4 eps of max |P|, like the closed forms
of test_polarization_emulation.py; pure voxels are the Voigt rule's bits."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import reuss_reference as rr
from helpers import emulation_build_flags
from oracle.ls_oracle import hooke

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emulate", "emu_reuss.cpp")
EPS = np.finfo(np.float64).eps
NCASE = 4000


def make_cases():
    """seeded voxels of 2 - 4 phases, moduli over two decades: random fractions, phi exactly 0 and exactly 1 (in every
    position), phi = 1e-17 -- below the Voigt rule's 10 eps threshold, it still takes part here -- and three phases in a voxel"""
    rng = np.random.default_rng(651)
    cases = []
    for i in range(NCASE):
        nph = 2 + i % 3
        mu = rng.uniform(0.5, 5.0, 4) * 10.0 ** rng.integers(-1, 2, 4)
        lam = rng.uniform(0.1, 4.0, 4) * mu
        phi = np.zeros(4)
        phi[:nph] = rng.dirichlet(np.ones(nph))
        kind = i % 10
        if kind == 0:                                   # pure in phase i mod nph, the others exactly 0
            phi[:] = 0.0
            phi[(i // 10) % nph] = 1.0
        elif kind == 1:                                 # one phase exactly 0
            phi[(i // 10) % nph] = 0.0
            phi[:nph] /= phi[:nph].sum()
        elif kind == 2:                                 # a fraction below the Voigt threshold that still takes part
            phi[:] = 0.0
            phi[0], phi[1] = 1e-17, 1.0 - 1e-15
            mu[0], lam[0] = 1e-6 * mu[1], 1e-6 * lam[1]   # soft enough for the tiny fraction to show
        elif kind == 3 and nph >= 3:                    # three phases in one voxel, a tiny third
            phi[:] = 0.0
            phi[0], phi[1], phi[2] = 0.5, 0.5 - 1e-17, 1e-17
        elif kind == 4:                                 # phi == 1 behind a phase with phi != 0: the first phi == 1 still answers alone
            phi[:] = 0.0
            phi[0], phi[1] = 1e-17, 1.0
        F = rng.standard_normal(6)
        mu_0, lam_0 = rng.uniform(0.0, 3.0), rng.uniform(0.0, 2.0)
        if i % 7 == 0:
            mu_0 = lam_0 = 0.0
        cases.append((nph, mu, lam, phi, F, mu_0, lam_0))
    return cases


CASES = make_cases()


def model(case):
    """P - C0 : F, the tangent extremes, P alone -- through the array model on a 1 x 1 x 1 grid"""
    nph, mu, lam, phi, F, mu_0, lam_0 = case
    o = rr.ReussLSOracle(1, 1, 1, mats=[(mu[p], lam[p]) for p in range(nph)], phis=[np.full((1, 1, 1), phi[p]) for p in range(nph)])
    eps = F.reshape(6, 1, 1, 1)
    return o.calc_stress(mu_0, lam_0, eps).ravel(), o.tangent_eig_minmax(), o.pk1(eps).ravel()


def test_closed_form_against_the_literal_restatement():
    worst = 0.0
    for nph, mu, lam, phi, F, _, _ in CASES:
        mats = [(mu[p], lam[p]) for p in range(nph)]
        lit = rr.pk1_reuss_literal(F, phi[:nph], mats)
        closed = rr.pk1_reuss(F.reshape(6, 1), [np.array([phi[p]]) for p in range(nph)], mats).ravel()
        worst = max(worst, np.abs(closed - lit).max() / np.abs(lit).max())
    print("closed form against literal restatement: worst relative difference %.3e" % worst)
    assert worst <= 1e-14
    assert worst <= rr.CLOSED_FORM_VS_LITERAL   # the figure the docstring of reuss_reference.py quotes


def test_model_properties():
    """a pure voxel is its phase's law to the bit, equal phases give that phase, the rule lies below the Voigt rule, W throws"""
    from oracle.ls_oracle import pk1_voigt
    rng = np.random.default_rng(5)
    eps = rng.standard_normal((6, 4, 3, 2))
    phi = rng.uniform(0.05, 0.95, (4, 3, 2))
    phi[0, 0, 0], phi[1, 0, 0] = 0.0, 1.0
    mats = [(0.4, 0.6), (6.0, 8.0)]
    P = rr.pk1_reuss(eps, [1 - phi, phi], mats)
    V = pk1_voigt(eps, [1 - phi, phi], mats)
    assert np.array_equal(P[:, 0, 0, 0], V[:, 0, 0, 0]) and np.array_equal(P[:, 1, 0, 0], V[:, 1, 0, 0])
    same = rr.pk1_reuss(eps, [1 - phi, phi], [mats[1], mats[1]])
    assert np.abs(same - hooke(eps, *mats[1])).max() <= 8 * EPS * np.abs(same).max()
    e_r = (P * eps).sum(axis=0) + (P[3:] * eps[3:]).sum(axis=0)
    e_v = (V * eps).sum(axis=0) + (V[3:] * eps[3:]).sum(axis=0)
    assert (e_r <= e_v * (1 + 1e-14)).all() and (e_r < e_v).sum() >= 22
    o = rr.ReussLSOracle(4, 3, 2, mats=mats, phis=[1 - phi, phi])
    with pytest.raises(RuntimeError, match="Reuss MaterialLaw energy not implemented"):
        o.mean_energy()
    lo, hi = o.tangent_eig_minmax()
    assert lo == 2 * 0.4 and hi == 2 * 6.0 + 3 * 8.0   # the pure voxels bound the spectrum


_BUILD = {}


@pytest.fixture
def results(tmp_path_factory):
    """built and run once; a build that fails (before the feature: no kMixReuss) fails every test that asks for it"""
    if "res" not in _BUILD:
        out = str(tmp_path_factory.mktemp("emu") / "emu_reuss.so")
        _BUILD["rc"] = subprocess.run(["g++"] + emulation_build_flags() + ["-o", out, SRC], capture_output=True, text=True)
        _BUILD["res"] = _run(out) if _BUILD["rc"].returncode == 0 else None
    return _BUILD["res"]


def built(results):
    assert results is not None, "emu_reuss.cpp does not compile:\n" + _BUILD["rc"].stderr[-2000:]
    return results


def _run(out):
    lib = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_reuss_batch.restype = None
    lib.emu_reuss_batch.argtypes = [ctypes.c_long, dp, dp]
    data = np.ascontiguousarray(np.concatenate([np.concatenate([[nph], mu, lam, phi, F, [mu_0, lam_0]])
                                                for nph, mu, lam, phi, F, mu_0, lam_0 in CASES]))
    res = np.zeros((len(CASES), 20))
    lib.emu_reuss_batch(len(CASES), data.ctypes.data_as(dp), res.ctypes.data_as(dp))
    return res


def test_stress_voxel_reuss_against_the_model(results):
    """before the feature: kMixReuss does not exist, the emulation does not compile"""
    worst = worst0 = 0.0
    for case, r in zip(CASES, built(results)):
        tau, _, P = model(case)
        scale = np.abs(P).max() + 2 * case[5] * np.abs(case[4]).max() + 3 * case[6] * np.abs(case[4]).max()
        worst = max(worst, np.abs(r[:6] - tau).max() / scale)
        worst0 = max(worst0, np.abs(r[14:20] - P).max() / np.abs(P).max())
    print("stress_voxel reuss against the model: %.3e (tau), %.3e (P)" % (worst, worst0))
    assert worst <= 4 * EPS and worst0 <= 4 * EPS


def test_tangent_eigs_reuss_against_the_model(results):
    worst = 0.0
    for case, r in zip(CASES, built(results)):
        lo, hi = model(case)[1]
        worst = max(worst, abs(r[6] - lo) / lo, abs(r[7] - hi) / hi)
    print("tangent_eigs reuss against the model: %.3e" % worst)
    assert worst <= 2 * EPS


def test_pure_voxels_are_the_voigt_rules_bits(results):
    n = 0
    for (nph, mu, lam, phi, F, mu_0, lam_0), r in zip(CASES, built(results)):
        if (phi == 1).any() and (phi[phi != 1] == 0).all():
            assert np.array_equal(r[:6], r[8:14])
            n += 1
    assert n >= NCASE // 10


def test_a_fraction_below_the_voigt_threshold_takes_part(results):
    """phi = (1e-17, 1 - 1e-15) with phase 0 a million times softer: 1e-17 / 2 mu_0 is 1e-11 of the sum, far above rounding.  The
    compiled code agrees with the model to 4 eps (above) and is 1e-12 away from the answer without phase 0, which is what a
    10 eps threshold would give"""
    n = 0
    for (nph, mu, lam, phi, F, _, _), r in zip(CASES, built(results)):
        if phi[0] != 1e-17 or phi[1] == 1.0:
            continue
        without = rr.pk1_reuss(F.reshape(6, 1), [np.array([0.0]), np.array([phi[1]])], [(mu[0], lam[0]), (mu[1], lam[1])]).ravel()
        assert np.abs(r[14:20] - without).max() > 1e-12 * np.abs(without).max()
        n += 1
    assert n >= NCASE // 10
