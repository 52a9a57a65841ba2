"""The energy of a general phase in the restatement (general_reference.GeneralLSOracle.mean_energy), on the CPU: against the
isotropic oracle on isotropic-equivalent stiffnesses, against the closed form 1/2 E^T M E, and through the energy estimator."""
import numpy as np

import general_reference as gr
from helpers import two_phase_setup
from oracle.ls_oracle import LSOracle

GRID = (8, 6, 5)


def three_iso_phases(grid, rng):
    a = rng.uniform(0.0, 1.0, grid)
    b = rng.uniform(0.0, 1.0, grid) * (1.0 - a)
    b[0, 0, :] = 0.0                 # a phase below the Voigt threshold in some voxels, and pure voxels
    a[1, :, 0] = 1.0
    b[1, :, 0] = 0.0
    return [1.0 - a - b, a, b], [(0.4, 0.6), (6.0, 8.0), (1.7, 0.2)]


def test_energy_of_isotropic_equivalent_stiffnesses_is_the_isotropic_energy():
    rng = np.random.default_rng(31)
    phis, mats = three_iso_phases(GRID, rng)
    iso = LSOracle(*GRID, mats=mats, phis=phis)
    for general in ([0, 1, 2], [1], [0, 2]):     # all phases as 6x6, and mixed with (mu, lambda) pairs
        gm = [gr.iso_stiffness(*m) if p in general else m for p, m in enumerate(mats)]
        gen = gr.GeneralLSOracle(*GRID, mats=gm, phis=phis)
        for _ in range(3):
            eps = rng.standard_normal((6,) + GRID)
            a, b = gen.mean_energy(eps), iso.mean_energy(eps)
            print("iso equivalence", general, a, b, abs(a - b) / abs(b))
            assert abs(a - b) <= 1e-14 * abs(b)
    iso.eps = gen.eps = rng.standard_normal((6,) + GRID)   # the default argument: the oracle's own field
    assert abs(gen.mean_energy() - iso.mean_energy()) <= 1e-14 * abs(iso.mean_energy())


def test_energy_of_a_homogeneous_general_phase_in_closed_form():
    """W = 1/2 E^T M E with M = [[C_nn, 2 C_ns], [2 C_sn, 4 C_ss]]: the normal-normal products once, the normal-shear products
    twice (once from the factor 2 of the law's product, or once from the doubled shear terms of the dot), the shear-shear products
    four times (both)"""
    rng = np.random.default_rng(32)
    C = gr.random_spd(rng, scale=0.7)
    E = rng.standard_normal(6)
    W = 0.0
    for i in range(3):
        for j in range(3):
            W += 0.5 * E[i] * C[i, j] * E[j]
    for i in range(3):
        for j in range(3, 6):
            W += 0.5 * 2.0 * E[i] * C[i, j] * E[j]     # S_i E_i, the law's factor 2 on E_j
            W += 0.5 * 2.0 * E[j] * C[j, i] * E[i]     # 2 S_j E_j, the dot's factor 2
    for i in range(3, 6):
        for j in range(3, 6):
            W += 0.5 * 4.0 * E[i] * C[i, j] * E[j]
    M = np.block([[C[:3, :3], 2 * C[:3, 3:]], [2 * C[3:, :3], 4 * C[3:, 3:]]])
    assert abs(W - 0.5 * E @ M @ E) <= 1e-14 * abs(W)
    phi = rng.uniform(0.0, 1.0, GRID)
    o = gr.GeneralLSOracle(*GRID, mats=[C, C], phis=[1.0 - phi, phi])
    eps = np.empty((6,) + GRID)
    eps[:] = E[:, None, None, None]
    got = o.mean_energy(eps)
    print("closed form", got, W)
    assert abs(got - W) <= 1e-13 * abs(W)
    # a field: the mean of the per-voxel closed forms
    eps = rng.standard_normal((6,) + GRID)
    want = 0.5 * np.einsum("i...,ij,j...->...", eps, M, eps).mean()
    assert abs(o.mean_energy(eps) - want) <= 1e-13 * abs(want)


def test_energy_estimator_run_matches_the_isotropic_oracle():
    mats, phis, _ = two_phase_setup(GRID)
    E = np.array([0.5, -0.25, 1.0, 0.1, 0.2, 0.3])
    for method in ("basic", "cg"):
        kw = dict(tol=1e-8, maxiter=200, error_estimator="energy")
        iso = LSOracle(*GRID, mats=mats, phis=phis, **kw)
        gen = gr.GeneralLSOracle(*GRID, mats=[gr.iso_stiffness(*m) for m in mats], phis=phis, **kw)
        fi = iso.run_load_steps(E, params=[0.0, 1.0], method=method)
        # the scan of the general oracle takes eigvalsh, the isotropic one the closed form: one mu_0 for both
        gen.mu_0, gen.update_ref = iso.mu_0, "never"
        fg = gen.run_load_steps(E, params=[0.0, 1.0], method=method)
        assert fi is False and fg is False
        assert iso.iterations == gen.iterations and iso.iterations < 200
        d = np.abs(np.array(iso.residuals) - np.array(gen.residuals)).max()
        print("energy estimator", method, iso.iterations, d)
        assert d <= 1e-12
