"""mixing_rule "reuss" restated in NumPy on the oracles (test infrastructure only).

F = src/fibergen.cpp of the reference.  ReussMixedMaterialLaw F:12651-12724, per voxel (PK1 F:12663-12689):
  a phase with phi == 0 is skipped; the first phase with phi == 1 (exact) answers alone with its own law; otherwise
  P = alpha (sum_p phi_p C_p^-1)^-1 F over all phases with phi != 0 -- no 10 eps threshold, that is the Voigt rule's.
W throws ("Reuss MaterialLaw energy not implemented", F:12657-12661).

For isotropic phases C_p = dPK1 of the identity rows = [[2 mu I + lambda 11^T, 0], [0, 2 mu I]] (the stored shear strains are
tensor components, hooke: S_i = 2 mu E_i there); such matrices share their eigenspaces, so the inverse sum is taken on the two
eigenvalues: 2 mu_bar = 1 / sum(phi_p / 2 mu_p), 3 K_bar = 1 / sum(phi_p / (2 mu_p + 3 lambda_p)), lambda_bar = (3 K_bar -
2 mu_bar) / 3.  The scalar laws (heat, porous; viscosity with the halved constant) have the single constant: mu_bar =
1 / sum(phi_p / mu_p).

  reuss_moduli          the closed form per voxel: (2 mu_bar, 3 K_bar, pure-phase index or -1)
  pk1_reuss             PK1 with it (a pure voxel: hooke of its phase, the bits of the Voigt rule there)
  pk1_reuss_literal     the literal restatement of F:12663-12689: numpy.linalg.inv per phase, sum, inverse again
  ReussLSOracle / ReussScalarOracle / ReussViscosityOracle

Closed form against the literal restatement (test_reuss_emulation.py, 4000 seeded voxels of 2-4 phases, moduli over two decades
and a phase a million times softer, fractions down to 1e-17): worst relative difference 1.33e-15 of max |P|, kept here rounded up
to 1.4e-15.  The reference inverts with gesv, so the closed form equals it to rounding, not to the bit; the stage tests take
10 x that figure, 1.4e-14, where they cannot hold the 1e-14 of the Voigt stage tests."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.ls_oracle import LSOracle, hooke
from oracle.scalar_oracle import ScalarOracle
from oracle.viscosity_oracle import ViscosityOracle

CLOSED_FORM_VS_LITERAL = 1.4e-15   # measured 1.33e-15, see above
STAGE_TOL = 10 * CLOSED_FORM_VS_LITERAL


def reuss_moduli(phis, mats):
    """(2 mu_bar, 3 K_bar, pure) per voxel, the phases in their order (F:12667-12673): phi == 0 is skipped, the first phi == 1
    answers alone (pure = its index, else -1), every other fraction adds phi / eigenvalue"""
    shape = np.shape(phis[0])
    sa, sk = np.zeros(shape), np.zeros(shape)
    pure = np.full(shape, -1)
    for p, (phi, (mu, lam)) in enumerate(zip(phis, mats)):
        phi = np.asarray(phi, dtype=np.float64)
        one = (phi == 1) & (pure < 0)
        pure = np.where(one, p, pure)
        live = (phi != 0) & (pure < 0)
        sa = np.where(live, sa + phi / (2 * mu), sa)
        sk = np.where(live, sk + phi / (2 * mu + 3 * lam), sk)
    with np.errstate(divide="ignore"):
        two_mu, three_k = 1 / sa, 1 / sk
    for p, (mu, lam) in enumerate(mats):
        two_mu = np.where(pure == p, 2 * mu, two_mu)
        three_k = np.where(pure == p, 2 * mu + 3 * lam, three_k)
    return two_mu, three_k, pure


def pk1_reuss(eps, phis, mats, alpha=1.0):
    two_mu, three_k, pure = reuss_moduli(phis, mats)
    P = hooke(eps, 0.5 * two_mu, (three_k - two_mu) / 3, alpha)
    for p, (mu, lam) in enumerate(mats):   # the phase's own law: the bits of a pure voxel under the Voigt rule
        P = np.where(pure == p, hooke(eps, mu, lam, alpha), P)
    return P


def iso_matrix(mu, lam):
    """dPK1 of LinearIsotropicMaterialLaw on the identity rows (F:11398-11425): row m = hooke(e_m)"""
    return np.stack([hooke(np.eye(6)[m], mu, lam, 1.0) for m in range(6)])


def pk1_reuss_literal(F, phi, mats, alpha=1.0):
    """one voxel, F:12663-12689 line by line"""
    S = np.zeros((6, 6))
    for f, (mu, lam) in zip(phi, mats):
        if f == 0:
            continue
        if f == 1:
            return hooke(F, mu, lam, alpha)
        S += f * np.linalg.inv(iso_matrix(mu, lam))
    C = np.linalg.inv(S)
    P = np.zeros(6)
    for k in range(6):
        for j in range(6):
            P[k] += alpha * C[k, j] * F[j]
    return P


def scalar_reuss_constant(phis, mus):
    """mu_bar per voxel of the scalar laws"""
    shape = np.shape(phis[0])
    s = np.zeros(shape)
    pure = np.full(shape, -1)
    for p, (phi, mu) in enumerate(zip(phis, mus)):
        phi = np.asarray(phi, dtype=np.float64)
        one = (phi == 1) & (pure < 0)
        pure = np.where(one, p, pure)
        live = (phi != 0) & (pure < 0)
        s = np.where(live, s + phi / mu, s)
    with np.errstate(divide="ignore"):
        mu_bar = 1 / s
    for p, mu in enumerate(mus):
        mu_bar = np.where(pure == p, mu, mu_bar)
    return mu_bar


@dataclass
class ReussLSOracle(LSOracle):
    """LSOracle with mixing_rule reuss (isotropic phases)"""

    mixing_rule: str = "reuss"

    def pk1(self, eps, alpha=1.0):
        return pk1_reuss(eps, self.phis, self.mats, alpha)

    def mean_energy(self, eps=None):
        raise RuntimeError("Reuss MaterialLaw energy not implemented")

    def tangent_eig_minmax(self):
        two_mu, three_k, _ = reuss_moduli(self.phis, self.mats)
        return float(min(two_mu.min(), three_k.min())), float(max(two_mu.max(), three_k.max()))


class ReussScalarOracle(ScalarOracle):
    """ScalarOracle (heat / porous) with mixing_rule reuss"""

    def pk1(self, g, alpha=1.0):
        return g * (alpha * scalar_reuss_constant(self.phis, self.mus))

    def mean_energy(self, g=None):
        raise RuntimeError("Reuss MaterialLaw energy not implemented")

    def calc_ref_material(self):
        mu_bar = scalar_reuss_constant(self.phis, self.mus)
        lo, hi = float(mu_bar.min()), float(mu_bar.max())
        if lo < 0:
            lo = 0.0
        self.mu_0 = 0.5 * (lo + hi) * (0.5 * self.ref_scale)


class ReussViscosityOracle(ViscosityOracle):
    """ViscosityOracle with mixing_rule reuss: the scalar law on six components with the halved constant (F:15237)"""

    def pk1(self, eps, alpha=1.0):
        return eps * (alpha * scalar_reuss_constant(self.phis, [0.5 * mu for mu, _ in self.mats]))

    def mean_energy(self, eps=None):
        raise RuntimeError("Reuss MaterialLaw energy not implemented")

    def tangent_eig_minmax(self):
        t = scalar_reuss_constant(self.phis, [0.5 * mu for mu, _ in self.mats])
        return float(t.min()), float(t.max())
