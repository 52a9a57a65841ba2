"""law="general" (a constant 6x6 stiffness per phase) restated in NumPy on LSOracle (test infrastructure only).

F = src/fibergen.cpp of the reference.  A material is either the isotropic pair (mu, lam) or a 6x6 array C in the
convention of LinearGeneralMaterialLaw F:11233-11349: Voigt shear entries (C44 = mu for an isotropic body), tensor shear
strains, the factor 2 in the product.

  general6            PK1 F:11254-11272 in its operation order
  pk1_voigt_general   VoigtMixedMaterialLaw::PK1 F:12752-12761 over mixed isotropic / general phases
  energy_general      W F:11247-11252; energy_voigt_general: VoigtMixedMaterialLaw::W F:12739-12750 over mixed phases
  scan_matrix         the matrix eig() hands dsyev (F:12518-12522): dPK1 of the identity rows, read through its upper triangle
  GeneralLSOracle     LSOracle with these two; the scan takes numpy.linalg.eigvalsh per voxel
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle.ls_oracle import VOIGT_THRESHOLD, LSOracle, energy_hooke, hooke


def is_general(mat):
    return np.ndim(mat) == 2


def iso_stiffness(mu, lam):
    """the isotropic body as a general stiffness: normal block 2 mu I + lam 11^T, shear entries mu"""
    C = np.zeros((6, 6))
    C[:3, :3] = lam
    for i in range(3):
        C[i, i] = 2 * mu + lam
        C[3 + i, 3 + i] = mu
    return C


def general6(E, C, alpha=1.0):
    """LinearGeneralMaterialLaw::PK1  F:11254-11272; E is [6, ...], alpha may be an array (phase fraction)"""
    S = np.empty_like(E)
    for i in range(6):
        S[i] = alpha * (E[0] * C[i, 0] + E[1] * C[i, 1] + E[2] * C[i, 2]
                        + 2.0 * (E[3] * C[i, 3] + E[4] * C[i, 4] + E[5] * C[i, 5]))
    return S


def pk1_voigt_general(eps, phis, mats, alpha=1.0):
    """oracle.ls_oracle.pk1_voigt with a per-phase law"""
    P = np.zeros_like(eps)
    first = np.ones(eps.shape[1:], dtype=bool)
    for phi, mat in zip(phis, mats):
        use = phi > VOIGT_THRESHOLD
        S = general6(eps, np.asarray(mat), phi * alpha) if is_general(mat) else hooke(eps, mat[0], mat[1], phi * alpha)
        P = np.where(use & first, S, np.where(use, P + S, P))
        first = first & ~use
    return P


def scan_matrix(C):
    """Row m of the matrix dPK1 fills from the identity rows is C(:, m) f_m with f = (1, 1, 1, 2, 2, 2) (F:9068-9075,
    F:11274-11298); dsyev reads its upper triangle: [[C_nn, C_ns], [C_ns^T, 2 C_ss]]"""
    C = np.asarray(C, dtype=np.float64)
    f = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    M = C.T * f[:, None]          # M[m, i] = C[i, m] f_m
    A = np.triu(M)
    return A + np.triu(M, 1).T


def voigt_tangent_matrices(phis, mats):
    """[nx, ny, nz, 6, 6]: sum_p phi_p scan_matrix(C_p) over the phases above the Voigt threshold (F:12763-12771)"""
    A = np.zeros(np.shape(phis[0]) + (6, 6))
    for phi, mat in zip(phis, mats):
        w = np.where(phi > VOIGT_THRESHOLD, phi, 0.0)
        Cp = np.asarray(mat) if is_general(mat) else iso_stiffness(*mat)
        A = A + w[..., None, None] * scan_matrix(Cp)
    return A


def energy_general(E, C):
    """LinearGeneralMaterialLaw::W  F:11247-11252: 0.5 * S.dot(E) with S = PK1(E, 1) and SymTensor3x3::dot F:9414-9417 (shear
    products doubled)"""
    S = general6(E, C, 1.0)
    return 0.5 * (S[0] * E[0] + S[1] * E[1] + S[2] * E[2] + 2 * (S[3] * E[3] + S[4] * E[4] + S[5] * E[5]))


def energy_voigt_general(eps, phis, mats):
    """oracle.ls_oracle.energy_voigt with a per-phase law (VoigtMixedMaterialLaw::W F:12739-12750: W += phi_p * W_p from zero,
    phases with phi <= 10 eps skipped)"""
    W = np.zeros(eps.shape[1:])
    for phi, mat in zip(phis, mats):
        use = phi > VOIGT_THRESHOLD
        Wp = energy_general(eps, np.asarray(mat)) if is_general(mat) else energy_hooke(eps, mat[0], mat[1])
        W = np.where(use, W + phi * Wp, W)
    return W


@dataclass
class GeneralLSOracle(LSOracle):
    """LSOracle whose materials may be 6x6 stiffnesses (Voigt mixing)"""

    def pk1(self, eps, alpha=1.0):
        if self.mixing_rule != "voigt":
            raise RuntimeError("general phases support Voigt mixing only")
        return pk1_voigt_general(eps, self.phis, self.mats, alpha)

    def mean_energy(self, eps=None):
        """meanW  F:12239-12262 over the Voigt rule's W with a per-phase law"""
        if self.mixing_rule != "voigt":
            raise RuntimeError("general phases support Voigt mixing only")
        eps = self.eps if eps is None else eps
        return float(energy_voigt_general(eps, self.phis, self.mats).sum()) / self.N

    def tangent_eig_minmax(self):
        if not any(is_general(m) for m in self.mats):
            return super().tangent_eig_minmax()
        A = voigt_tangent_matrices(self.phis, self.mats).reshape(-1, 6, 6)
        A = np.unique(A, axis=0) if A.shape[0] > 4096 else A
        w = np.linalg.eigvalsh(A)
        return float(w.min()), float(w.max())


def random_spd(rng, coupling=True, scale=1.0):
    """a random symmetric positive definite stiffness; coupling=False zeroes the normal-shear block"""
    B = rng.standard_normal((6, 6))
    C = B @ B.T + 6 * np.eye(6)
    if not coupling:
        C[:3, 3:] = 0.0
        C[3:, :3] = 0.0
    C = 0.5 * (C + C.T)
    return scale * C


def distinct_stiffness(scale=1.0):
    """an SPD stiffness whose 21 constants are all distinct (diagonally dominant)"""
    C = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i + 1, 6):
            k += 1
            C[i, j] = C[j, i] = 0.05 * k * (1 if k % 2 else -1)
    for i in range(6):
        C[i, i] = 9.0 + 1.3 * i
    return scale * C
