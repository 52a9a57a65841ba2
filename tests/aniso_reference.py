"""law="aniso" of the scalar modes (a constant symmetric 3x3 conductivity per phase) restated in NumPy on ScalarOracle (test
infrastructure only).

F = src/fibergen.cpp of the reference.  A material is either the number mu (ScalarLinearIsotropicMaterialLaw F:11158-11215) or a
symmetric 3x3 array K (MatrixLinearAnisotropicMaterialLaw F:11087-11156, attributes c11 c22 c33 c23 c13 c12).

  aniso3              PK1 F:11114-11128 in its operation order
  pk1_voigt_aniso     VoigtMixedMaterialLaw::PK1 F:12752-12761 over mixed iso / aniso phases
  voigt_tangent3      the matrix eig() hands dsyev (F:12518-12522) for DIM = 3: dPK1 (F:12763-12771 over F:11130-11150 and
                      F:11200-11222) of the identity rows
  AnisoScalarOracle   ScalarOracle with these two; the scan takes numpy.linalg.eigvalsh per voxel

calcStress F:18134-18184 evaluates the law per voxel index on the three stored gradient components; ScalarOracle.calc_stress
already does (its arrays are indexed by voxel), so the 13-point stencil of the product follows from pk1 alone.
"""
from __future__ import annotations

import numpy as np

from oracle.scalar_oracle import VOIGT_THRESHOLD, ScalarOracle


def is_aniso(mat):
    return np.ndim(mat) == 2


def k6(K):
    """the six constants in the order of the C interface: 11, 22, 33, 23, 13, 12"""
    K = np.asarray(K, dtype=np.float64)
    return np.array([K[0, 0], K[1, 1], K[2, 2], K[1, 2], K[0, 2], K[0, 1]])


def aniso3(E, K, alpha=1.0):
    """MatrixLinearAnisotropicMaterialLaw::PK1  F:11114-11128: S[c] = alpha * (K_c0 E_0 + K_c1 E_1 + K_c2 E_2), summed left
    to right; E is [3, ...], alpha may be an array (phi * alpha of the Voigt mixing)"""
    S = np.empty_like(E)
    for c in range(3):
        S[c] = alpha * (K[c, 0] * E[0] + K[c, 1] * E[1] + K[c, 2] * E[2])
    return S


def iso3(E, mu, alpha=1.0):
    """ScalarLinearIsotropicMaterialLaw::PK1  F:11182-11198: S_m = E_m * (alpha * mu)"""
    return E * (alpha * mu)


def pk1_voigt_aniso(g, phis, mats, alpha=1.0):
    """VoigtMixedMaterialLaw<.,.,3>::PK1  F:12752-12761: phases with phi <= 10 eps skipped, the first one that counts assigns,
    the others accumulate; the law is called with phi * alpha"""
    P = np.zeros_like(g)
    first = np.ones(g.shape[1:], dtype=bool)
    for phi, mat in zip(phis, mats):
        use = phi > VOIGT_THRESHOLD
        S = aniso3(g, np.asarray(mat, dtype=np.float64), phi * alpha) if is_aniso(mat) else iso3(g, mat, phi * alpha)
        P = np.where(use & first, S, np.where(use, P + S, P))
        first = first & ~use
    return P


def voigt_tangent3(phis, mats):
    """[nx, ny, nz, 3, 3]: eig() F:12518-12522 calls dPK1(i, F, 1, false, Id, dP, 3).  Row m of what
    MatrixLinearAnisotropicMaterialLaw::dPK1 F:11130-11150 fills from identity row m is alpha * K(:, m) (the products with the
    zeros of the identity row are exact), the scalar law's F:11200-11222 is alpha * mu * e_m; VoigtMixedMaterialLaw::dPK1
    F:12763-12771 calls them with alpha = phi * 1 for the phases above its threshold, the first assigning, the others
    accumulating.  The matrix is symmetric, so which triangle dsyev reads makes no difference for DIM = 3."""
    A = np.zeros(np.shape(phis[0]) + (3, 3))
    first = np.ones(np.shape(phis[0]), dtype=bool)
    for phi, mat in zip(phis, mats):
        use = phi > VOIGT_THRESHOLD
        if is_aniso(mat):
            t = (phi * 1.0)[..., None, None] * np.asarray(mat, dtype=np.float64).T
        else:
            t = ((phi * 1.0) * float(mat))[..., None, None] * np.eye(3)
        A = np.where((use & first)[..., None, None], t, np.where(use[..., None, None], A + t, A))
        first = first & ~use
    return A


class AnisoScalarOracle(ScalarOracle):
    """ScalarOracle whose materials may be symmetric 3x3 conductivities: mus[p] is a number or a 3x3 array"""

    def pk1(self, g, alpha=1.0):
        if not any(is_aniso(m) for m in self.mus):
            return super().pk1(g, alpha)
        return pk1_voigt_aniso(g, self.phis, self.mus, alpha)

    def calc_ref_material(self):
        """calcRefMaterial  F:22283-22313 over getRefMaterial / eig  F:12153-12236, F:12472-12559: the extreme eigenvalues of
        the per-voxel tangent over all voxels, a negative minimum cut to 0, mu_0 = (min + max) / 2 * ref_scale / 2"""
        if not any(is_aniso(m) for m in self.mus):
            return super().calc_ref_material()
        lo, hi = self.tangent_eig_minmax()
        if lo < 0:
            lo = 0.0
        self.mu_0 = 0.5 * (lo + hi) * (0.5 * self.ref_scale)

    def tangent_eig_minmax(self):
        A = voigt_tangent3(self.phis, self.mus).reshape(-1, 3, 3)
        A = np.unique(A, axis=0) if A.shape[0] > 4096 else A
        w = np.linalg.eigvalsh(A)
        return float(w.min()), float(w.max())


class FixedRefOracle(AnisoScalarOracle):
    """the restatement run with a reference medium handed in (the product's), so that the last bits of mu_0 do not decide the
    histories: calc_ref_material keeps self.mu_0"""

    def calc_ref_material(self):
        if np.isnan(self.mu_0):
            raise RuntimeError("FixedRefOracle needs mu_0")


def random_spd3(rng, scale=1.0):
    """a random symmetric positive definite 3x3 with six distinct constants and non-zero off-diagonals"""
    B = rng.standard_normal((3, 3))
    K = B @ B.T + 1.5 * np.eye(3)
    K = 0.5 * (K + K.T)
    return scale * K / np.trace(K) * 3.0


# ---- the laminate: a closed form the staggered discretisation reproduces exactly (every field depends on one coordinate)
def layer_problem(axis, seed=21):
    """three layers normal to `axis` on the 20 x 4 x 6 grid turned so that `axis` has 20 voxels; distinct full SPD K per layer"""
    rng = np.random.default_rng(seed)
    fr = [0.2, 0.3, 0.5]
    shape = [4, 6]
    shape.insert(axis, 20)
    shape = tuple(shape)
    edges = np.round(np.cumsum([0.0] + fr) * 20).astype(int)
    phis = []
    for a, b in zip(edges[:-1], edges[1:]):
        p = np.zeros(shape)
        sl = [slice(None)] * 3
        sl[axis] = slice(a, b)
        p[tuple(sl)] = 1.0
        phis.append(p)
    Ks = [random_spd3(rng, s) for s in (1.0, 5.0, 0.5)]
    return shape, fr, edges, phis, Ks


def laminate_closed_form(axis, fr, Ks, E):
    """q_a uniform, g_b = E_b for b != a, g_a per layer from q_a = K_aa g_a + sum_{b != a} K_ab E_b, <g_a> = E_a"""
    others = [b for b in range(3) if b != axis]
    shift = [sum(K[axis, b] * E[b] for b in others) for K in Ks]
    qa = (E[axis] + sum(f * s / K[axis, axis] for f, s, K in zip(fr, shift, Ks))) / sum(f / K[axis, axis] for f, K in zip(fr, Ks))
    ga = [(qa - s) / K[axis, axis] for s, K in zip(shift, Ks)]
    return qa, ga


def check_laminate(axis, eps, sigma, fr, edges, Ks, E, tol):
    qa, ga = laminate_closed_form(axis, fr, Ks, E)
    scale = np.abs(E).max()
    assert np.abs(sigma[axis] - qa).max() <= tol * abs(qa)
    for b in range(3):
        if b != axis:
            assert np.abs(eps[b] - E[b]).max() <= tol * scale
    for (a, b), gl in zip(zip(edges[:-1], edges[1:]), ga):
        sl = [slice(None)] * 3
        sl[axis] = slice(a, b)
        assert np.abs(eps[axis][tuple(sl)] - gl).max() <= tol * max(scale, abs(gl))
