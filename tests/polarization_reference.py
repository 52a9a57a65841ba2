"""method "polarization" (the Eyre-Milton scheme) restated in NumPy on the oracles (test infrastructure only).

F = src/fibergen.cpp of the reference.

  polarize_iso        LinearIsotropicMaterialLaw::calcPolarization F:11427-11467 in its operation order
  tangent_full        the FULL matrix dPK1 fills from the identity rows (F:10431, F:9068-9075, F:11274-11298, F:12763-12771):
                      row m = C(:, m) f_m, f = (1, 1, 1, 2, 2, 2) -- not symmetric when normal and shear components couple
  polarize_generic    MaterialLaw::calcPolarization F:10414-10445: (C + 2 mu_0 Id) R = F (numpy.linalg.solve for gesv),
                      Q = C R - 2 mu_0 R, Id the plain identity on the six stored components
  calc_polarization   calcPolarization F:18044-18131 through MixedMaterialLaw::calcPolarization F:12087-12099: the first phase
                      with phi == 1 (exact) answers with its own law -- an isotropic one in closed form; a general one has no
                      form of its own (the reference's throws, F:11303) and takes the generic one like every mixed voxel
  polarization_scheme polarizationScheme F:20536-20554; run_polarization: runPolarization F:21808-21851

gamma_scheme collocated and willot follow the reference (beta = 1 honoured, F:19286-19734).  gamma_scheme "staggered" is the
project's STATED DEVIATION: GammaOperatorStaggered F:20288-20300 takes beta and drops it; the consistent form
P <- Q - 4 mu_0 grad_s_h G0 div_h Q with its mean replaced by P00 + P0 is restated here, the reference's pass as written is kept
as scheme "staggered_as_written" (it does not converge to the cell problem's solution: test_polarization_reference.py).
Also unlike the reference, whose loop never advances its iteration counter, iterations are counted and maxiter ends the loop.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

import general_reference as gr
from oracle.ls_oracle import SMALLEST, VOIGT_THRESHOLD, LSOracle
from willot_reference import WillotMixin

F6 = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])


def polarize_iso(F, mu, lam, mu_0, inv=False):
    """F:11444-11465; F is [6, ...]"""
    m = 2.0 * (mu + mu_0)
    a = 1.0 / m
    b = lam / (m * (3.0 * lam + m))
    tr_F = F[0] + F[1] + F[2]
    P = np.empty_like(F)
    for i in range(3):
        P[i] = a * F[i] - b * tr_F
        P[3 + i] = a * F[3 + i]
    if not inv:
        m = 2.0 * (mu - mu_0)
        tr_P = P[0] + P[1] + P[2]
        for i in range(3):
            P[i] = m * P[i] + lam * tr_P
            P[3 + i] = m * P[3 + i]
    return P


def dpk1_matrix(mat):
    """the matrix dPK1 fills from the identity rows for one phase: M[m, i] = C[i, m] f_m"""
    C = np.asarray(mat, dtype=np.float64) if gr.is_general(mat) else gr.iso_stiffness(*mat)
    return C.T * F6[:, None]


def tangent_full(phis, mats):
    """[..., 6, 6]: sum_p phi_p dpk1_matrix(C_p) over the phases above the Voigt threshold"""
    A = np.zeros(np.shape(phis[0]) + (6, 6))
    for phi, mat in zip(phis, mats):
        w = np.where(phi > VOIGT_THRESHOLD, phi, 0.0)
        A = A + w[..., None, None] * dpk1_matrix(mat)
    return A


def polarize_generic(F, C, mu_0, inv=False):
    """F:10431-10444; F is [6, ...], C is [..., 6, 6]"""
    Fv = np.moveaxis(F, 0, -1)[..., None]
    R = np.linalg.solve(C + 2.0 * mu_0 * np.eye(6), Fv)
    out = R if inv else C @ R - 2.0 * mu_0 * R
    return np.moveaxis(out[..., 0], -1, 0)


def generic_mask(phis, mats):
    """voxels that take the 6 x 6 solve: no isotropic phase with phi == 1 before any general phase with phi == 1"""
    decided = np.zeros(np.shape(phis[0]), dtype=bool)
    iso = np.zeros_like(decided)
    for phi, mat in zip(phis, mats):
        one = (phi == 1) & ~decided
        if not gr.is_general(mat):
            iso |= one
        decided |= one
    return ~iso


def polarization_plan(phis, mats):
    """what does not change from pass to pass: the voxels of the 6 x 6 solve with their matrices, and per isotropic phase the
    voxels it answers for"""
    gen = generic_mask(phis, mats)
    plan = {"generic": gen, "C": tangent_full([phi[gen] for phi in phis], mats), "iso": []}
    decided = np.zeros(np.shape(phis[0]), dtype=bool)
    for phi, mat in zip(phis, mats):
        one = (phi == 1) & ~decided
        if not gr.is_general(mat):
            plan["iso"].append((one, mat))
        decided |= one
    return plan


def calc_polarization(F, phis, mats, mu_0, inv=False, plan=None):
    plan = polarization_plan(phis, mats) if plan is None else plan
    out = np.empty_like(F)
    gen = plan["generic"]
    out[:, gen] = polarize_generic(F[:, gen], plan["C"], mu_0, inv)
    for one, mat in plan["iso"]:
        out[:, one] = polarize_iso(F[:, one], mat[0], mat[1], mu_0, inv)
    return out


@dataclass
class PolarizationOracle(WillotMixin, gr.GeneralLSOracle):
    """GeneralLSOracle (+ the willot operator) with runPolarization; gamma_scheme "staggered", "collocated", "willot" or
    "staggered_as_written" (polarisation loop only)"""

    def basic_scheme(self, E, eps):
        if self.gamma_scheme == "willot":
            return WillotMixin.basic_scheme(self, E, eps)
        return LSOracle.basic_scheme(self, E, eps)

    def calc_ref_material_polarization(self):
        """calcRefMaterial F:22283-22313 with getRefMaterial(..., polarization = true) F:12227-12229"""
        lo, hi = self.tangent_eig_minmax()
        lo = max(lo, 0.0)
        self.mu_0 = math.sqrt(lo * hi) * 0.5 * self.ref_scale
        self._set_bc_projector(self.BC_P)

    def calc_polarization(self, P, inv=False):
        if "_polar_plan" not in self.__dict__:   # phases and materials of an oracle do not change
            self._polar_plan = polarization_plan(self.phis, self.mats)
        return calc_polarization(P, self.phis, self.mats, self.mu_0, inv, self._polar_plan)

    def polarization_scheme(self, P0, P):
        """polarizationScheme F:20536-20554: one pass on the polarisation field"""
        Q = self.calc_polarization(P)
        P00 = Q.reshape(6, -1).sum(axis=1) / self.N
        alpha = -4 * self.mu_0
        if self.gamma_scheme == "collocated":
            return self.gamma_collocated(P00 + P0, self.mu_0, self.lambda_0, Q, alpha, 1.0)
        if self.gamma_scheme == "willot":
            return self.gamma_willot(P00 + P0, self.mu_0, self.lambda_0, Q, alpha, 1.0)
        if self.gamma_scheme == "staggered_as_written":   # GammaOperatorStaggered F:20288-20300: beta dropped
            return self.gamma_staggered(P00 + P0, self.mu_0, self.lambda_0, Q, alpha)
        # the consistent staggered form: sym grad_h of a periodic u has zero mean, so <Q> = P00 passes through unchanged
        u = self.g0_staggered(self.mu_0, self.lambda_0, self.div_staggered(Q), alpha)
        return Q + self.eps_staggered(P0, u)

    def run_polarization(self, E0, callback=None):
        """runPolarization F:21808-21851, one load step continuing from self.eps (zero for a first step), pure-strain boundary
        conditions.  Returns True on error.  callback(iteration, P) after every pass."""
        E = np.asarray(E0, dtype=np.float64)
        self.residuals = []
        prev = self._norm9(self.component_norm(self.eps))   # the estimator's constructor  F:21814
        if self.update_ref != "never":
            self.calc_ref_material_polarization()
        P0 = 4 * self.mu_0 * E
        P = np.empty_like(self.eps)
        P[:] = P0[:, None, None, None]
        it = 1
        failed = False
        while True:
            P = self.polarization_scheme(P0, P)
            cur = self._norm9(self.component_norm(P))
            abs_err = abs(prev - cur)
            rel_err = abs_err / (SMALLEST + cur)
            prev = cur
            if self.error_estimator == "none":
                abs_err = rel_err = 1.0
            if math.isnan(rel_err):
                failed = True
                break
            self.residuals.append(rel_err)
            if callback is not None:
                callback(it, P)
            if it >= self.maxiter or rel_err <= self.tol or abs_err <= self.abs_tol:   # check_bc = false  F:21819
                break
            it += 1
        self.iterations = it
        self.P = P
        self.eps = self.calc_polarization(P, inv=True)   # F:21850
        return failed

    def run_polarization_steps(self, E0, params):
        """runLoadsteppingSolver F:21584-21685 over runPolarization: every step continues from the strain of the one before"""
        self.eps = np.zeros((6, self.nx, self.ny, self.nz))
        self.step_iterations, res = [], []
        for t in params:
            if self.run_polarization(float(t) * np.asarray(E0, dtype=np.float64)):
                return True
            self.step_iterations.append(self.iterations)
            res += self.residuals
        self.residuals = res
        return False


def sphere_phi(shape, radius=0.35, smooth=True):
    """a centred sphere inclusion: phi_1 in {0, 1}, with a shell of mixed voxels when smooth"""
    ax = [(np.arange(n) + 0.5) / n - 0.5 for n in shape]
    r = np.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
    h = 1.0 / min(shape)
    phi1 = np.clip((radius - r) / h + 0.5, 0.0, 1.0) if smooth else (r < radius).astype(np.float64)
    return [1.0 - phi1, phi1]


def make_polarization_oracle(shape, mats, phis=None, scheme="collocated", **kw):
    phis = sphere_phi(shape) if phis is None else phis
    return PolarizationOracle(*shape, mats=list(mats), phis=list(phis), gamma_scheme=scheme, **kw)
