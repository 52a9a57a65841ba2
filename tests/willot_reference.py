"""gamma_scheme willot (Willot's rotated scheme, "Willot-R") restated in NumPy (test infrastructure only).

F = src/fibergen.cpp of the reference.  `WillotMixin.gamma_willot` restates GammaOperatorWillotR F:20322-20330 =
fftTensor, initBCProjector, GammaOperatorFourierWillotR F:19083-19299, applyBCProjector, fftInvTensor, with per-axis tables
and rfftn / irfftn exactly as LSOracle.gamma_collocated does; `basic_scheme` dispatches to it (F:20500) and, for the
viscosity oracle, to DeltaOperatorWillotR F:20380-20418 (F:20483).

One deviation from the reference, the lambda_0 rule: the reference's active branch (F:19233-19240) is written in
mu_0 / lambda_0 and yields NaN for lambda_0 = 0 (this project's default); its disabled sibling (F:19243-19250) is the same
expression multiplied through by lambda_0.  Finite lambda_0 (0 included) takes the multiplied-through form, lambda_0 = inf
takes the active form with mu_0 / lambda_0 = 0.  `form` = "active" / "multiplied" forces one of them (tests compare them).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle.ls_oracle import SMALLEST, LSOracle, voigt_dyad4_mv
from oracle.viscosity_oracle import ViscosityOracle

VI = (0, 1, 2, 1, 0, 0)   # indices for Voigt notation  F:19120-19121
VJ = (0, 1, 2, 2, 2, 1)


def willot_axis_tables(shape, dims):
    """per axis (q[n], tan(q / 2)[n], e[n] = 1 + polar(1, q)) with xi = (2 pi / d) * signed index, q = xi * (d / n)
    F:19089, 19115-19117, 19130-19148; libm per entry like the reference's per-frequency calls"""
    out = []
    for n, d in zip(shape, dims):
        xi_0 = 2 * math.pi / d
        w = d / n
        half = (n // 2 - 1) if (n % 2 == 0) else n // 2
        q = np.array([(xi_0 * (float(i) if i <= half else (float(i) - float(n)))) * w for i in range(n)])
        tn = np.array([math.tan(0.5 * v) for v in q])
        e = np.array([complex(1.0 + math.cos(v), math.sin(v)) for v in q])
        out.append((q, tn, e, w))
    return out


def willot_r(shape, dims):
    """r[3] on the half spectrum [nx, ny, nzc]: kvec_i = (0, 0.25 tan(q_i / 2)) * exp012 / w_i, r = kvec / (|kvec| + small)
    F:19149-19156"""
    tabs = willot_axis_tables(shape, dims)
    nzc = shape[2] // 2 + 1
    bc = [lambda a: a[:, None, None], lambda a: a[None, :, None], lambda a: a[None, None, :nzc]]
    exp012 = bc[0](tabs[0][2]) * bc[1](tabs[1][2]) * bc[2](tabs[2][2])
    kvec = []
    for i in range(3):
        tn, w = tabs[i][1], tabs[i][3]
        kvec.append((1j * (0.25 * bc[i](tn))) * exp012 / w)
    norm = lambda z: z.real * z.real + z.imag * z.imag   # std::norm
    mag_k = np.sqrt(norm(kvec[0]) + norm(kvec[1]) + norm(kvec[2])) + SMALLEST
    return [k / mag_k for k in kvec]


def willot_gamma_hat(r, mu_0, lambda_0, form=None, pairs=None):
    """the 6x6 Gamma_hat per frequency as a dict {(iv, jv): array}, F:19161-19256"""
    if form is None:
        form = "active" if math.isinf(lambda_0) else "multiplied"
    rc = [np.conj(v) for v in r]
    norm = lambda z: z.real * z.real + z.imag * z.imag
    r2 = norm(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    delta = np.eye(3)
    with np.errstate(divide="ignore"):   # F:19091 as the C++ evaluates it: inf for lambda_0 = 0, 0 for lambda_0 = inf
        mu_lambda_0 = float(np.float64(mu_0) / np.float64(lambda_0))
    im = lambda a, b: (r[a] * np.conj(r[b])).imag

    def s(x, y, z):   # F:19183-19214: the pair (y, z) of the entry whose other index is x
        if z == y:
            v = im(x, z)
            return 4.0 * v * v
        return -4.0 * im(z, y) * im(z, x)

    def entry(iv, jv):
        i, j, k, l = VI[iv], VJ[iv], VI[jv], VJ[jv]
        sjk, sjl, sik, sil = s(i, j, k), s(i, j, l), s(j, i, k), s(j, i, l)
        t_delta = (r[i] * rc[l] * delta[j, k] + r[j] * rc[l] * delta[i, k] + r[i] * rc[k] * delta[j, l]
                   + r[j] * rc[k] * delta[i, l])
        t_s = (0.25 * (r[i] * rc[l] * sjk + r[j] * rc[l] * sik + r[i] * rc[k] * sjl + r[j] * rc[k] * sil)
               - (r[i] * rc[j]).real * (r[k] * rc[l]).real)
        if form == "active":      # defined for lambda_0 -> infinity  F:19233-19240
            g = ((1 + 2 * mu_lambda_0) * 0.25 * t_delta + t_s - mu_lambda_0 * r[i] * r[j] * rc[k] * rc[l]) \
                / (mu_0 * (2 * (1 + mu_lambda_0) - r2))
        else:                     # undefined for lambda_0 -> infinity  F:19243-19250
            g = ((lambda_0 + 2 * mu_0) * 0.25 * t_delta + lambda_0 * t_s - mu_0 * r[i] * r[j] * rc[k] * rc[l]) \
                / (mu_0 * (2 * (lambda_0 + mu_0) - lambda_0 * r2))
        return g

    if pairs is not None:   # any entries straight from the formula (the reference evaluates the upper triangle only)
        return {p: entry(*p) for p in pairs}
    gamma = {}
    for iv in range(6):
        for jv in range(iv, 6):
            gamma[iv, jv] = entry(iv, jv)
            gamma[jv, iv] = np.conj(gamma[iv, jv])   # F:19255
    return gamma


def willot_apply_hat(gamma, th, alpha, beta):
    """eta_hat = alpha * ey + beta * tau_hat with the factor 2 on the shear columns, F:19258-19287"""
    eh = np.empty_like(th)
    for iv in range(6):
        c = 0
        for j in range(3, 6):
            c = c + gamma[iv, j] * th[j]
        c = c * 2
        for j in range(3):
            c = c + gamma[iv, j] * th[j]
        eh[iv] = alpha * c + beta * th[iv]
    return eh


class WillotMixin:
    """gamma_scheme "willot" for LSOracle and ViscosityOracle"""

    def _willot_gamma(self, mu_0, lambda_0, form=None):
        key = (float(mu_0), float(lambda_0), form)
        cache = self.__dict__.setdefault("_willot_cache", {})
        if key not in cache:
            cache.clear()
            r = willot_r((self.nx, self.ny, self.nz), (self.dx, self.dy, self.dz))
            with np.errstate(divide="ignore", invalid="ignore"):
                cache[key] = willot_gamma_hat(r, mu_0, lambda_0, form)
        return cache[key]

    def gamma_willot(self, E, mu_0, lambda_0, tau, alpha=-1.0, beta=0.0, form=None):
        """GammaOperatorWillotR  F:20322-20330"""
        th = np.fft.rfftn(tau, axes=(1, 2, 3)) * (1 / float(self.N))
        F0 = th[:, 0, 0, 0].real.copy()   # initBCProjector(tau_hat)  F:20219-20225
        eh = willot_apply_hat(self._willot_gamma(mu_0, lambda_0, form), th, alpha, beta)
        eh[:, 0, 0, 0] = np.asarray(E, dtype=np.float64)   # set zero component  F:19296-19298
        R = alpha * (self.bc_relax * voigt_dyad4_mv(self.BC_MQ, F0)
                     - (1 - self.bc_relax) * voigt_dyad4_mv(self.BC_M, voigt_dyad4_mv(self.BC_QC0, self._F00)))
        eh[:, 0, 0, 0] += R               # applyBCProjector(eta_hat, alpha)  F:20272-20279
        return np.fft.irfftn(eh, s=(self.nx, self.ny, self.nz), axes=(1, 2, 3)) * float(self.N)

    def delta_willot(self, E, mu_0, lambda_0, tau, alpha=-1.0):
        """DeltaOperatorWillotR  F:20380-20418"""
        m = 1 / (4 * mu_0)                                  # fluidity -> viscosity
        tau_copy = tau.copy()
        adj = E - 2 * alpha * m * (tau_copy.reshape(6, -1).sum(axis=1) / self.N)
        eta = self.gamma_willot(adj, -1.0 / (4 * m), math.inf, tau, alpha)
        return eta + (2 * alpha * m) * tau_copy             # eta.xpay(eta, 2 alpha mu_0, tau_copy)

    def basic_scheme(self, E, eps):
        """basicScheme  F:20558-20578 with GammaOperator / DeltaOperator's willot branches  F:20500, F:20483"""
        if isinstance(self, ViscosityOracle):
            self._F00 = np.zeros(6)
            tau = self.calc_stress(self.mu_0, self.lambda_0, eps)
            return self.delta_willot(np.asarray(E, dtype=np.float64), self.mu_0, self.lambda_0, tau, -1.0)
        self._F00 = eps.reshape(6, -1).sum(axis=1) / self.N if self.bc_relax != 1.0 else np.zeros(6)
        tau = self.calc_stress(self.mu_0, self.lambda_0, eps)
        return self.gamma_willot(E, self.mu_0, self.lambda_0, tau, -1.0)


@dataclass
class WillotLSOracle(WillotMixin, LSOracle):
    gamma_scheme: str = "willot"


class WillotViscosityOracle(WillotMixin, ViscosityOracle):
    pass


def make_willot_oracle(n, dims=(1.0, 1.0, 1.0), mixing="voigt", **kw):
    """helpers.make_oracle with the willot scheme: the two-phase sphere problem of the parity tests"""
    from helpers import two_phase_setup
    mats, phis, normals = two_phase_setup(n, mixing)
    return WillotLSOracle(*n, *dims, mats=mats, phis=phis, normals=normals, mixing_rule=mixing, **kw)
