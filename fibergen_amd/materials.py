"""Elastic-constant conversion of the project layer: any of the ten supported pairs
(K,E) (K,lambda) (K,mu) (K,nu) (E,mu) (E,nu) (lambda,mu) (lambda,nu) (mu,nu) (mu,M)
-> all six constants.  Mirrors Material::readSettings and calc_from_* (F:7333-7454),
including the "Incomplete" / "Ambiguous material definition" errors."""
from __future__ import annotations

PAIRS = [("K", "E"), ("K", "lambda"), ("K", "mu"), ("K", "nu"), ("E", "mu"),
         ("E", "nu"), ("lambda", "mu"), ("lambda", "nu"), ("mu", "nu"), ("mu", "M")]
NAMES = ("K", "E", "lambda", "mu", "nu", "M")


def _from_K_E(K, E):
    return dict(lam=(3 * K * (3 * K - E)) / (9 * K - E), mu=(3 * K * E) / (9 * K - E), nu=(3 * K - E) / (6 * K),
                M=(3 * K * (3 * K + E)) / (9 * K - E), K=K, E=E)


def _from_K_lambda(K, lam):
    return dict(E=(9 * K * (K - lam)) / (3 * K - lam), mu=(3 * (K - lam)) / 2, nu=lam / (3 * K - lam),
                M=3 * K - 2 * lam, K=K, lam=lam)


def _from_K_mu(K, mu):
    return dict(E=(9 * K * mu) / (3 * K + mu), lam=K - (2 * mu) / 3, nu=(3 * K - 2 * mu) / (2 * (3 * K + mu)),
                M=K + (4 * mu) / 3, K=K, mu=mu)


def _from_K_nu(K, nu):
    return dict(E=3 * K * (1 - 2 * nu), lam=(3 * K * nu) / (1 + nu), mu=(3 * K * (1 - 2 * nu)) / (2 * (1 + nu)),
                M=(3 * K * (1 - nu)) / (1 + nu), K=K, nu=nu)


def _from_E_mu(E, mu):
    return dict(K=(E * mu) / (3 * (3 * mu - E)), lam=(mu * (E - 2 * mu)) / (3 * mu - E), nu=E / (2 * mu) - 1,
                M=(mu * (4 * mu - E)) / (3 * mu - E), E=E, mu=mu)


def _from_E_nu(E, nu):
    return dict(K=E / (3 * (1 - 2 * nu)), lam=(E * nu) / ((1 + nu) * (1 - 2 * nu)), mu=E / (2 * (1 + nu)),
                M=(E * (1 - nu)) / ((1 + nu) * (1 - 2 * nu)), E=E, nu=nu)


def _from_lambda_mu(lam, mu):
    return dict(K=lam + (2 * mu) / 3, E=(mu * (3 * lam + 2 * mu)) / (lam + mu), nu=lam / (2 * (lam + mu)),
                M=lam + 2 * mu, lam=lam, mu=mu)


def _from_lambda_nu(lam, nu):
    return dict(K=(lam * (1 + nu)) / (3 * nu), E=(lam * (1 + nu) * (1 - 2 * nu)) / nu, mu=(lam * (1 - 2 * nu)) / (2 * nu),
                M=(lam * (1 - nu)) / nu, lam=lam, nu=nu)


def _from_mu_nu(mu, nu):
    return dict(K=(2 * mu * (1 + nu)) / (3 * (1 - 2 * nu)), E=2 * mu * (1 + nu), lam=(2 * mu * nu) / (1 - 2 * nu),
                M=(2 * mu * (1 - nu)) / (1 - 2 * nu), mu=mu, nu=nu)


def _from_mu_M(mu, M):
    return dict(K=M - (4 * mu) / 3, E=(mu * (3 * M - 4 * mu)) / (M - mu), lam=M - 2 * mu,
                nu=(M - 2 * mu) / (2 * M - 2 * mu), mu=mu, M=M)


_CALC = {("K", "E"): _from_K_E, ("K", "lambda"): _from_K_lambda, ("K", "mu"): _from_K_mu, ("K", "nu"): _from_K_nu,
         ("E", "mu"): _from_E_mu, ("E", "nu"): _from_E_nu, ("lambda", "mu"): _from_lambda_mu,
         ("lambda", "nu"): _from_lambda_nu, ("mu", "nu"): _from_mu_nu, ("mu", "M"): _from_mu_M}


def material_constants(attrs, evaluate=float):
    """attrs: mapping name -> string/number for a subset of K,E,lambda,mu,nu,M (+ anything else).
    Returns dict with K, E, lambda, mu, nu, M."""
    present = [k for k in NAMES if k in attrs]
    icalc = None
    for pair in PAIRS:  # the last complete pair in table order wins, as in F:7358-7364
        if pair[0] in attrs and pair[1] in attrs:
            icalc = pair
    if icalc is None:
        raise RuntimeError("Incomplete material definition")
    if any(k not in icalc for k in present):
        raise RuntimeError("Ambiguous material definition")
    r = _CALC[icalc](evaluate(attrs[icalc[0]]), evaluate(attrs[icalc[1]]))
    return {"K": r["K"], "E": r["E"], "lambda": r["lam"], "mu": r["mu"], "nu": r["nu"], "M": r["M"]}


# law="general": the combinations it does not cover, in the wording of the solver library (law_refusal in csrc/fg_sweep_plan.h)
GENERAL_MODE_ERROR = "general (anisotropic) phases are available in elasticity mode only"
GENERAL_MIXING_ERROR = ("general (anisotropic) phases support Voigt mixing only (the laminate split is written for isotropic "
                        "phases)")
GENERAL_DFG_ERROR = "general (anisotropic) phases are not available with gamma_scheme full_staggered / half_staggered"
GENERAL_SLAB_ERROR = "general (anisotropic) phases are not available on slab-decomposed solvers"


# law="aniso" (heat / porous): in the wording of the solver library (Solver::set_phase_conductivity)
ANISO_SLAB_ERROR = "aniso (3 x 3 conductivity) phases are not available on slab-decomposed solvers"


def aniso_conductivity(attrs, evaluate=float):
    """MatrixLinearAnisotropicMaterialLaw::readSettings  F:11097-11105: the six attributes c11 c22 c33 c23 c13 c12 of the
    symmetric 3x3 matrix, defaults 1, 1, 1, 0, 0, 0 (F:11094).  Only these six names are read (c21, c31, c32 are not).
    Returns the six numbers in that order."""
    defaults = (("c11", 1.0), ("c22", 1.0), ("c33", 1.0), ("c23", 0.0), ("c13", 0.0), ("c12", 0.0))
    return [evaluate(attrs[k]) if k in attrs else d for k, d in defaults]


def general_stiffness(attrs, evaluate=float):
    """LinearGeneralMaterialLaw::readSettings  F:11240-11245 = read_matrix(attr, C, "c", true)  F:1101-1119 on Voigt::Id4(6)
    F:501-512 (diag 1, 1, 1, 0.5, 0.5, 0.5 -- not the plain identity): i, j row-major, every attribute c<i><j> found sets (i, j)
    and (j, i), so of c12 and c21 the one later in the loop (c21) wins.  Returns the 6x6 list of rows."""
    C = [[0.0] * 6 for _ in range(6)]
    for i in range(6):
        C[i][i] = 1.0 if i < 3 else 0.5
    for i in range(6):
        for j in range(6):
            name = "c%d%d" % (i + 1, j + 1)
            if name in attrs:
                C[i][j] = evaluate(attrs[name])
                C[j][i] = C[i][j]
    return C
