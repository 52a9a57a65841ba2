"""The pressure of mode viscosity, get_raw_field("p") F:15554-15573, restated in NumPy on the oracles (test infrastructure only).

F = src/fibergen.cpp of the reference.  The chain is

  calcStressDiff(epsilon, sigma)  F:18030-18033   sigma = P(epsilon) - 2 mu_0 epsilon     (oracle.calc_stress)
  divOperatorStaggered(sigma, sigma)              the body force, three components        (oracle.div_staggered)
  divVector(sigma, f, 1 / (2 mu_0))  F:19983-20003                                        (div_vector)
  poisson_solve(f, p)  F:23454-23500                                                      (poisson_solve)

  div_vector       b = alpha sum_a (t_a[k] - t_a[k + _ffd_a]) n_a / d_a with the forward offsets of F:14867-14891
  poisson_solve    the division in Fourier space with the reference's transform conventions
  laplacian7       the 7-point periodic Laplacian, the operator poisson_solve inverts (SCALE = 1)
  pressure_rhs / pressure   the chain on an oracle (ViscosityOracle, reuss_reference.ReussViscosityOracle,
                   dfg_reference.DfgViscosityOracle: the mixing rule and the scheme enter through oracle.calc_stress alone)
"""
from __future__ import annotations

import math

import numpy as np

# L_h(poisson_solve(f)) = SCALE * f for every f of zero mean, see poisson_solve
SCALE = 1.0


def div_vector(t, dims, alpha=1.0):
    """divVector  F:19983-20003 on t[3, nx, ny, nz]:  b[k] = (t0[k] - t0[k + _ffd_x[ii]]) chx + (t1[k] - t1[k + _ffd_y[jj]]) chy
    + (t2[k] - t2[k + _ffd_z[kk]]) chz,  ch_a = alpha n_a / d_a.  _ffd_a[i] = ((i + 1) % n - i) * stride (F:14871, 14879, 14887)
    names the NEXT voxel along a, periodic -- each term is the value minus its forward neighbour."""
    nx, ny, nz = t.shape[1:]
    chx, chy, chz = alpha * nx / dims[0], alpha * ny / dims[1], alpha * nz / dims[2]
    return ((t[0] - np.roll(t[0], -1, axis=0)) * chx + (t[1] - np.roll(t[1], -1, axis=1)) * chy
            + (t[2] - np.roll(t[2], -1, axis=2)) * chz)


def poisson_solve(f, dims):
    """poisson_solve  F:23454-23500 on f[nx, ny, nz].

    Scaling conventions, as written in the reference:
      * get_fft(1)->forward is FFT3<double>::forward F:7232-7237 = fftw_execute_dft_r2c: the UNNORMALISED sum
        uc[m] = sum_k f[k] e^{-2 pi i m.k/n}  (numpy.fft.rfftn without a factor);
      * every bin is divided by c (hax (cos xi0 - 1) + hay (cos xi1 - 1) + haz (cos xi2 - 1)) with c = 2 nxyz (F:23463),
        ha_a = n_a^2 / d_a^2 (F:23464-23466), xi_a = (2 pi / n_a) m_a (F:23462, 23471-23482); bin 0 is divided by zero and then
        overwritten with zero (F:23496);
      * get_fft(1)->backward is FFT3<double>::backward F:7239-7244 = fftw_execute_dft_c2r, UNNORMALISED as well
        (numpy.fft.irfftn times nxyz).
    Forward and backward together multiply by nxyz, so u = F^-1[ F[f] / (2 sum_a ha_a (cos xi_a - 1)) ] with the normalised
    inverse.  2 n^2/d^2 (cos xi - 1) is the symbol of (u[k+1] - 2 u[k] + u[k-1]) / h^2, h = d / n: the divisor is the symbol of the
    7-point periodic Laplacian L_h, hence L_h u = f - mean(f) and mean(u) = 0: SCALE = 1."""
    nx, ny, nz = f.shape
    N = nx * ny * nz
    uc = np.fft.rfftn(f)
    c = 2 * float(N)
    hax, hay, haz = nx * nx / (dims[0] * dims[0]), ny * ny / (dims[1] * dims[1]), nz * nz / (dims[2] * dims[2])
    cx = np.array([math.cos(2.0 * math.pi / nx * i) for i in range(nx)])
    cy = np.array([math.cos(2.0 * math.pi / ny * j) for j in range(ny)])
    cz = np.array([math.cos(2.0 * math.pi / nz * k) for k in range(nz // 2 + 1)])
    den = c * (hax * (cx[:, None, None] - 1.0) + hay * (cy[None, :, None] - 1.0) + haz * (cz[None, None, :] - 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        uc = uc / den
    uc[0, 0, 0] = 0.0
    return np.fft.irfftn(uc, s=(nx, ny, nz), axes=(0, 1, 2)) * float(N)


def laplacian7(u, dims):
    """the 7-point periodic Laplacian: sum_a (u[k + e_a] - 2 u[k] + u[k - e_a]) n_a^2 / d_a^2"""
    out = np.zeros_like(u)
    for a in range(3):
        h2 = (u.shape[a] / dims[a]) ** 2
        out += (np.roll(u, -1, axis=a) - 2 * u + np.roll(u, 1, axis=a)) * h2
    return out


def pressure_rhs(oracle, eps=None):
    """the right-hand side f of F:15562-15564 for the strain state eps (default: the oracle's)"""
    eps = oracle.eps if eps is None else eps
    tau = oracle.calc_stress(oracle.mu_0, oracle.lambda_0, eps)
    return div_vector(oracle.div_staggered(tau), (oracle.dx, oracle.dy, oracle.dz), 1 / (2 * oracle.mu_0))


def pressure(oracle, eps=None):
    """get_raw_field("p")  F:15554-15573 -> [nx, ny, nz]"""
    return poisson_solve(pressure_rhs(oracle, eps), (oracle.dx, oracle.dy, oracle.dz))
