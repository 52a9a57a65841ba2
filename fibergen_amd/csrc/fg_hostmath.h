// Small dense host-side algebra of the solver driver: Voigt contractions
// (F:494-598) and the pseudo inverse needed by the boundary-condition projector
// (F:20599-20665).  The reference calls LAPACK gesvd on the symmetric 9x9 matrix
// Q:C0:Q; LAPACK is not available here, a cyclic Jacobi eigen-decomposition gives
// the same Moore-Penrose inverse for a symmetric matrix.
#pragma once

#include <cmath>
#include <cstring>
#include <stdexcept>

namespace fg {
namespace hostmath {

struct Mat6 {
  double a[6][6];
};

inline Mat6 mat6_zero() {
  Mat6 m;
  std::memset(&m, 0, sizeof(m));
  return m;
}

// Voigt::Id4(6)  F:501-512
inline Mat6 voigt_id4() {
  Mat6 m = mat6_zero();
  for (int i = 0; i < 3; ++i) m.a[i][i] = 1.0;
  for (int i = 3; i < 6; ++i) m.a[i][i] = 0.5;
  return m;
}

// Voigt::II4(6)  F:517-525
inline Mat6 voigt_ii4() {
  Mat6 m = mat6_zero();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m.a[i][j] = 1.0;
  return m;
}

// Voigt::dyad4(M, v): shear entries of v doubled  F:563-575
inline void voigt_mv(const Mat6& M, const double* v, double* out) {
  double vc[6];
  for (int i = 0; i < 6; ++i) vc[i] = v[i];
  vc[3] *= 2;
  vc[4] *= 2;
  vc[5] *= 2;
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
    for (int j = 0; j < 6; ++j) s += M.a[i][j] * vc[j];
    out[i] = s;
  }
}

// calcBCMean  F:20242-20245: E = E0 + bc_relax M:(S0 - QC0:E0)
inline void bc_mean(const Mat6& QC0, const Mat6& M, double bc_relax, const double* E0, const double* S0, double* E) {
  double t1[6], t2[6], t3[6];
  voigt_mv(QC0, E0, t1);
  for (int i = 0; i < 6; ++i) t2[i] = S0[i] - t1[i];
  voigt_mv(M, t2, t3);
  for (int i = 0; i < 6; ++i) E[i] = E0[i] + bc_relax * t3[i];
}

// applyBCProjector  F:20247-20270: R = alpha (bc_relax MQ:F0 - (1 - bc_relax) M:(QC0:F00)), F0 = <tau>, F00 = mean of the
// operator's argument
inline void bc_correction(const Mat6& MQ, const Mat6& M, const Mat6& QC0, double bc_relax, double alpha, const double* F0,
                          const double* F00, double* R) {
  double t1[6], t2[6], t3[6];
  voigt_mv(MQ, F0, t1);
  voigt_mv(QC0, F00, t2);
  voigt_mv(M, t2, t3);
  for (int i = 0; i < 6; ++i) R[i] = alpha * (bc_relax * t1[i] - (1 - bc_relax) * t3[i]);
}

// Voigt::dyad4(A, B) column by column  F:582-597
inline Mat6 voigt_mm(const Mat6& A, const Mat6& B) {
  Mat6 C;
  for (int c = 0; c < 6; ++c) {
    double col[6], out[6];
    for (int i = 0; i < 6; ++i) col[i] = B.a[i][c];
    voigt_mv(A, col, out);
    for (int i = 0; i < 6; ++i) C.a[i][c] = out[i];
  }
  return C;
}

// Voigt::norm_2  F:530-537
inline double voigt_norm2(const double* v) {
  double s = 0.0;
  for (int i = 0; i < 6; ++i) s += v[i] * v[i];
  return std::sqrt(s + v[3] * v[3] + v[4] * v[4] + v[5] * v[5]);
}

inline double frobenius(const Mat6& m) {
  double s = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) s += m.a[i][j] * m.a[i][j];
  return std::sqrt(s);
}

inline double norm2(const double* v, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += v[i] * v[i];
  return std::sqrt(s);
}

// bc_error  F:21129-21161 from the two means: max of |P:<eps> - E| / |P:E| and |Q:<sigma> - S| / |S| (a norm below bc_tol
// divides by 1)
inline double bc_error_value(const Mat6& P, const Mat6& Q, double bc_tol, const double* Emean, const double* Smean,
                             const double* E_cur, const double* S_cur) {
  double PE[6], QS[6], PEc[6], d[6];
  voigt_mv(P, Emean, PE);
  voigt_mv(Q, Smean, QS);
  voigt_mv(P, E_cur, PEc);
  const double norm_E = voigt_norm2(PEc);
  for (int i = 0; i < 6; ++i) d[i] = PE[i] - E_cur[i];
  const double err_F = voigt_norm2(d) / ((norm_E < bc_tol) ? 1 : norm_E);
  const double norm_S = voigt_norm2(S_cur);
  for (int i = 0; i < 6; ++i) d[i] = QS[i] - S_cur[i];
  const double err_S = voigt_norm2(d) / ((norm_S < bc_tol) ? 1 : norm_S);
  return err_F > err_S ? err_F : err_S;
}

// LSSolver::run's check of the prescribed values against the projector  F:21356-21364: P:S and Q:E must vanish
inline void check_bc_compatible(const Mat6& P, const Mat6& Q, const double* Emax, const double* Smax) {
  const double se = std::sqrt(2.220446049250313e-16);
  double t[6];
  voigt_mv(P, Smax, t);
  if (norm2(t, 6) > se * norm2(Smax, 6)) throw std::runtime_error("Incompatible stress boundary condition specified");
  voigt_mv(Q, Emax, t);
  if (norm2(t, 6) > se * norm2(Emax, 6)) throw std::runtime_error("Incompatible strain boundary condition specified");
}

// runLoadsteppingSolver  F:21584-21685: the steps first .. nparams - 1 of a load path, and the prescribed values of the step with
// parameter t
inline void check_load_steps(const double* params, int nparams, int first) {
  if (nparams < 1 || first < 0 || !params) throw std::runtime_error("invalid load steps");
}
inline void load_step_values(double t, const double* Emax, const double* Smax, double* E, double* S) {
  for (int i = 0; i < 6; ++i) E[i] = t * Emax[i], S[i] = t * Smax[i];
}

// getRefMaterial  F:12153-12236 on the extreme tangent eigenvalues: the lower one clamped at 0 (F:12183-12223), their
// arithmetic mean -- method polarization (2): their geometric mean, F:12227-12229 --, halved and scaled
inline double ref_mu0(double lambda_min, double lambda_max, int method, double ref_scale) {
  if (lambda_min < 0) lambda_min = 0;
  double mu_0 = method == 2 ? std::sqrt(lambda_min * lambda_max) : 0.5 * (lambda_min + lambda_max);
  mu_0 *= 0.5 * ref_scale;
  return mu_0;
}

// Weights of the polynomial load-step extrapolation  F:21468-21514: w = V^-T tpowers with V_ij = t_i^j, i.e. V^T w = tpowers
// with tpowers_i = t_new^i, by Gauss elimination with partial pivoting (n <= 8).  False: a pivot is zero ("Error inverting
// Vandermonde matrix", F:21487-21490), w is not written.
inline bool extrapolation_weights(const double* t, int n, double t_new, double* w) {
  double A[8][9];
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[i][j] = std::pow(t[j], i);   // (V^T)_ij = t_j^i
    A[i][n] = std::pow(t_new, i);
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    if (A[piv][c] == 0.0) return false;
    for (int j = 0; j <= n; ++j) {
      const double s = A[c][j];
      A[c][j] = A[piv][j], A[piv][j] = s;
    }
    for (int r = c + 1; r < n; ++r) {
      const double m = A[r][c] / A[c][c];
      for (int j = c; j <= n; ++j) A[r][j] -= m * A[c][j];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double v = A[r][n];
    for (int j = r + 1; j < n; ++j) v -= A[r][j] * w[j];
    w[r] = v / A[r][r];
  }
  return true;
}

// Symmetric N x N eigen-decomposition by cyclic Jacobi: A = V diag(w) V^T.
template <int N>
inline void jacobi_eig(double A[N][N], double V[N][N], double w[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    if (off == 0.0) break;
    for (int p = 0; p < N; ++p) {
      for (int q = p + 1; q < N; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    }
  }
  for (int i = 0; i < N; ++i) w[i] = A[i][i];
}

// Moore-Penrose inverse of the symmetric 6x6 Voigt operator Q:C0:Q through its
// 9x9 extension, then folded back to 6x6 -- setBCProjector  F:20621-20661.
inline Mat6 bc_pseudo_inverse(const Mat6& QC0Q) {
  double A[9][9], V[9][9], w[9];
  for (int i = 0; i < 9; ++i)
    for (int j = i; j < 9; ++j) A[j][i] = A[i][j] = QC0Q.a[i < 6 ? i : i - 3][j < 6 ? j : j - 3];
  jacobi_eig<9>(A, V, w);
  double snorm = 0.0;
  for (int i = 0; i < 9; ++i) snorm += w[i] * w[i];
  const double alpha = std::sqrt(2.220446049250313e-16) * std::sqrt(snorm);
  double M[9][9];
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) {
      double s = 0.0;
      for (int k = 0; k < 9; ++k)
        if (std::fabs(w[k]) > alpha) s += V[i][k] * V[j][k] / w[k];
      M[i][j] = s;
    }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 6; ++j) M[j][3 + i] = 0.5 * (M[j][3 + i] + M[j][6 + i]);
    for (int j = 0; j < 6; ++j) M[3 + i][j] = 0.5 * (M[3 + i][j] + M[6 + i][j]);
  }
  Mat6 out;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) out.a[i][j] = M[i][j];
  return out;
}

}  // namespace hostmath
}  // namespace fg
