// Willot's rotated Green operator ("willot", Willot-R): per-frequency arithmetic of GammaOperatorFourierWillotR
// F:19083-19299, shared by the HIP kernel (fg_kernels_willot.hip) and the host emulation in tests, and the per-axis tables
// the solver builds once per geometry.
//
//   q_a = xi_a d_a / n_a          kvec_a = i tan(q_a / 2) / (4 w_a) (1 + e^{i q_0}) (1 + e^{i q_1}) (1 + e^{i q_2}),  w_a = d_a / n_a
//   r = kvec / (|kvec| + DBL_MIN)
// and the Hermitian 6x6 Gamma_hat of F:19165-19256 in Voigt order 11, 22, 33, 23, 13, 12.
//
// One deviation from the reference.  Its active branch (F:19233-19240) is written in mu_0 / lambda_0 and yields NaN for
// lambda_0 = 0, this library's default; its disabled sibling (F:19243-19250) is the same expression multiplied through by
// lambda_0 and is finite there.  Rule: finite lambda_0 (0 included) takes the multiplied-through form, lambda_0 = infinity
// (the Stokes operator) takes the active form with mu_0 / lambda_0 = 0.  For finite lambda_0 != 0 the two agree to rounding.
#pragma once

#include <cfloat>
#include <cmath>
#include <complex>
#include <vector>

#include "fg_common.h"

namespace fg {

// The scalars of one application: entry = (a1 sumA + b1 B - c1 Q) * inv_den(r2) with
//   finite lambda_0:  a1 = (lambda_0 + 2 mu_0) / 4, b1 = lambda_0, c1 = mu_0, den = mu_0 (d0 - lambda_0 r2), d0 = 2 (lambda_0 + mu_0)
//   lambda_0 = inf:   a1 = 1 / 4,                   b1 = 1,        c1 = 0,    den = mu_0 (2 - r2)
struct WillotCoef {
  double a1, b1, c1, d0, mu_0;
  double alpha, beta;
};

FG_HD WillotCoef willot_coef(double mu_0, double lambda_0, bool inf_lambda, double alpha, double beta) {
  WillotCoef c;
  if (inf_lambda) {
    c.a1 = (1 + 2 * 0.0) * 0.25;
    c.b1 = 1.0;
    c.c1 = 0.0;
    c.d0 = 2 * (1 + 0.0);
  } else {
    c.a1 = (lambda_0 + 2 * mu_0) * 0.25;
    c.b1 = lambda_0;
    c.c1 = mu_0;
    c.d0 = 2 * (lambda_0 + mu_0);
  }
  c.mu_0 = mu_0;
  c.alpha = alpha;
  c.beta = beta;
  return c;
}

// eta_hat = alpha Gamma_hat : tau_hat + beta tau_hat at one non-zero frequency.  ta: the three table entries
// tan(q_a / 2) / (4 w_a), e012 = e_0 e_1 e_2.  Every index below is a compile-time constant once the loops are unrolled.
template <bool INF_LAMBDA>
FG_HD void willot_point(const double* ta, cplx e012, const WillotCoef& cf, const cplx* t, cplx* out) {
  constexpr int vi[6] = {0, 1, 2, 1, 0, 0};   // F:19120-19121
  constexpr int vj[6] = {0, 1, 2, 2, 2, 1};
  cplx kv[3], r[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) kv[a] = cmul(cmake(0.0, ta[a]), e012);   // F:19152
  const double mag_k = std::sqrt((kv[0].re * kv[0].re + kv[0].im * kv[0].im) + (kv[1].re * kv[1].re + kv[1].im * kv[1].im) +
                                 (kv[2].re * kv[2].re + kv[2].im * kv[2].im)) + DBL_MIN;
#pragma unroll
  for (int a = 0; a < 3; ++a) r[a] = cmake(kv[a].re / mag_k, kv[a].im / mag_k);
  // P_ab = r_a conj(r_b) (Hermitian), M_ab = Im P_ab (antisymmetric), RR_ab = r_a r_b
  cplx P[3][3], RR[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      P[a][b] = cmul(r[a], cconj(r[b]));
      RR[a][b] = cmul(r[a], r[b]);
    }
  const cplx rr = cadd(cadd(RR[0][0], RR[1][1]), RR[2][2]);
  const double r2 = rr.re * rr.re + rr.im * rr.im;   // F:19162
  const double den = INF_LAMBDA ? cf.mu_0 * (cf.d0 - r2) : cf.mu_0 * (cf.d0 - cf.b1 * r2);
  const double inv_den = 1.0 / den;

  // s of F:19181-19214 for the pair (x; y, z): z == y ? 4 Im(r_x conj r_z)^2 : -4 Im(r_z conj r_y) Im(r_z conj r_x)
#define FG_WILLOT_S(x, y, z) ((z) == (y) ? 4.0 * P[x][z].im * P[x][z].im : -4.0 * P[z][y].im * P[z][x].im)
  cplx G[6][6];
#pragma unroll
  for (int iv = 0; iv < 6; ++iv) {
#pragma unroll
    for (int jv = iv; jv < 6; ++jv) {
      const int i = vi[iv], j = vj[iv], k = vi[jv], l = vj[jv];
      const double sjk = FG_WILLOT_S(i, j, k), sjl = FG_WILLOT_S(i, j, l), sik = FG_WILLOT_S(j, i, k), sil = FG_WILLOT_S(j, i, l);
      cplx sa = cmake(0.0, 0.0);
      if (j == k) sa = cadd(sa, P[i][l]);
      if (i == k) sa = cadd(sa, P[j][l]);
      if (j == l) sa = cadd(sa, P[i][k]);
      if (i == l) sa = cadd(sa, P[j][k]);
      const cplx sb = cadd(cadd(cadd(cscale(sjk, P[i][l]), cscale(sik, P[j][l])), cscale(sjl, P[i][k])), cscale(sil, P[j][k]));
      const double re_re = P[i][j].re * P[k][l].re;
      cplx num;
      if (INF_LAMBDA) {
        num = cmake(cf.a1 * sa.re + (0.25 * sb.re - re_re), cf.a1 * sa.im + 0.25 * sb.im);
      } else {
        const cplx q = cmul(RR[i][j], cconj(RR[k][l]));
        num = cmake(cf.a1 * sa.re + cf.b1 * (0.25 * sb.re - re_re) - cf.c1 * q.re,
                    cf.a1 * sa.im + cf.b1 * (0.25 * sb.im) - cf.c1 * q.im);
      }
      G[iv][jv] = cscale(inv_den, num);
      if (jv != iv) G[jv][iv] = cconj(G[iv][jv]);   // F:19255
    }
  }
#undef FG_WILLOT_S
#pragma unroll
  for (int iv = 0; iv < 6; ++iv) {
    // the shear columns first, doubled, then the normal ones  F:19260-19268
    cplx c = cadd(cadd(cmul(G[iv][3], t[3]), cmul(G[iv][4], t[4])), cmul(G[iv][5], t[5]));
    c = cscale(2.0, c);
    c = cadd(cadd(cadd(c, cmul(G[iv][0], t[0])), cmul(G[iv][1], t[1])), cmul(G[iv][2], t[2]));
    out[iv] = cmake(cf.alpha * c.re + cf.beta * t[iv].re, cf.alpha * c.im + cf.beta * t[iv].im);   // F:19286
  }
}

// Per-axis tables, evaluated on the host in double with the reference's expressions and their order (F:19089, 19115-19117,
// 19130-19152): the Nyquist index of an even axis maps to q = -pi, where tan(q / 2) ~ -1.6e16 meets 1 + e^{iq} ~ (0, -1.2e-16);
// their product is finite and well conditioned, but it is defined by exactly these table values.  cnt <= n entries.
inline void willot_axis_table(int n, double d, int cnt, std::vector<double>* t, std::vector<cplx>* e) {
  const double xi_0 = 2 * M_PI / d;
  const double w = d / n;
  const bool even = (n & 1) == 0;
  const size_t half = even ? (size_t)(n / 2 - 1) : (size_t)(n / 2);
  t->resize(cnt);
  e->resize(cnt);
  for (size_t i = 0; i < (size_t)cnt; ++i) {
    const double xi = xi_0 * ((i <= half) ? (double)i : ((double)i - (double)n));
    const double q = xi * w;
    const std::complex<double> ex = 1.0 + std::polar<double>(1, q);
    (*t)[i] = 0.25 * std::tan(0.5 * q) / w;
    (*e)[i] = cmake(ex.real(), ex.imag());
  }
}

}  // namespace fg
