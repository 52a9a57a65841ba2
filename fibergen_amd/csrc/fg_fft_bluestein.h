// Transform passes for lengths with a prime factor above 13 (67, 127, 170, 190, 340 ..., every prime): Bluestein's algorithm on
// the Stockham tile kernels of fg_fft_smooth.h.  With c[k] = e^{-i pi k^2 / n} and j k = (j^2 + k^2 - (k - j)^2) / 2
//   X[k] = sum_j x[j] e^{-2 pi i j k / n} = c[k] sum_j (x[j] c[j]) conj c[k - j]
// is a cyclic convolution of length M >= 2 n - 1 with the wrapped conjugate chirp, and M may be any 13-smooth length the tile
// planner has a plan for.  A workgroup holds a tile of whole lines, padded to M points each, in ONE LDS image:
//   load n points per line, times c[j], zeros up to M | M-point passes | times B^ = DFT_M(wrapped conj c) / M, conjugated |
//   the same M-point passes again (the inverse transform as conj DFT conj) | times c[k], scale, store n points
// -- one read and one write of the field per axis, in place, O(M log M) per line instead of the O(n^2) sums such lengths took.
// The inverse direction runs the same phases on the conjugated line.  Three forms: strided (x / y), z with even nz (packed-real
// trick on nz / 2 points, then the real split / merge of fg_fft_core.h), z with odd nz (the row as nz complex points).
// The per-thread code is FG_HD: tests/emulate/emu_bluestein.cpp runs it on the host against numpy.
#pragma once

#include <vector>

#include "fg_fft_smooth.h"

namespace fg {
namespace fft {

constexpr int kBluesteinMin = 64;   // shorter lines stay on the O(n^2) kernels (a 41-point line is 1 681 multiplies; its image would be 81+ points)

struct BluesteinPlan {
  int n = 0;         // line length (z passes: nz / 2, odd nz: nz); 0 = no plan
  SmoothPlan pass;   // the tile plan of the padded length M = pass.n >= 2 n - 1, lines = pass.lines
  int m() const { return n ? pass.n : 0; }
};

inline bool bluestein_is_smooth(int m) {
  for (int f : {2, 3, 5, 7, 11, 13})
    while (m % f == 0) m /= f;
  return m == 1;
}

// smallest 13-smooth M >= 2 n - 1 for which the tile planner has a plan: at >= 2 columns (strided) / >= 1 row (z), image <= kSmoothLdsMax
inline bool bluestein_plan_strided(int n, BluesteinPlan* p) {
  *p = BluesteinPlan();
  if (n < kBluesteinMin) return false;
  for (long m = 2L * n - 1; (size_t)m * 2 * sizeof(cplx) <= kSmoothLdsMax; ++m) {
    if (!bluestein_is_smooth((int)m) || !smooth_plan_strided((int)m, &p->pass)) continue;
    p->n = n;
    return true;
  }
  return false;
}

inline bool bluestein_plan_z(int n, BluesteinPlan* p) {
  *p = BluesteinPlan();
  if (n < kBluesteinMin) return false;
  for (long m = 2L * n - 1; (size_t)smooth_z_pitch((int)m) * sizeof(cplx) <= kSmoothLdsMax; ++m) {
    if (!bluestein_is_smooth((int)m) || !smooth_plan_z((int)m, &p->pass)) continue;
    p->n = n;
    return true;
  }
  return false;
}

// ---- tables (long double, rounded once)
// c[k] = e^{-i pi k^2 / n}, k < n: the index k^2 reduced mod 2 n BEFORE the angle is formed (k^2 ~ 10^6 at n = 1000 would cost
// the angle six digits)
inline std::vector<cplx> make_bluestein_chirp(int n) {
  std::vector<cplx> c(n);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int k = 0; k < n; ++k) {
    const long r = ((long)k * k) % (2L * n);
    const long double a = pi * (long double)r / (long double)n;
    c[k] = cmake((double)cosl(a), (double)-sinl(a));
  }
  return c;
}

// B^[p] = (1 / M) sum_m b[m] e^{-2 pi i m p / M}, b = conj c wrapped: b[m] = b[M - m] = conj c[m], m < n, zero between.
// b is even, so B^[p] = (b[0] + 2 sum_{m = 1}^{n - 1} b[m] cos(2 pi m p / M)) / M
inline std::vector<cplx> make_bluestein_filter(int n, int M) {
  const long double pi = 3.141592653589793238462643383279502884L;
  std::vector<long double> cs(M), br(n), bi(n);
  for (int k = 0; k < M; ++k) cs[k] = cosl(2 * pi * (long double)k / (long double)M);
  for (int k = 0; k < n; ++k) {
    const long r = ((long)k * k) % (2L * n);
    const long double a = pi * (long double)r / (long double)n;
    br[k] = cosl(a), bi[k] = sinl(a);
  }
  std::vector<cplx> f(M);
  for (int p = 0; p < M; ++p) {
    long double sr = 0, si = 0;
    long idx = 0;   // m p mod M
    for (int m = 1; m < n; ++m) {
      idx += p;
      if (idx >= M) idx -= M;
      sr += br[m] * cs[idx];
      si += bi[m] * cs[idx];
    }
    f[p] = cmake((double)((br[0] + 2 * sr) / M), (double)((bi[0] + 2 * si) / M));
  }
  return f;
}

// ---- arguments
struct BluesteinTables {
  const cplx* chirp;   // c[k], k < n
  const cplx* filter;  // B^[p], p < M
  const cplx* w;       // e^{-2 pi i k / M}, k < M: roots of the passes
};

struct BluesteinArgs {   // strided pass: the contract of SmoothArgs (ragged last tile included)
  cplx* data;
  long ls, os;
  int ncols, tiles_per_outer;
  double scale;
  int nt;
  int dir;               // -1 forward, +1 inverse
  int n;
  BluesteinTables t;
  SmoothPlan plan;       // of M; lines = columns per tile (a power of two)
};

struct BluesteinZArgs {
  double* data;          // component base (padded real rows / complex rows)
  long nrows;
  int nzp;
  int nt;
  int fwd;               // 1: r2c, 0: c2r
  int odd;               // 1: nz odd, the row as n = nz complex points; 0: n = nz / 2 packed points
  int n;
  BluesteinTables t;
  const cplx* wz;        // e^{-2 pi i k / nz}, k < nz: real split / merge (even nz)
  SmoothPlan plan;       // of M; lines = rows per tile
};

// ---- the image: point p of line t at p * C + t (strided, C = 2^lg columns) or t * pitch + p (z rows)
struct BluesteinGeom {
  int M, lines, lg, pitch;   // lg < 0: z rows
  FG_HD int total() const { return M * lines; }
  // element idx of the tile's M * lines points (the order the threads sweep them in: memory order) -> line t, point p, LDS slot
  FG_HD int at(int idx, int* t, int* p) const {
    if (lg >= 0) {
      *p = idx >> lg, *t = idx & (lines - 1);
      return idx;
    }
    *t = smooth_div(idx, 1.0 / (double)M), *p = idx - *t * M;
    return *t * pitch + *p;
  }
  FG_HD int slot(int t, int p) const { return lg >= 0 ? (p << lg) + t : t * pitch + p; }
  FG_HD SmoothMap map() const { return lg >= 0 ? SmoothMap{lines, 1, lines, false} : smooth_z_map(M, lines); }
  FG_HD size_t lds_bytes() const { return (size_t)(lg >= 0 ? M * lines : lines * pitch) * sizeof(cplx); }
};

FG_HD BluesteinGeom bluestein_geom_strided(const SmoothPlan& plan) {
  int lg = 0;
  while ((1 << lg) < plan.lines) ++lg;
  return BluesteinGeom{plan.n, plan.lines, lg, 0};
}
FG_HD BluesteinGeom bluestein_geom_z(const SmoothPlan& plan) { return BluesteinGeom{plan.n, plan.lines, -1, smooth_z_pitch(plan.n)}; }

// ---- tile phases (between two workgroup barriers each; thread `tid` of `nthreads`); loads in batches of B as in fg_fft_smooth.h

// strided: columns [col0, col0 + C) of outer index o; x[j] c[j] (inverse: conj x[j] c[j]) -> image, zeros for j >= n
template <int B, bool NTL>
FG_HD void bluestein_strided_load_impl(const BluesteinArgs& a, const BluesteinGeom& G, int block, int tid, int nthreads, cplx* img) {
  const int C = G.lines, o = block / a.tiles_per_outer, col0 = (block % a.tiles_per_outer) * C;
  const long base = (long)o * a.os + col0;
  const int total = G.total();
  for (int i0 = tid; i0 < total; i0 += B * nthreads) {
    cplx v[B], c[B];
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const int idx = i0 + i * nthreads;
      const int p = idx >> G.lg, t = idx & (C - 1);
      const bool in = idx < total && p < a.n;
      v[i] = in && col0 + t < a.ncols ? smooth_cload<NTL>(&a.data[base + (long)p * a.ls + t]) : cmake(0.0, 0.0);
      c[i] = in ? a.t.chirp[p] : cmake(0.0, 0.0);
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const int idx = i0 + i * nthreads;
      if (idx < total) img[idx] = cmul(a.dir > 0 ? cconj(v[i]) : v[i], c[i]);
    }
  }
}

template <int B>
FG_HD void bluestein_strided_load(const BluesteinArgs& a, const BluesteinGeom& G, int block, int tid, int nthreads, cplx* img) {
  if (a.nt & 2) bluestein_strided_load_impl<B, true>(a, G, block, tid, nthreads, img);
  else bluestein_strided_load_impl<B, false>(a, G, block, tid, nthreads, img);
}

// between the two pass sets: A[p] -> conj(A[p] B^[p])  (the second forward transform of the conjugate is the conjugate of the
// inverse transform)
FG_HD void bluestein_filter(const BluesteinGeom& G, const cplx* filter, int tid, int nthreads, cplx* img) {
  for (int idx = tid; idx < G.total(); idx += nthreads) {
    int t, p;
    const int s = G.at(idx, &t, &p);
    img[s] = cconj(cmul(img[s], filter[p]));
  }
}

// the transform's coefficient k of a line from the image after the second pass set: c[k] conj y[k] (inverse: conj c[k] y[k])
FG_HD cplx bluestein_out(cplx y, cplx c, bool inverse) { return inverse ? cmul(cconj(c), y) : cmul(c, cconj(y)); }

FG_HD void bluestein_strided_store(const BluesteinArgs& a, const BluesteinGeom& G, int block, int tid, int nthreads, const cplx* img) {
  const int C = G.lines, o = block / a.tiles_per_outer, col0 = (block % a.tiles_per_outer) * C;
  const long base = (long)o * a.os + col0;
  for (int idx = tid; idx < a.n * C; idx += nthreads) {
    const int p = idx >> G.lg, t = idx & (C - 1);
    if (col0 + t < a.ncols)
      cstore_stream(&a.data[base + (long)p * a.ls + t], cscale(a.scale, bluestein_out(img[idx], a.t.chirp[p], a.dir > 0)), a.nt);
  }
}

// z rows, first phase.  r2c even: the packed real row, n = nz / 2 complex points; r2c odd: the nz reals; c2r odd: the half
// spectrum and its mirror image conj X[nz - k] -- each times the chirp (c2r: conjugated first), zeros from n on.
// c2r even: the n + 1 coefficients as they are (bluestein_z_merge forms the packed line), zeros from n + 1 on.
template <int B, bool NTL>
FG_HD void bluestein_z_load_impl(const BluesteinZArgs& a, const BluesteinGeom& G, long row0, int tid, int nthreads, cplx* img) {
  const int n = a.n, total = G.total(), nzf = n / 2 + 1;
  const bool raw = !a.odd && !a.fwd;
  const double inv = 1.0 / (double)G.M;
  for (int i0 = tid; i0 < total; i0 += B * nthreads) {
    cplx v[B], c[B];
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const int idx = i0 + i * nthreads;
      const int l = smooth_div(idx, inv), p = idx - l * G.M;
      const long row = row0 + l;
      const bool live = idx < total && row < a.nrows;
      const double* rp = a.data + row * a.nzp;
      v[i] = cmake(0.0, 0.0);
      if (a.odd && a.fwd) {
        v[i].re = live && p < n ? rp[p] : 0.0;
      } else if (a.odd) {
        const int k = p < nzf ? p : n - p;   // p >= nzf: the mirror image
        if (live && p < n) v[i] = smooth_cload<NTL>(&reinterpret_cast<const cplx*>(rp)[k]);
        if (k == 0) v[i].im = 0.0;           // FFTW's c2r ignores the imaginary part of the DC bin
        if (p < nzf) v[i].im = -v[i].im;     // conj X[k] here, conj conj X[n - p] = X[n - p] in the mirror half
      } else {
        if (live && p < (raw ? n + 1 : n)) v[i] = smooth_cload<NTL>(&reinterpret_cast<const cplx*>(rp)[p]);
        if (raw && (p == 0 || p == n)) v[i].im = 0.0;   // ... and of the Nyquist bin
      }
      c[i] = idx < total && p < n ? a.t.chirp[p] : cmake(0.0, 0.0);
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const int idx = i0 + i * nthreads;
      const int l = smooth_div(idx, inv), p = idx - l * G.M;
      if (idx < total) img[l * G.pitch + p] = raw ? v[i] : cmul(v[i], c[i]);
    }
  }
}

template <int B>
FG_HD void bluestein_z_load(const BluesteinZArgs& a, const BluesteinGeom& G, long row0, int tid, int nthreads, cplx* img) {
  if (a.nt & 2) bluestein_z_load_impl<B, true>(a, G, row0, tid, nthreads, img);
  else bluestein_z_load_impl<B, false>(a, G, row0, tid, nthreads, img);
}

// c2r even: Z'[k] = merge(X[k], X[n - k]), k < n, then conj Z'[k] c[k] in place: thread (l, k), k <= n / 2, owns the slots k
// and n - k (k = 0: slot n, which becomes part of the zero tail)
FG_HD void bluestein_z_merge(const BluesteinZArgs& a, const BluesteinGeom& G, int tid, int nthreads, cplx* img) {
  const int n = a.n, half = n / 2 + 1, total = G.lines * half;
  const double inv = 1.0 / (double)half;
  for (int idx = tid; idx < total; idx += nthreads) {
    const int l = smooth_div(idx, inv), k = idx - l * half;
    cplx* row = img + l * G.pitch;
    const cplx xk = row[k], xm = row[n - k];
    row[k] = cmul(cconj(c2r_merge(xk, xm, a.wz[k])), a.t.chirp[k]);
    if (k == 0) row[n] = cmake(0.0, 0.0);
    else if (n - k != k) row[n - k] = cmul(cconj(c2r_merge(xm, xk, a.wz[n - k])), a.t.chirp[n - k]);
  }
}

// last phase.  r2c even: the real split X[k], k = 0 .. n, of the packed line's transform; r2c odd: the coefficients
// k = 0 .. nz / 2; c2r even: the n complex points = the nz reals; c2r odd: the real parts
FG_HD void bluestein_z_store(const BluesteinZArgs& a, const BluesteinGeom& G, long row0, int tid, int nthreads, const cplx* img) {
  const int n = a.n;
  const int per = a.fwd ? (a.odd ? n / 2 + 1 : n + 1) : n;
  const double inv = 1.0 / (double)per;
  for (int idx = tid; idx < G.lines * per; idx += nthreads) {
    const int l = smooth_div(idx, inv), k = idx - l * per;
    const long row = row0 + l;
    if (row >= a.nrows) continue;
    const cplx* line = img + l * G.pitch;
    double* rp = a.data + row * a.nzp;
    if (a.fwd && !a.odd) {
      const int k0 = k == n ? 0 : k, k1 = k == 0 ? 0 : n - k;
      const cplx zk = bluestein_out(line[k0], a.t.chirp[k0], false), zmk = bluestein_out(line[k1], a.t.chirp[k1], false);
      cstore_stream(&reinterpret_cast<cplx*>(rp)[k], r2c_split(zk, zmk, a.wz[k]), a.nt);
    } else {
      const cplx x = bluestein_out(line[k], a.t.chirp[k], !a.fwd);
      if (!a.fwd && a.odd) rp[k] = x.re;
      else cstore_stream(&reinterpret_cast<cplx*>(rp)[k], x, a.nt);
    }
  }
}

}  // namespace fft
}  // namespace fg
