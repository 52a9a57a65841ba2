// Stand-alone run of the Bluestein emulation (emu_bluestein.cpp) for sanitizer builds: g++ -fsanitize=address,undefined,
// no shared library, no preloaded runtime.  Lengths: strided 67, z even nz = 136, z odd nz = 127; ragged tiles, two directions
// each; the results against direct O(n^2) sums.  Exit status 0 = clean and correct.
#include <cstdio>

#include "emu_bluestein.cpp"

static double urand(unsigned* s) {
  *s = *s * 1664525u + 1013904223u;
  return (double)(*s >> 8) / (double)(1u << 24) - 0.5;
}

static int check_strided(int n, int dir) {
  const int ncols = 11, nouter = 2;
  unsigned seed = 7u + n;
  std::vector<cplx> x((size_t)nouter * n * ncols);
  for (auto& v : x) v = cmake(urand(&seed), urand(&seed));
  std::vector<cplx> y = x;
  if (emu_bluestein_strided(n, dir, reinterpret_cast<double*>(y.data()), ncols, nouter, 0.5)) return 1;
  const long double two_pi = 6.283185307179586476925286766559005768L;
  double err = 0, top = 0;
  for (int o = 0; o < nouter; ++o)
    for (int c = 0; c < ncols; ++c)
      for (int k = 0; k < n; ++k) {
        long double sr = 0, si = 0;
        for (int j = 0; j < n; ++j) {
          const long double a = dir * two_pi * (long double)(((long)j * k) % n) / n, cr = cosl(a), ci = sinl(a);
          const cplx v = x[((size_t)o * n + j) * ncols + c];
          sr += v.re * cr - v.im * ci;
          si += v.re * ci + v.im * cr;
        }
        const cplx g = y[((size_t)o * n + k) * ncols + c];
        err = fmax(err, fmax(fabs(g.re - 0.5 * (double)sr), fabs(g.im - 0.5 * (double)si)));
        top = fmax(top, fmax(fabs((double)sr), fabs((double)si)));
      }
  std::printf("strided n=%d dir=%+d rel err %.3g\n", n, dir, err / top);
  return err / top < 1e-13 ? 0 : 2;
}

static int check_z(int nz) {
  const long nrows = 5;
  const int nzc = nz / 2 + 1, nzp = 2 * nzc;
  unsigned seed = 11u + nz;
  const long double two_pi = 6.283185307179586476925286766559005768L;
  std::vector<double> buf((size_t)nrows * nzp, NAN), x((size_t)nrows * nz);
  for (long r = 0; r < nrows; ++r)
    for (int m = 0; m < nz; ++m) buf[r * nzp + m] = x[r * nz + m] = urand(&seed);
  if (emu_bluestein_z(nz, 1, buf.data(), nrows)) return 1;
  double err = 0, top = 0;
  for (long r = 0; r < nrows; ++r)
    for (int k = 0; k < nzc; ++k) {
      long double sr = 0, si = 0;
      for (int m = 0; m < nz; ++m) {
        const long double a = -two_pi * (long double)(((long)m * k) % nz) / nz;
        sr += x[r * nz + m] * cosl(a);
        si += x[r * nz + m] * sinl(a);
      }
      err = fmax(err, fmax(fabs(buf[r * nzp + 2 * k] - (double)sr), fabs(buf[r * nzp + 2 * k + 1] - (double)si)));
      top = fmax(top, fmax(fabs((double)sr), fabs((double)si)));
    }
  std::printf("r2c nz=%d rel err %.3g\n", nz, err / top);
  if (!(err / top < 1e-13)) return 2;
  // c2r of a non-Hermitian spectrum: the imaginary parts of the DC (and Nyquist) bins are ignored
  std::vector<double> X((size_t)nrows * nzp);
  for (auto& v : X) v = urand(&seed);
  buf = X;
  if (emu_bluestein_z(nz, 0, buf.data(), nrows)) return 1;
  err = top = 0;
  for (long r = 0; r < nrows; ++r)
    for (int m = 0; m < nz; ++m) {
      long double s = X[r * nzp];
      for (int k = 1; k < nzc; ++k) {
        const long double a = two_pi * (long double)(((long)m * k) % nz) / nz;
        const double re = X[r * nzp + 2 * k], im = X[r * nzp + 2 * k + 1];
        if (nz % 2 == 0 && k == nz / 2) s += re * cosl(a);
        else s += 2 * (re * cosl(a) - im * sinl(a));
      }
      err = fmax(err, fabs(buf[r * nzp + m] - (double)s));
      top = fmax(top, fabs((double)s));
    }
  std::printf("c2r nz=%d rel err %.3g\n", nz, err / top);
  return err / top < 1e-13 ? 0 : 2;
}

int main() {
  int bad = 0;
  bad |= check_strided(67, -1);
  bad |= check_strided(67, +1);
  bad |= check_z(136);
  bad |= check_z(127);
  return bad;
}
