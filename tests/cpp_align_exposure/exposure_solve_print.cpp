// tf_align_exposure_solve.h on its own, built with the host compiler (tests/test_align_exposure_cpu.py compares the output
// with the restatement bit for bit; this program is also where a host sanitizer build belongs).  One line per case, f64
// values as 16 hex digits:
//   E <unknowns> <rank> min_gain max_gain pair[2] S[17] Ac[21] bc[6] xi[6] Ac'[21] bc'[6] de[2] pair'[2]
// The sums are those of seeded random pixels (wJc[6], wc, Lf, rc), so that F is a Gram matrix as on the device; then the
// special cases: a constant Lf (the second pivot fails), no pixel at all, and a step that runs into the clamp at either end.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_align_exposure_solve.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {  // xorshift64*, uniform in [-1, 1)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 4503599627370496.0 - 1.0;
}
static void put(const double* v, int n) {
  for (int i = 0; i < n; ++i) {
    uint64_t u;
    std::memcpy(&u, v + i, 8);
    std::printf(" %016llx", (unsigned long long)u);
  }
}

// the sums of n pixels; spread 0: every pixel has the same Lf
static void pixels(int n, double spread, double rc_scale, double S[17], double Ac[21], double bc[6]) {
  for (int i = 0; i < 17; ++i) S[i] = 0.0;
  for (int i = 0; i < 21; ++i) Ac[i] = 0.0;
  for (int i = 0; i < 6; ++i) bc[i] = 0.0;
  for (int k = 0; k < n; ++k) {
    double J[6];
    const double w = 0.55 + 0.45 * rnd(), lf = 0.5 + 0.4 * spread * rnd(), rc = rc_scale * rnd() + 0.1 * (lf - 0.5) - 0.03;
    for (int i = 0; i < 6; ++i) J[i] = rnd() * (i < 3 ? 4.0 : 1.5);
    for (int i = 0; i < 6; ++i) {
      for (int j = i; j < 6; ++j) Ac[tf::align_upper(i, j)] += w * J[i] * J[j];
      bc[i] += w * J[i] * rc;
      S[tf::kExpP + i] += w * J[i];
      S[tf::kExpQ + i] += w * J[i] * lf;
    }
    S[tf::kExpSw] += w; S[tf::kExpSl] += w * lf; S[tf::kExpSll] += w * lf * lf;
    S[tf::kExpSr] += w * rc; S[tf::kExpSlr] += w * lf * rc;
  }
}

static void run_case(int unknowns, double min_gain, double max_gain, double gain, double offset, const double S[17],
                     const double Ac_in[21], const double bc_in[6], double xi_scale) {
  double Ac[21], bc[6], xi[6], de[2], pair[2] = {gain, offset};
  for (int i = 0; i < 21; ++i) Ac[i] = Ac_in[i];
  for (int i = 0; i < 6; ++i) { bc[i] = bc_in[i]; xi[i] = xi_scale * rnd(); }
  tf::ExposureElim el;
  tf::exposure_eliminate(S, unknowns, Ac, bc, &el);
  std::printf("E %d %d", unknowns, el.rank);
  put(&min_gain, 1); put(&max_gain, 1); put(pair, 2); put(S, 17); put(Ac_in, 21); put(bc_in, 6); put(xi, 6);
  tf::exposure_step(S, el, xi, de);
  tf::exposure_apply(pair, el.rank, de, min_gain, max_gain);
  put(Ac, 21); put(bc, 6); put(de, 2); put(pair, 2);
  std::printf("\n");
}

int main() {
  double S[17], Ac[21], bc[6];
  for (int k = 0; k < 36; ++k) {
    pixels(8 + 5 * k, 1.0, k % 2 ? 0.05 : 0.3, S, Ac, bc);
    run_case(k % 3, 0.25, 4.0, 1.0 + 0.2 * rnd(), 0.05 * rnd(), S, Ac, bc, k % 4 ? 1e-2 : 0.3);
  }
  for (int u = 0; u < 3; ++u) {  // a constant Lf: rank 1 at the most; no pixel: rank 0
    pixels(40, 0.0, 0.1, S, Ac, bc);
    run_case(u, 0.25, 4.0, 1.1, -0.02, S, Ac, bc, 1e-2);
    pixels(0, 1.0, 0.1, S, Ac, bc);
    run_case(u, 0.25, 4.0, 0.9, 0.03, S, Ac, bc, 1e-2);
  }
  // the clamp at either end: the residuals ask for a gain far from the start
  pixels(60, 1.0, 0.02, S, Ac, bc);
  run_case(2, 0.98, 1.02, 1.0, 0.0, S, Ac, bc, 1e-3);
  for (int i = 0; i < 6; ++i) S[tf::kExpQ + i] = -S[tf::kExpQ + i];
  S[tf::kExpSlr] = -S[tf::kExpSlr] + 5.0;
  run_case(2, 0.98, 1.02, 1.0, 0.0, S, Ac, bc, 1e-3);
  S[tf::kExpSlr] = S[tf::kExpSlr] - 10.0;
  run_case(2, 0.98, 1.02, 1.0, 0.0, S, Ac, bc, 1e-3);
  return 0;
}
