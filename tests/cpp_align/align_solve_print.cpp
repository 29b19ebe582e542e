// tf_align_solve.h on its own, built with the host compiler (tests/test_align_cpu.py compares the output with numpy; this
// program is also where a host sanitizer build belongs).  Prints, one line per case, f64 values as 16 hex digits:
//   S <ok> A[21] b[6] damping xi[6]      a 6 x 6 system: seeded random SPD ones, then printed special cases
//   R w[3] E[9]                          exp([w]x)
//   U pose[12] xi[6] pose'[12]           a pose update
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_align_solve.h"

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
static void solve_case(const double A[21], const double b[6], double damping) {
  double xi[6];
  const bool ok = tf::align_solve6(A, b, damping, xi);
  std::printf("S %d", ok ? 1 : 0);
  put(A, 21); put(b, 6); put(&damping, 1); put(xi, 6);
  std::printf("\n");
}
// A = G^T G (+ shift on the diagonal) from an m x 6 matrix of random rows scaled per column
static void gram(int m, const double scale[6], double shift, double A[21]) {
  for (int i = 0; i < 21; ++i) A[i] = 0.0;
  for (int r = 0; r < m; ++r) {
    double g[6];
    for (int i = 0; i < 6; ++i) g[i] = rnd() * scale[i];
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j) A[tf::align_upper(i, j)] += g[i] * g[j];
  }
  for (int i = 0; i < 6; ++i) A[tf::align_upper(i, i)] += shift;
}

int main() {
  const double one[6] = {1, 1, 1, 1, 1, 1}, mixed[6] = {1, 1, 1, 1.7, 0.4, 2.5}, wide[6] = {1e3, 1, 1e-2, 30, 1e-1, 5};
  double A[21], b[6];
  for (int k = 0; k < 48; ++k) {
    gram(6 + k, k % 3 == 0 ? one : (k % 3 == 1 ? mixed : wide), 0.0, A);
    for (int i = 0; i < 6; ++i) b[i] = rnd() * (k % 2 ? 1e-3 : 10.0);
    solve_case(A, b, k % 4 == 0 ? 0.0 : (k % 4 == 1 ? 1e-6 : (k % 4 == 2 ? 1e-2 : 1.0)));
  }
  // identity, a diagonal matrix, rank 3 (a plane alone: three free directions), rank 5, all zero, a negative diagonal
  for (int i = 0; i < 21; ++i) A[i] = 0.0;
  for (int i = 0; i < 6; ++i) { A[tf::align_upper(i, i)] = 1.0; b[i] = i + 1.0; }
  solve_case(A, b, 0.0);
  for (int i = 0; i < 6; ++i) A[tf::align_upper(i, i)] = 1.0 + 3.0 * i;
  solve_case(A, b, 0.5);
  gram(3, one, 0.0, A);
  solve_case(A, b, 0.0);
  solve_case(A, b, 1e-3);
  gram(5, mixed, 0.0, A);
  solve_case(A, b, 0.0);
  for (int i = 0; i < 21; ++i) A[i] = 0.0;
  solve_case(A, b, 0.0);
  for (int i = 0; i < 6; ++i) A[tf::align_upper(i, i)] = 1.0;
  A[tf::align_upper(4, 4)] = -1.0;
  solve_case(A, b, 0.0);
  const double th[6] = {0.0, 1e-12, 1e-8, 1e-3, 1.0, 3.14159265358979323846 - 1e-6};
  const double ax[3][3] = {{1, 0, 0}, {0.6, -0.64, 0.48}, {-0.36, 0.48, 0.8}};
  for (int a = 0; a < 3; ++a)
    for (int t = 0; t < 6; ++t) {
      double w[3], E[9];
      for (int i = 0; i < 3; ++i) w[i] = ax[a][i] * th[t];
      tf::align_rodrigues(w, E);
      std::printf("R");
      put(w, 3); put(E, 9);
      std::printf("\n");
    }
  for (int k = 0; k < 6; ++k) {
    double w[3] = {rnd(), rnd(), rnd()}, pose[12], E[9], xi[6];
    tf::align_rodrigues(w, E);
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose[4 * i + j] = E[3 * i + j];
      pose[4 * i + 3] = 2.0 * rnd();
    }
    for (int i = 0; i < 6; ++i) xi[i] = rnd() * (k < 3 ? 1e-2 : 0.5);
    std::printf("U");
    put(pose, 12); put(xi, 6);
    tf::align_update(pose, xi);
    put(pose, 12);
    std::printf("\n");
  }
  return 0;
}
