// tf_align_group_solve.h on its own, built with the host compiler (tests/test_align_group_cpu.py compares the output with
// a 60-digit reference; this program is also where a host sanitizer build belongs).  Prints, one line per case, f64 values
// as 16 hex digits:
//   G pose[12] xi[6] c[3] pose'[12]       a frame moved by the twist xi about the centre c (align_update_about)
//   A pose[12] xi[6] upd[12] about[12]    the anchor case, c = the pose's own t: align_update's result, then
//                                         align_update_about's
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_align_group_solve.h"

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
static void random_pose(double pose[12], bool as_f32) {
  double w[3] = {rnd(), rnd(), rnd()}, E[9];
  tf::align_rodrigues(w, E);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose[4 * i + j] = E[3 * i + j];
    pose[4 * i + 3] = 2.0 * rnd();
  }
  if (as_f32)  // as k_galign_begin hands the poses over
    for (int i = 0; i < 12; ++i) pose[i] = (double)(float)pose[i];
}

int main() {
  // steps from the size of a converged one to half a radian, about centres a few centimetres to metres away
  const double step[6] = {0.0, 1e-9, 1e-5, 1e-2, 0.1, 0.5}, reach[3] = {0.03, 0.5, 3.0};
  for (int k = 0; k < 18; ++k) {
    double pose[12], xi[6], c[3], E[9];
    random_pose(pose, k % 2 == 0);
    for (int i = 0; i < 6; ++i) xi[i] = rnd() * step[k % 6];
    for (int i = 0; i < 3; ++i) c[i] = pose[4 * i + 3] + rnd() * reach[k / 6];
    std::printf("G");
    put(pose, 12); put(xi, 6); put(c, 3);
    tf::align_rodrigues(xi + 3, E);
    tf::align_update_about(pose, E, c, xi);
    put(pose, 12);
    std::printf("\n");
  }
  for (int k = 0; k < 12; ++k) {
    double pose[12], other[12], xi[6], c[3], E[9];
    random_pose(pose, k % 2 == 0);
    for (int i = 0; i < 6; ++i) xi[i] = rnd() * step[k % 6];
    std::memcpy(other, pose, sizeof(pose));
    for (int i = 0; i < 3; ++i) c[i] = pose[4 * i + 3];
    std::printf("A");
    put(pose, 12); put(xi, 6);
    tf::align_update(pose, xi);
    put(pose, 12);
    tf::align_rodrigues(xi + 3, E);
    tf::align_update_about(other, E, c, xi);
    put(other, 12);
    std::printf("\n");
  }
  return 0;
}
