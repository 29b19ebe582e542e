// Stand-alone host program around texturefusion_amd/csrc/tf_cc_solve.h (the solve tf_compensate_color runs on the host and
// k_ccd_combine on the device): prints, per covariance pair of a fixed set, cov_src[9] cov_tar[9] T[9] as the 27 f32 bit
// patterns in hex, one pair per line.  tests/test_cc_device_cpu.py feeds the printed inputs to the oracle and compares T.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../texturefusion_amd/csrc/tf_cc_solve.h"

namespace {

struct Pair { float cs[9], ct[9]; };

uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform() {  // (-1, 1), 53 bits of a 64-bit LCG
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 4503599627370496.0 - 1.0;
}
void gram(float out[9], double scale) {  // M M^T * scale: symmetric positive definite (almost surely)
  double M[9];
  for (double& m : M) m = uniform();
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) out[3 * i + j] = (float)((M[3 * i] * M[3 * j] + M[3 * i + 1] * M[3 * j + 1] + M[3 * i + 2] * M[3 * j + 2]) * scale);
}
void diag(float out[9], float a, float b, float c) {
  for (int i = 0; i < 9; i++) out[i] = 0.0f;
  out[0] = a; out[4] = b; out[8] = c;
}
void print(const Pair& p, const float T[9]) {
  const float* rows[3] = {p.cs, p.ct, T};
  for (const float* r : rows)
    for (int i = 0; i < 9; i++) {
      uint32_t u;
      std::memcpy(&u, &r[i], 4);
      std::printf("%08x ", u);
    }
  std::printf("\n");
}

}  // namespace

int main() {
  std::vector<Pair> set;
  Pair p;
  diag(p.cs, 1.0f, 1.0f, 1.0f); diag(p.ct, 1.0f, 1.0f, 1.0f); set.push_back(p);             // the identity
  diag(p.cs, 0.04f, 0.09f, 0.01f); diag(p.ct, 0.02f, 0.05f, 0.03f); set.push_back(p);       // a diagonal pair
  {  // a rank-1 source (two zero eigenvalues: the + 1e-2 guard), a full-rank target
    const float v[3] = {0.3f, 0.2f, 0.1f};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) p.cs[3 * i + j] = v[i] * v[j];
    gram(p.ct, 0.05);
    set.push_back(p);
  }
  for (int k = 0; k < 64; k++) {  // random symmetric positive definite pairs, colour-sized and small
    const double scale = k % 4 == 3 ? 1e-4 : 0.05;
    gram(p.cs, scale); gram(p.ct, scale);
    set.push_back(p);
  }
  for (const Pair& q : set) {
    float T[9];
    tf::color_transfer(q.cs, q.ct, T);
    print(q, T);
  }
  return 0;
}
