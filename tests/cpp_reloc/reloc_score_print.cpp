// The relocalisation score of tf_reloc_score.h on the host: reads lines of
//   sum_d2 sum_d sum_z2 m n bw bh grey_weight depth_weight min_overlap
// from standard input and prints the bits of s_grey and of the score, one line each.  tests/test_reloc_cpu.py compares
// them with the restatement's (tests/reloc_ref.py) bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_reloc_score.h"

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

int main() {
  uint64_t sd2, sz2;
  int64_t sd;
  uint32_t m, n, bw, bh;
  float gw, dw;
  int32_t mo;
  while (std::scanf("%" SCNu64 " %" SCNd64 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %f %f %" SCNd32, &sd2, &sd,
                    &sz2, &m, &n, &bw, &bh, &gw, &dw, &mo) == 10)
    std::printf("%016" PRIx64 " %016" PRIx64 "\n", bits(tf::reloc_grey_score(sd2, sd, n, bw, bh)),
                bits(tf::reloc_score(sd2, sd, sz2, m, n, bw, bh, gw, dw, mo)));
  return 0;
}
