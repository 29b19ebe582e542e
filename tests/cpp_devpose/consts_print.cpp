// make_select_consts (texturefusion_amd/csrc/tf_host_math.h) on its own, built with the host compiler: what the library's
// launchers compute on the host and k_pose_consts restates on the device (tests/test_devpose_cpu.py compares the output with
// tests/pose_consts_ref.py; this program is also where a host sanitizer build belongs).  Reads cases from standard input,
// one per line: res and pose[12] as 8 hex digits each (f32 bit patterns).  Prints one line per case, 8 hex digits per word:
//   step  rot[9] tc[3] r0[3] r1[3] r2[3] coarse[24] fine[24] pose[12]
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_host_math.h"

static void put(const float* v, int n) {
  for (int i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, v + i, 4);
    std::printf(" %08x", u);
  }
}

int main() {
  unsigned w[13];
  while (std::scanf("%x %x %x %x %x %x %x %x %x %x %x %x %x", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8],
                    &w[9], &w[10], &w[11], &w[12]) == 13) {
    float f[13];
    for (int i = 0; i < 13; ++i) {
      const uint32_t u = w[i];
      std::memcpy(&f[i], &u, 4);
    }
    const tf::SelectConsts sc = tf::make_select_consts(f + 1, f[0]);
    std::printf("%d", sc.step);
    put(&sc.rot[0][0], 9); put(sc.tc, 3); put(sc.r0, 3); put(sc.r1, 3); put(sc.r2, 3);
    put(&sc.coarse[0][0], 24); put(&sc.fine[0][0], 24); put(sc.pose, 12);
    std::printf("\n");
  }
  return 0;
}
