// devpose_inverse16 (texturefusion_amd/csrc/tf_devpose.h) on its own, as the host runs it: the matrix a frame tracked on the
// device is textured with, which k_pose_consts computes on the device by the same text (tests/test_devpose_textured_cpu.py
// compares the output with tests/pose_inverse_ref.py; this program is also where a host sanitizer build belongs).  The
// header names device intrinsics next to the function, so the program is built with the HIP compiler, host side only; it
// makes no HIP call and needs no GPU.  Reads cases from standard input, one per line: pose[12] as 8 hex digits each (f32
// bit patterns).  Prints one line per case: T[16], 8 hex digits per word.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../texturefusion_amd/csrc/tf_devpose.h"

int main() {
  unsigned w[12];
  while (std::scanf("%x %x %x %x %x %x %x %x %x %x %x %x", &w[0], &w[1], &w[2], &w[3], &w[4], &w[5], &w[6], &w[7], &w[8], &w[9],
                    &w[10], &w[11]) == 12) {
    float pose[12], T[16];
    for (int i = 0; i < 12; ++i) {
      const uint32_t u = w[i];
      std::memcpy(&pose[i], &u, 4);
    }
    tf::devpose_inverse16(pose, T);
    for (int i = 0; i < 16; ++i) {
      uint32_t u;
      std::memcpy(&u, &T[i], 4);
      std::printf(i ? " %08x" : "%08x", u);
    }
    std::printf("\n");
  }
  return 0;
}
