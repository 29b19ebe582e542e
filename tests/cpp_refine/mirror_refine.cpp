// Chisel::GetDistanceFromSurface / GetDistancesFromSurface / RefineFrameInVoxel of the host mirror
// (texturefusion_amd/host/tf_chisel.hpp) on a fronto-parallel wall integrated on the device: the mirror's results must
// equal the C ABI's bit for bit.  Built and run by tests/test_gpu_refine.py; prints "mirror ok <checked>" and exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main() {
  const float res = 0.005f;
  const int W = 640, H = 480;
  tf_config cfg = {};
  cfg.max_chunks = 1 << 14;
  const int chunkSize[3] = {8, 8, 8};
  chisel::Chisel ch(chunkSize, res, true, &cfg);
  tf_volume* v = ch.Handle();
  chisel::tf_check(tf_set_camera(v, 525.f, 525.f, 319.5f, 239.5f, W, H, 0.01f, 5.f), "camera");
  std::vector<float> depth((size_t)W * H, 1.22f);
  std::vector<uint8_t> rgba((size_t)W * H * 4);
  for (size_t i = 0; i < (size_t)W * H; ++i) {
    if (i % 53 == 0) depth[i] = 0.f;
    rgba[4 * i] = 200; rgba[4 * i + 1] = 100; rgba[4 * i + 2] = 50; rgba[4 * i + 3] = 1;
  }
  const float pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  chisel::tf_check(tf_integrate_frame_host(v, depth.data(), rgba.data(), pose, nullptr, 0), "integrate");
  chisel::tf_check(tf_sync(v), "sync");

  // point distances: single calls and the batched form against the ABI
  chisel::Vec3List pts;
  for (int i = -40; i <= 40; ++i)
    for (int k = -6; k <= 6; ++k) pts.emplace_back(0.0037f * i, -0.0021f * i + 0.01f, 1.22f + 0.0025f * k);
  pts.emplace_back(50.f, 50.f, 50.f);  // absent
  std::vector<float> xyz, d_abi(pts.size()), w_abi(pts.size()), d_b, w_b;
  for (const auto& p : pts) { xyz.push_back(p(0)); xyz.push_back(p(1)); xyz.push_back(p(2)); }
  chisel::tf_check(tf_distance_from_surface(v, xyz.data(), (int64_t)pts.size(), d_abi.data(), w_abi.data()), "abi");
  ch.GetDistancesFromSurface(pts, &d_b, &w_b);
  int checked = 0, weighted = 0;
  for (size_t i = 0; i < pts.size(); ++i) {
    float tw = -7.f;
    const float d = ch.GetDistanceFromSurface(pts[i], tw);
    if (!same(d, d_abi[i]) || !same(tw, w_abi[i]) || !same(d_b[i], d_abi[i]) || !same(w_b[i], w_abi[i])) {
      std::printf("distance differs at %zu\n", i);
      return 1;
    }
    weighted += w_abi[i] > 0.f;
    ++checked;
  }
  if (w_abi.back() != 0.f || d_abi.back() != 0.f || weighted < 100) {
    std::printf("absent point weighted / too few weighted points (%d)\n", weighted);
    return 1;
  }

  // RefineFrameInVoxel on a noisy copy of the depth against tf_refine_frame_in_voxel
  std::vector<float> noisy(depth), ref_d, ref_w((size_t)W * H, -7.f), m_w((size_t)W * H, -7.f);
  for (size_t i = 0; i < noisy.size(); ++i)
    if (noisy[i] > 0.f) noisy[i] += 0.003f * (float)((int)(i * 2654435761u % 2001u) - 1000) / 1000.f;
  ref_d = noisy;
  chisel::tf_check(tf_refine_frame_in_voxel(v, ref_d.data(), ref_w.data(), pose), "abi refine");
  chisel::ProjectionIntegrator integ;
  chisel::PinholeCamera cam;  // 525 / 319.5 / 640 x 480 / 0.01 .. 5, as above
  chisel::Transform T;
  std::vector<float> m_d(noisy);
  ch.RefineFrameInVoxel(integ, m_d.data(), m_w.data(), T, cam);
  int accepted = 0;
  for (size_t i = 0; i < m_d.size(); ++i) {
    if (!same(m_d[i], ref_d[i]) || !same(m_w[i], ref_w[i])) { std::printf("refine differs at %zu\n", i); return 1; }
    accepted += m_w[i] > 0.f;
    ++checked;
  }
  if (accepted < W * H / 2) { std::printf("too few accepted pixels (%d)\n", accepted); return 1; }
  std::printf("mirror ok %d\n", checked);
  return 0;
}
