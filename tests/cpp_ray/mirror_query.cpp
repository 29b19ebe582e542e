// ChunkManager::GetSDF / GetWeight / GetSDFAndGradient of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on a
// small scene: a fronto-parallel wall integrated on the device.  Single-point calls must agree with the batched form,
// and GetSDF at a voxel centre must be the voxel downloaded with tf_chunk_download.  Built and run by
// tests/test_gpu_raycast.py; prints "mirror ok <checked>" and exits 0.
#include <cstdio>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

int main() {
  const float res = 0.005f;
  const int W = 640, H = 480;
  tf_config cfg = {};
  cfg.max_chunks = 1 << 14;
  tf_volume* v = nullptr;
  const int32_t dims[3] = {8, 8, 8};
  if (tf_volume_create(dims, res, 1, &cfg, &v) != TF_OK) { std::printf("create: %s\n", tf_last_error()); return 2; }
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

  chisel::ChunkManager cm;
  cm.Bind(v, res);
  chisel::Vec3List pts;
  for (int i = -40; i <= 40; ++i)
    for (int k = -6; k <= 6; ++k) pts.emplace_back(0.0037f * i, -0.0021f * i + 0.01f, 1.22f + 0.0025f * k);
  pts.emplace_back(50.f, 50.f, 50.f);  // absent
  std::vector<double> s, w;
  chisel::Vec3List g;
  std::vector<uint32_t> valid;
  cm.GetSDFAndGradients(pts, &s, &w, &g, &valid);
  int checked = 0, grads = 0;
  for (size_t i = 0; i < pts.size(); ++i) {
    double d1 = -7, w1 = -7;
    chisel::Vec3 g1;
    const bool a = cm.GetSDF(pts[i], &d1), b = cm.GetWeight(pts[i], &w1), c = cm.GetSDFAndGradient(pts[i], g1);
    if (a != bool(valid[i] & 1u) || b != bool(valid[i] & 2u) || c != bool(valid[i] & 4u)) {
      std::printf("validity differs at %zu\n", i);
      return 1;
    }
    if ((a && d1 != s[i]) || (b && w1 != w[i]) || (c && (g1(0) != g[i](0) || g1(1) != g[i](1) || g1(2) != g[i](2)))) {
      std::printf("value differs at %zu\n", i);
      return 1;
    }
    grads += c;
    ++checked;
  }
  if (valid.back() != 0u || grads < 100) { std::printf("absent point valid / too few gradients (%d)\n", grads); return 1; }
  // voxel centres against the downloaded chunk
  const int32_t cid[3] = {0, 0, 30};
  std::vector<float> sdf(512), wt(512);
  std::vector<uint16_t> col(2048);
  chisel::tf_check(tf_chunk_download(v, cid, sdf.data(), wt.data(), col.data()), "download");
  for (int vi = 0; vi < 512; ++vi) {
    const int x = vi & 7, y = (vi >> 3) & 7, z = vi >> 6;
    const chisel::Vec3 p((x + 0.5f) * res, (y + 0.5f) * res, (240 + z + 0.5f) * res);
    double d = 0, ww = 0;
    const bool ok = cm.GetSDF(p, &d);
    if (!cm.GetWeight(p, &ww) || ww != wt[vi] || ok != (wt[vi] > 1e-12) || (ok && d != sdf[vi])) {
      std::printf("voxel %d differs\n", vi);
      return 1;
    }
    ++checked;
  }
  tf_volume_destroy(v);
  std::printf("mirror ok %d\n", checked);
  return 0;
}
