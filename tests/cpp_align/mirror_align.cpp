// Chisel::AlignFrameToModel of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on a hand-built corner: chunks
// holding sdf = min(x - x0, y - y0, z - z0) at 10 mm voxels with weight 1, the depth image rendered analytically from a
// pose looking into the corner (pixels within 6 voxels of an edge left out), the start moved by (3, -2, 2.5) mm.  Away from
// the edges the SDF is linear, so one Gauss-Newton step returns the true pose (1e-5 m, 1e-5 in every rotation entry).
// Built and run by tests/test_gpu_align.py; prints "mirror ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

int main() {
  const float res = 0.01f;
  const int W = 160, H = 120;
  const double x0[3] = {1.005, 0.845, 1.245};
  const int layer[3] = {12, 10, 15}, span = 7;
  tf_config cfg = {};
  cfg.max_chunks = 1 << 10;
  const int dims[3] = {8, 8, 8};
  chisel::Chisel map(dims, res, true, &cfg);
  tf_volume* v = map.Handle();
  chisel::tf_check(tf_set_camera(v, 131.25f, 131.25f, 79.5f, 59.5f, W, H, 0.01f, 5.f), "camera");
  std::vector<float> sdf(512), wt(512, 1.0f);
  std::vector<uint16_t> col(2048, 0);
  for (int a = 0; a < 3; ++a)
    for (int i = 0; i < span; ++i)
      for (int j = 0; j < span; ++j) {
        int32_t cid[3];
        cid[a] = layer[a]; cid[(a + 1) % 3] = layer[(a + 1) % 3] + i; cid[(a + 2) % 3] = layer[(a + 2) % 3] + j;
        for (int vi = 0; vi < 512; ++vi) {
          const int l[3] = {vi & 7, (vi >> 3) & 7, vi >> 6};
          double d = 1e9;
          for (int c = 0; c < 3; ++c) d = std::fmin(d, (cid[c] * 8 + l[c] + 0.5) * 0.01 - x0[c]);
          sdf[vi] = (float)d;
        }
        chisel::tf_check(tf_chunk_upload(v, cid, sdf.data(), wt.data(), col.data()), "upload");
      }
  // camera: forward (-1, -1, -1) / sqrt(3), 0.38 m from the corner
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0);
  const double R[9] = {-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3};  // columns: right, down, forward
  const double t[3] = {x0[0] + 0.38 * s3 + 0.01, x0[1] + 0.38 * s3 - 0.015, x0[2] + 0.38 * s3 + 0.02};
  std::vector<float> depth((size_t)W * H, 0.f);
  int lit = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double dc[3] = {(x - 79.5) / 131.0, (y - 59.5) / 131.0, 1.0};
      double d[3], best = 1e30;
      for (int r = 0; r < 3; ++r) d[r] = R[3 * r] * dc[0] + R[3 * r + 1] * dc[1] + R[3 * r + 2] * dc[2];
      for (int r = 0; r < 3; ++r)
        if (d[r] < 0) best = std::fmin(best, (x0[r] - t[r]) / d[r]);
      if (!(best > 0 && best < 1e29)) continue;
      int near_planes = 0;
      for (int r = 0; r < 3; ++r) near_planes += (t[r] + best * d[r] - x0[r]) < 6.0 * 0.01;
      if (near_planes == 1) { depth[(size_t)y * W + x] = (float)best; ++lit; }
    }
  chisel::Transform truth, start;
  const double delta[3] = {0.003, -0.002, 0.0025};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) truth(r, c) = start(r, c) = (float)R[3 * r + c];
    truth(r, 3) = (float)t[r];
    start(r, 3) = (float)(t[r] + delta[r]);
  }
  tf_align_params p;
  chisel::tf_check(tf_align_default_params(&p), "defaults");
  p.n_levels = 1; p.stride[0] = 1; p.iters[0] = 1; p.huber = 0.f; p.damping = 0.f;
  tf_align_result out;
  const int status = map.AlignFrameToModel(depth.data(), start, &p, &out);
  if (status != TF_ALIGN_MAX_ITERS || out.evaluations != 2) { std::printf("status %d, %d evaluations\n", status, out.evaluations); return 1; }
  double worst_t = 0, worst_r = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) worst_r = std::fmax(worst_r, std::fabs((double)out.pose[4 * r + c] - truth(r, c)));
    worst_t = std::fmax(worst_t, std::fabs((double)out.pose[4 * r + 3] - truth(r, 3)));
  }
  if (worst_t > 1e-5 || worst_r > 1e-5) { std::printf("pose off by %g m / %g\n", worst_t, worst_r); return 1; }
  const std::vector<tf_align_iter> log = map.AlignLog();
  if (log.size() != 2 || log[0].n_valid < lit / 2 || log[0].n_valid > lit || log[1].n_valid != log[0].n_valid) {
    std::printf("log: %zu records, %d valid of %d lit\n", log.size(), log.empty() ? -1 : log[0].n_valid, lit);
    return 1;
  }
  for (int i = 0; i < 3; ++i)
    if (std::fabs(log[0].xi[i] + delta[i]) > 1e-5 || std::fabs(log[0].xi[3 + i]) > 1e-5 || log[1].xi[i] != 0.0) {
      std::printf("step %d: %g %g\n", i, log[0].xi[i], log[0].xi[3 + i]);
      return 1;
    }
  // the defaults through the null-params form: the same fixed point
  tf_align_result out2;
  map.AlignFrameToModel(depth.data(), start, nullptr, &out2);
  for (int i = 0; i < 12; ++i)
    if (std::fabs((double)out2.pose[i] - out.pose[i]) > 1e-5) { std::printf("defaults: entry %d off\n", i); return 1; }
  std::printf("mirror ok %d valid of %d, %g m\n", log[0].n_valid, lit, worst_t);
  return 0;
}
