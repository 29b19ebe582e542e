// Chisel::AlignFrameToModelColor of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on a hand-built textured plane:
// chunks holding sdf = x - x0 at 10 mm voxels with weight 1 and the colour word (v, v, v, 100), v = rint(100 * intensity at
// the voxel's centre); the depth and colour images rendered analytically from a pose looking at the plane obliquely; the
// start moved by (0, 15, 12) mm inside the plane.  AlignFrameToModel alone is TF_ALIGN_SINGULAR there; with colour the call
// ends within 2.1e-4 m of the true pose (twice the offset tests/test_align_color_cpu.py measures for this scene:
// the trilinear field's smoothing of the texture and the u8 rounding of the frame).
// Built and run by tests/test_gpu_align_color.py; prints "mirror ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

static double intensity(double y, double z) {
  const double pi = 3.14159265358979323846;
  return 128.0 + 55.0 * std::sin(2.0 * pi * y / 0.17 + 0.3) * std::cos(2.0 * pi * z / 0.23) +
         45.0 * std::sin(2.0 * pi * (y + z) / 0.31 + 1.0);
}

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
  for (int i = 0; i < span; ++i)
    for (int j = 0; j < span; ++j) {
      const int32_t cid[3] = {layer[0], layer[1] + i, layer[2] + j};
      for (int vi = 0; vi < 512; ++vi) {
        const int l[3] = {vi & 7, (vi >> 3) & 7, vi >> 6};
        double c[3];
        for (int a = 0; a < 3; ++a) c[a] = (cid[a] * 8 + l[a] + 0.5) * 0.01;
        sdf[vi] = (float)(c[0] - x0[0]);
        const uint16_t g = (uint16_t)std::lrint(100.0 * intensity(c[1], c[2]));
        col[4 * vi] = col[4 * vi + 1] = col[4 * vi + 2] = g;
        col[4 * vi + 3] = 100;
      }
      chisel::tf_check(tf_chunk_upload(v, cid, sdf.data(), wt.data(), col.data()), "upload");
    }
  // camera: forward (-1, -1, -1) / sqrt(3), 0.38 m from the corner point x0
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0);
  const double R[9] = {-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3};  // columns: right, down, forward
  const double t[3] = {x0[0] + 0.38 * s3 + 0.01, x0[1] + 0.38 * s3 - 0.015, x0[2] + 0.38 * s3 + 0.02};
  std::vector<float> depth((size_t)W * H, 0.f);
  std::vector<uint8_t> rgba((size_t)W * H * 4, 0);
  int lit = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double dc[3] = {(x - 79.5) / 131.0, (y - 59.5) / 131.0, 1.0};
      double d[3];
      for (int r = 0; r < 3; ++r) d[r] = R[3 * r] * dc[0] + R[3 * r + 1] * dc[1] + R[3 * r + 2] * dc[2];
      if (!(d[0] < 0)) continue;
      const double s = (x0[0] - t[0]) / d[0];
      if (!(s > 0)) continue;
      const size_t o = (size_t)y * W + x;
      depth[o] = (float)s;
      const uint8_t g = (uint8_t)std::lrint(intensity(t[1] + s * d[1], t[2] + s * d[2]));
      rgba[4 * o] = rgba[4 * o + 1] = rgba[4 * o + 2] = g;
      rgba[4 * o + 3] = 1;
      ++lit;
    }
  chisel::Transform truth, start;
  const double delta[3] = {0.0, 0.015, 0.012};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) truth(r, c) = start(r, c) = (float)R[3 * r + c];
    truth(r, 3) = (float)t[r];
    start(r, 3) = (float)(t[r] + delta[r]);
  }
  tf_align_color_params p;
  chisel::tf_check(tf_align_color_default_params(&p), "defaults");
  p.geo.n_levels = 2; p.geo.stride[0] = 2; p.geo.iters[0] = 4; p.geo.stride[1] = 1; p.geo.iters[1] = 6;
  p.geo.eps_t = 0.f; p.geo.eps_r = 0.f;
  tf_align_result geo;
  if (map.AlignFrameToModel(depth.data(), start, &p.geo, &geo) != TF_ALIGN_SINGULAR) {
    std::printf("geometric alone: status %d\n", geo.status);
    return 1;
  }
  tf_align_color_result out;
  const int status = map.AlignFrameToModelColor(depth.data(), rgba.data(), start, &p, &out);
  if (status != TF_ALIGN_MAX_ITERS || out.geo.evaluations != 11) {
    std::printf("status %d, %d evaluations\n", status, out.geo.evaluations);
    return 1;
  }
  double worst_t = 0, worst_r = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) worst_r = std::fmax(worst_r, std::fabs((double)out.geo.pose[4 * r + c] - truth(r, c)));
    worst_t = std::fmax(worst_t, std::fabs((double)out.geo.pose[4 * r + 3] - truth(r, 3)));
  }
  if (worst_t > 2.1e-4 || worst_r > 7.4e-4) { std::printf("pose off by %g m / %g\n", worst_t, worst_r); return 1; }
  const std::vector<tf_align_color_iter> log = map.AlignColorLog();
  if (log.size() != 11 || log[10].geo.n_valid < 1000 || log[10].geo.n_valid > lit || log[10].n_photo != log[10].geo.n_valid ||
      out.n_photo_last != log[10].n_photo || !(out.rms_photo_last < out.rms_photo_first)) {
    std::printf("log: %zu records, %d photometric of %d valid of %d lit\n", log.size(), log.empty() ? -1 : log.back().n_photo,
                log.empty() ? -1 : log.back().geo.n_valid, lit);
    return 1;
  }
  // the geometric log is still the geometric call's: one record, the singular one
  if (map.AlignLog().size() != 1) { std::printf("AlignLog changed\n"); return 1; }
  // the defaults through the null-params form: the same pose to within their early stop
  tf_align_color_result out2;
  map.AlignFrameToModelColor(depth.data(), rgba.data(), start, nullptr, &out2);
  for (int i = 0; i < 12; ++i)
    if (std::fabs((double)out2.geo.pose[i] - out.geo.pose[i]) > 1e-4) { std::printf("defaults: entry %d off\n", i); return 1; }
  std::printf("mirror ok %d photometric of %d lit, %g m\n", log[10].n_photo, lit, worst_t);
  return 0;
}
