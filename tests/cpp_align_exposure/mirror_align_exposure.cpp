// Chisel::SetAlignExposure of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on the hand-built textured plane of
// tests/cpp_align_color/mirror_align_color.cpp, seen by a camera at another exposure: every colour channel of the frame is
// rint(0.8 v + 255 * 0.06).  Without the setting AlignFrameToModelColor ends millimetres from the true pose; with it the
// call ends within 2.1e-4 m (twice the offset tests/test_align_color_cpu.py measures for this scene) and the estimate lies
// within twice the deviation tests/align_exposure_inputs.py records of the pair predicted from the unmodified frame's.
// Built and run by tests/test_gpu_align_exposure.py; prints "mirror ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../texturefusion_amd/host/tf_chisel.hpp"

static double intensity(double y, double z) {
  const double pi = 3.14159265358979323846;
  return 128.0 + 55.0 * std::sin(2.0 * pi * y / 0.17 + 0.3) * std::cos(2.0 * pi * z / 0.23) +
         45.0 * std::sin(2.0 * pi * (y + z) / 0.31 + 1.0);
}

static void worst(const tf_align_color_result& out, const chisel::Transform& truth, double* wt, double* wr) {
  *wt = *wr = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) *wr = std::fmax(*wr, std::fabs((double)out.geo.pose[4 * r + c] - truth(r, c)));
    *wt = std::fmax(*wt, std::fabs((double)out.geo.pose[4 * r + 3] - truth(r, 3)));
  }
}

int main() {
  const float res = 0.01f;
  const int W = 160, H = 120;
  const double x0[3] = {1.005, 0.845, 1.245};
  const int layer[3] = {12, 10, 15}, span = 7;
  const double gain = 0.8, offset = 0.06;
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
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0);
  const double R[9] = {-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3};  // columns: right, down, forward
  const double t[3] = {x0[0] + 0.38 * s3 + 0.01, x0[1] + 0.38 * s3 - 0.015, x0[2] + 0.38 * s3 + 0.02};
  std::vector<float> depth((size_t)W * H, 0.f);
  std::vector<uint8_t> rgba((size_t)W * H * 4, 0);
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
      const double g = std::rint(intensity(t[1] + s * d[1], t[2] + s * d[2]));
      rgba[4 * o] = rgba[4 * o + 1] = rgba[4 * o + 2] = (uint8_t)std::lrint(gain * g + 255.0 * offset);
      rgba[4 * o + 3] = 1;
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
  tf_align_color_result off, on, again;
  double wt_off, wr_off, wt_on, wr_on, g = 0, o = 0;
  tf_align_exposure e;
  if (map.GetAlignExposure(&e)) { std::printf("the setting is on in a new map\n"); return 1; }
  map.AlignFrameToModelColor(depth.data(), rgba.data(), start, &p, &off);
  worst(off, truth, &wt_off, &wr_off);
  if (map.AlignExposureEstimate(0, &g, &o) || !map.AlignExposureLog(0).empty()) { std::printf("an estimate without the setting\n"); return 1; }
  map.SetAlignExposure();
  if (!map.GetAlignExposure(&e) || e.unknowns != 2 || e.carry != 0 || e.gain0 != 1.0f || e.offset0 != 0.0f) {
    std::printf("GetAlignExposure\n");
    return 1;
  }
  const int status = map.AlignFrameToModelColor(depth.data(), rgba.data(), start, &p, &on);
  worst(on, truth, &wt_on, &wr_on);
  if (status != TF_ALIGN_MAX_ITERS || on.geo.evaluations != 11 || !map.AlignExposureEstimate(0, &g, &o)) {
    std::printf("status %d, %d evaluations\n", status, on.geo.evaluations);
    return 1;
  }
  const std::vector<tf_align_exposure_iter> log = map.AlignExposureLog(0);
  if (log.size() != 11 || map.AlignColorLog().size() != 11 || log[0].gain != 1.0 || log[0].offset != 0.0 || log[10].rank != 2 ||
      log[10].gain != g || log[10].offset != o || log[10].n_photo != on.n_photo_last) {
    std::printf("log: %zu records\n", log.size());
    return 1;
  }
  // predicted from the unmodified frame's estimate (0.988436, 0.005818): (g_id / gain, o_id - g_id * offset / gain)
  const double pg = 0.988436 / gain, po = 0.005818 - 0.988436 * offset / gain;
  if (wt_off < 1e-3 || wt_on > 2.1e-4 || wr_on > 7.4e-4 || std::fabs(g - pg) > 2 * 2.0e-3 || std::fabs(o - po) > 2 * 1.2e-3) {
    std::printf("off %g m, on %g m / %g, estimate %g %g (predicted %g %g)\n", wt_off, wt_on, wr_on, g, o, pg, po);
    return 1;
  }
  map.ClearAlignExposure();
  map.AlignFrameToModelColor(depth.data(), rgba.data(), start, &p, &again);
  for (int i = 0; i < 12; ++i)
    if (again.geo.pose[i] != off.geo.pose[i]) { std::printf("cleared: entry %d differs\n", i); return 1; }
  std::printf("mirror ok off %g m, on %g m, gain %g offset %g\n", wt_off, wt_on, g, o);
  return 0;
}
