// Chisel::AlignFrameToModelICP, AlignIcpLog and TrackFrame of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on the
// hand-built corner of tests/cpp_align/mirror_align.cpp: one frame rendered analytically at its true pose, started 80 mm
// and 5 degrees away.  AlignFrameToModel finds no valid pixel from there (TF_ALIGN_TOO_FEW); the projective ICP against
// the model raycast at the start lands within 2 mm (a fifth of a voxel: the raycast surface of the trilinear SDF is that
// good away from the edges, and the SDF stage's basin is ten times wider), and TrackFrame ends in stage 2 within 1e-4 m of
// the true pose.  Built and run by tests/test_gpu_align_icp.py; prints "mirror ok" and exits 0.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../texturefusion_amd/csrc/tf_align_solve.h"
#include "../../texturefusion_amd/host/tf_chisel.hpp"

static const int W = 160, H = 120;
static const double x0[3] = {1.005, 0.845, 1.245};

struct Pose { double R[9], t[3]; };

// pose turned about its camera centre by the rotation vector w (world) and moved by dt
static Pose perturb(const Pose& p, const double dt[3], const double w[3]) {
  double E[9];
  tf::align_rodrigues(w, E);
  Pose q;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) q.R[3 * i + j] = E[3 * i] * p.R[j] + E[3 * i + 1] * p.R[3 + j] + E[3 * i + 2] * p.R[6 + j];
    q.t[i] = p.t[i] + dt[i];
  }
  return q;
}

// z-depth of the corner from p, pixels within 6 voxels of an edge left out
static int render(const Pose& p, std::vector<float>& depth) {
  depth.assign((size_t)W * H, 0.f);
  int lit = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double dc[3] = {(x - 79.5) / 131.0, (y - 59.5) / 131.0, 1.0};
      double d[3], best = 1e30;
      for (int r = 0; r < 3; ++r) d[r] = p.R[3 * r] * dc[0] + p.R[3 * r + 1] * dc[1] + p.R[3 * r + 2] * dc[2];
      for (int r = 0; r < 3; ++r)
        if (d[r] < 0 && (x0[r] - p.t[r]) / d[r] < best) best = (x0[r] - p.t[r]) / d[r];
      if (!(best > 0 && best < 1e29)) continue;
      int near_planes = 0;
      for (int r = 0; r < 3; ++r) near_planes += (p.t[r] + best * d[r] - x0[r]) < 6.0 * 0.01;
      if (near_planes == 1) { depth[(size_t)y * W + x] = (float)best; ++lit; }
    }
  return lit;
}

static chisel::Transform as_transform(const Pose& p) {
  chisel::Transform T;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T(r, c) = (float)p.R[3 * r + c];
    T(r, 3) = (float)p.t[r];
  }
  return T;
}

static bool near_truth(const float* pose, const chisel::Transform& truth, double tol, const char* what) {
  double worst_t = 0, worst_r = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) worst_r = std::fmax(worst_r, std::fabs((double)pose[4 * r + c] - truth(r, c)));
    worst_t = std::fmax(worst_t, std::fabs((double)pose[4 * r + 3] - truth(r, 3)));
  }
  std::printf("%s: %g m / %g from the true pose\n", what, worst_t, worst_r);
  return worst_t <= tol && worst_r <= tol;
}

int main() {
  const float res = 0.01f;
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
  // forward (-1, -1, -1) / sqrt(3), 0.38 m from the corner; the start 80 mm and 5 degrees away
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0), deg = 3.14159265358979323846 / 180.0;
  const Pose T = {{-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3},
                  {x0[0] + 0.38 * s3 + 0.01, x0[1] + 0.38 * s3 - 0.015, x0[2] + 0.38 * s3 + 0.02}};
  const double dir_t[3] = {0.6, 0.53, 0.6}, dir_r[3] = {0.6, -0.64, 0.48};
  const double nt = std::sqrt(dir_t[0] * dir_t[0] + dir_t[1] * dir_t[1] + dir_t[2] * dir_t[2]);
  const double nr = std::sqrt(dir_r[0] * dir_r[0] + dir_r[1] * dir_r[1] + dir_r[2] * dir_r[2]);
  double dt[3], w[3];
  for (int i = 0; i < 3; ++i) { dt[i] = 0.080 * dir_t[i] / nt; w[i] = 5.0 * deg * dir_r[i] / nr; }
  std::vector<float> depth;
  const int lit = render(T, depth);
  const chisel::Transform truth = as_transform(T), start = as_transform(perturb(T, dt, w));

  tf_align_result alone;
  if (map.AlignFrameToModel(depth.data(), start, nullptr, &alone) != TF_ALIGN_TOO_FEW || alone.n_valid_first != 0) {
    std::printf("the SDF alignment from the far start: status %d, %d valid\n", alone.status, alone.n_valid_first);
    return 1;
  }
  const size_t sdf_records = map.AlignLog().size();
  tf_align_result icp;
  const int status = map.AlignFrameToModelICP(depth.data(), start, nullptr, nullptr, &icp);
  const std::vector<tf_align_iter> log = map.AlignIcpLog();
  if (status > TF_ALIGN_MAX_ITERS || (int)log.size() != icp.evaluations || log.size() < 4 || log.back().n_valid != icp.n_valid_last ||
      icp.n_valid_last < lit * 9 / 10 || icp.n_valid_last > lit || map.AlignLog().size() != sdf_records) {
    std::printf("icp: status %d, %d evaluations, %zu records, %d valid of %d lit\n", status, icp.evaluations, log.size(),
                icp.n_valid_last, lit);
    return 1;
  }
  if (!near_truth(icp.pose, truth, 2e-3, "icp")) return 1;
  // the model rendered elsewhere: at the true pose
  if (map.AlignFrameToModelICP(depth.data(), start, &truth, nullptr, &icp) > TF_ALIGN_MAX_ITERS ||
      !near_truth(icp.pose, truth, 2e-3, "icp, model at the true pose")) return 1;
  tf_track_result trk;
  const int stage = map.TrackFrame(depth.data(), start, nullptr, nullptr, &trk);
  if (stage != 2 || trk.icp.status > TF_ALIGN_MAX_ITERS || trk.sdf.status > TF_ALIGN_MAX_ITERS) {
    std::printf("track: stage %d, icp %d, sdf %d\n", stage, trk.icp.status, trk.sdf.status);
    return 1;
  }
  if (!near_truth(trk.pose, truth, 1e-4, "track")) return 1;
  for (int i = 0; i < 12; ++i)
    if (trk.pose[i] != trk.sdf.pose[i]) { std::printf("track: pose is not the SDF stage's\n"); return 1; }
  // nothing to track: stage 0, the caller's pose
  std::vector<float> empty((size_t)W * H, 0.f);
  if (map.TrackFrame(empty.data(), start, nullptr, nullptr, &trk) != 0 || trk.icp.status != TF_ALIGN_TOO_FEW || trk.sdf.status != -1) {
    std::printf("empty frame: stage %d, icp %d, sdf %d\n", trk.stage, trk.icp.status, trk.sdf.status);
    return 1;
  }
  for (int i = 0; i < 12; ++i)
    if (trk.pose[i] != start.data()[i]) { std::printf("empty frame: pose moved\n"); return 1; }
  std::printf("mirror ok %d valid of %d\n", icp.n_valid_last, lit);
  return 0;
}
