// Chisel::AlignGroupToModel, AlignGroupLog and OptimizeKeyframeVoxelDomain of the host mirror
// (texturefusion_amd/host/tf_chisel.hpp) on the hand-built corner of tests/cpp_align/mirror_align.cpp: three frames, each
// rendered analytically at its own true pose, the keyframe's image kept only where it sees the face x = x0 (alone it is
// singular).  All three true poses are moved by (3, -2, 2.5) mm; away from the edges the SDF is linear, so one Gauss-Newton
// step of the three frames as one body returns every frame (1e-5 m, 1e-5 in every rotation entry).
// Built and run by tests/test_gpu_align_group.py; prints "mirror ok" and exits 0.
#include <hip/hip_runtime_api.h>

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

// z-depth of the corner from p, pixels within 6 voxels of an edge left out; face >= 0: only that face
static int render(const Pose& p, int face, std::vector<float>& depth) {
  depth.assign((size_t)W * H, 0.f);
  int lit = 0;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double dc[3] = {(x - 79.5) / 131.0, (y - 59.5) / 131.0, 1.0};
      double d[3], best = 1e30;
      int which = -1;
      for (int r = 0; r < 3; ++r) d[r] = p.R[3 * r] * dc[0] + p.R[3 * r + 1] * dc[1] + p.R[3 * r + 2] * dc[2];
      for (int r = 0; r < 3; ++r)
        if (d[r] < 0 && (x0[r] - p.t[r]) / d[r] < best) { best = (x0[r] - p.t[r]) / d[r]; which = r; }
      if (!(best > 0 && best < 1e29)) continue;
      int near_planes = 0;
      for (int r = 0; r < 3; ++r) near_planes += (p.t[r] + best * d[r] - x0[r]) < 6.0 * 0.01;
      if (near_planes == 1 && (face < 0 || which == face)) { depth[(size_t)y * W + x] = (float)best; ++lit; }
    }
  return lit;
}

static chisel::Transform as_transform(const Pose& p, const double delta[3]) {
  chisel::Transform T;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T(r, c) = (float)p.R[3 * r + c];
    T(r, 3) = (float)(p.t[r] + delta[r]);
  }
  return T;
}

static bool near_truth(const float* pose, const chisel::Transform& truth, const char* what) {
  double worst_t = 0, worst_r = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) worst_r = std::fmax(worst_r, std::fabs((double)pose[4 * r + c] - truth(r, c)));
    worst_t = std::fmax(worst_t, std::fabs((double)pose[4 * r + 3] - truth(r, 3)));
  }
  if (worst_t > 1e-5 || worst_r > 1e-5) { std::printf("%s: pose off by %g m / %g\n", what, worst_t, worst_r); return false; }
  return true;
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
  // keyframe: forward (-1, -1, -1) / sqrt(3), 0.38 m from the corner; two local frames a few centimetres and degrees away
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0), deg = 3.14159265358979323846 / 180.0;
  Pose T[3] = {{{-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3},
                {x0[0] + 0.38 * s3 + 0.01, x0[1] + 0.38 * s3 - 0.015, x0[2] + 0.38 * s3 + 0.02}}, {}, {}};
  const double dt1[3] = {0.03, -0.02, 0.01}, w1[3] = {3 * deg, -2 * deg, 1 * deg};
  const double dt2[3] = {-0.02, 0.03, 0.02}, w2[3] = {-2 * deg, 3.5 * deg, -1.5 * deg};
  T[1] = perturb(T[0], dt1, w1);
  T[2] = perturb(T[0], dt2, w2);
  std::vector<float> depth[3];
  int lit = 0, lit0 = 0;
  for (int k = 0; k < 3; ++k) {
    const int n = render(T[k], k == 0 ? 0 : -1, depth[k]);
    lit += n;
    if (k == 0) lit0 = n;
  }
  const double delta[3] = {0.003, -0.002, 0.0025}, none[3] = {0, 0, 0};
  std::vector<chisel::Transform> truth, start;
  for (int k = 0; k < 3; ++k) { truth.push_back(as_transform(T[k], none)); start.push_back(as_transform(T[k], delta)); }
  tf_align_params p;
  chisel::tf_check(tf_align_default_params(&p), "defaults");
  p.n_levels = 1; p.stride[0] = 1; p.iters[0] = 1; p.huber = 0.f; p.damping = 0.f;

  // the keyframe alone faces one plane
  tf_align_result alone;
  if (map.AlignFrameToModel(depth[0].data(), start[0], &p, &alone) != TF_ALIGN_SINGULAR) { std::printf("keyframe alone: status %d\n", alone.status); return 1; }
  // the three frames as one body
  tf_align_group_result out;
  const std::vector<const float*> images = {depth[0].data(), depth[1].data(), depth[2].data()};
  int status = map.AlignGroupToModel(images, start, {}, &p, &out);
  if (status != TF_ALIGN_MAX_ITERS || out.n_frames != 3 || out.n_bodies != 1 || out.body[0].evaluations != 2) {
    std::printf("group: status %d, %d frames, %d bodies, %d evaluations\n", status, out.n_frames, out.n_bodies, out.body[0].evaluations);
    return 1;
  }
  for (int k = 0; k < 3; ++k)
    if (!near_truth(out.pose[k], truth[k], "one body")) return 1;
  const std::vector<tf_align_iter> log = map.AlignGroupLog(0);
  const int n_valid = out.frame_valid_first[0] + out.frame_valid_first[1] + out.frame_valid_first[2];
  if (log.size() != 2 || log[0].n_valid != n_valid || n_valid < lit / 2 || n_valid > lit || out.frame_valid_first[0] > lit0 ||
      !map.AlignGroupLog(1).empty()) {
    std::printf("log: %zu records, %d valid (%d by frames) of %d lit\n", log.size(), log.empty() ? -1 : log[0].n_valid, n_valid, lit);
    return 1;
  }
  for (int i = 0; i < 3; ++i)
    if (std::fabs(log[0].xi[i] + delta[i]) > 1e-5 || std::fabs(log[0].xi[3 + i]) > 1e-5 || log[1].xi[i] != 0.0) {
      std::printf("step %d: %g %g\n", i, log[0].xi[i], log[0].xi[3 + i]);
      return 1;
    }
  // every frame its own body: the keyframe stops, the others go on
  status = map.AlignGroupToModel(images, start, {0, 1, 2}, &p, &out);
  if (status != TF_ALIGN_SINGULAR || out.n_bodies != 3 || out.body[0].status != TF_ALIGN_SINGULAR ||
      out.body[1].status != TF_ALIGN_MAX_ITERS || out.body[2].status != TF_ALIGN_MAX_ITERS) {
    std::printf("three bodies: %d / %d %d %d\n", status, out.body[0].status, out.body[1].status, out.body[2].status);
    return 1;
  }
  if (!near_truth(out.pose[1], truth[1], "body 1") || !near_truth(out.pose[2], truth[2], "body 2")) return 1;

  // OptimizeKeyframeVoxelDomain on the struct the keyframe unit takes: device images, poses written back
  float* d_depth[3] = {nullptr, nullptr, nullptr};
  tf_unit_group g = {};
  g.kf_id = 0; g.n_local = 2;
  for (int k = 0; k < 3; ++k) {
    if (hipMalloc((void**)&d_depth[k], sizeof(float) * W * H) != hipSuccess ||
        hipMemcpy(d_depth[k], depth[k].data(), sizeof(float) * W * H, hipMemcpyHostToDevice) != hipSuccess) {
      std::printf("device image %d\n", k);
      return 1;
    }
    tf_unit_frame& f = k == 0 ? g.keyframe : g.local[k - 1];
    f.d_depth = d_depth[k];
    for (int i = 0; i < 12; ++i) f.pose[i] = start[k].data()[i];
  }
  tf_unit_group loose = g;
  status = map.OptimizeKeyframeVoxelDomain(g, true, &p);
  if (status != TF_ALIGN_MAX_ITERS || !near_truth(g.keyframe.pose, truth[0], "unit keyframe") ||
      !near_truth(g.local[0].pose, truth[1], "unit local 0") || !near_truth(g.local[1].pose, truth[2], "unit local 1")) {
    std::printf("rigid unit group: status %d\n", status);
    return 1;
  }
  // not rigid: the keyframe's body is singular and its pose stays the start's
  status = map.OptimizeKeyframeVoxelDomain(loose, false, &p, &out);
  bool kept = true;
  for (int i = 0; i < 12; ++i) kept = kept && loose.keyframe.pose[i] == start[0].data()[i];
  if (status != TF_ALIGN_SINGULAR || !kept || !near_truth(loose.local[0].pose, truth[1], "loose local 0") ||
      !near_truth(loose.local[1].pose, truth[2], "loose local 1")) {
    std::printf("loose unit group: status %d, keyframe kept %d\n", status, (int)kept);
    return 1;
  }
  for (int k = 0; k < 3; ++k) (void)hipFree(d_depth[k]);
  std::printf("mirror ok %d valid of %d\n", n_valid, lit);
  return 0;
}
