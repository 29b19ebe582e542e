// Chisel::RelocConfigure, RelocIndexAdd and Relocalise of the host mirror (texturefusion_amd/host/tf_chisel.hpp) on the
// hand-built corner of tests/cpp_align_icp/mirror_align_icp.cpp with a smooth colour painted on its faces: two keyframes,
// the diagonal view and the same view rolled by 40 degrees, cached with their poses and put into the index; a frame
// rendered 80 mm and 5 degrees off the first one is handed to Relocalise without a pose.  It comes back TF_RELOC_FOUND
// from keyframe 7 at rank 0, within 1e-4 m of the frame's true pose.  Compiled by tests/test_reloc_cpu.py, built and run by
// tests/test_gpu_reloc.py; prints "mirror ok" and exits 0.
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

// z-depth of the corner from p (pixels within 2 voxels of an edge left out) and the colour of the point each ray meets
static void render(const Pose& p, std::vector<float>& depth, std::vector<uint8_t>& rgb) {
  depth.assign((size_t)W * H, 0.f);
  rgb.assign((size_t)W * H * 3, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double dc[3] = {(x - 79.5) / 131.0, (y - 59.5) / 131.0, 1.0};
      double d[3], best = 1e30;
      for (int r = 0; r < 3; ++r) d[r] = p.R[3 * r] * dc[0] + p.R[3 * r + 1] * dc[1] + p.R[3 * r + 2] * dc[2];
      for (int r = 0; r < 3; ++r)
        if (d[r] < 0 && (x0[r] - p.t[r]) / d[r] < best) best = (x0[r] - p.t[r]) / d[r];
      if (!(best > 0 && best < 1e29)) continue;
      double q[3];
      int near_planes = 0;
      for (int r = 0; r < 3; ++r) {
        q[r] = p.t[r] + best * d[r] - x0[r];
        near_planes += q[r] < 2.0 * 0.01;
      }
      uint8_t* c = &rgb[((size_t)y * W + x) * 3];
      c[0] = (uint8_t)std::lrint(128.0 + 110.0 * std::sin(7.0 * q[0] + 11.0 * q[1] + 0.3));
      c[1] = (uint8_t)std::lrint(128.0 + 110.0 * std::sin(9.0 * q[1] - 8.0 * q[2] + 1.1));
      c[2] = (uint8_t)std::lrint(128.0 + 110.0 * std::cos(10.0 * q[2] + 6.0 * q[0] - 0.7));
      if (near_planes == 1) depth[(size_t)y * W + x] = (float)best;
    }
}

static chisel::Transform as_transform(const Pose& p) {
  chisel::Transform T;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T(r, c) = (float)p.R[3 * r + c];
    T(r, 3) = (float)p.t[r];
  }
  return T;
}

// f32 of [R^T | -R^T t; 0 0 0 1], row-major: what tf_keyframe_set_pose takes
static void pose_inv16(const Pose& p, float out[16]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * r + c] = (float)p.R[3 * c + r];
    out[4 * r + 3] = (float)-(p.R[r] * p.t[0] + p.R[3 + r] * p.t[1] + p.R[6 + r] * p.t[2]);
  }
  out[12] = out[13] = out[14] = 0.f;
  out[15] = 1.f;
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
  // forward (-1, -1, -1) / sqrt(3), 0.38 m from the corner; the second keyframe rolled by 40 degrees about that axis
  const double s3 = 1.0 / std::sqrt(3.0), s2 = 1.0 / std::sqrt(2.0), s6 = 1.0 / std::sqrt(6.0), deg = 3.14159265358979323846 / 180.0;
  const Pose K0 = {{-s2, -s6, -s3, 0.0, 2.0 * s6, -s3, s2, -s6, -s3},
                   {x0[0] + 0.38 * s3, x0[1] + 0.38 * s3, x0[2] + 0.38 * s3}};
  const double none[3] = {0.0, 0.0, 0.0}, roll[3] = {-40.0 * deg * s3, -40.0 * deg * s3, -40.0 * deg * s3};
  const Pose K1 = perturb(K0, none, roll);
  const double dir_t[3] = {0.6, 0.53, 0.6}, dir_r[3] = {0.6, -0.64, 0.48};
  const double nt = std::sqrt(dir_t[0] * dir_t[0] + dir_t[1] * dir_t[1] + dir_t[2] * dir_t[2]);
  const double nr = std::sqrt(dir_r[0] * dir_r[0] + dir_r[1] * dir_r[1] + dir_r[2] * dir_r[2]);
  double dt[3], w[3];
  for (int i = 0; i < 3; ++i) { dt[i] = 0.080 * dir_t[i] / nt; w[i] = 5.0 * deg * dir_r[i] / nr; }
  const Pose Q = perturb(K0, dt, w);

  std::vector<float> depth;
  std::vector<uint8_t> rgb;
  const Pose* kf[2] = {&K0, &K1};
  const int32_t ids[2] = {7, 9};
  for (int k = 0; k < 2; ++k) {
    float inv[16];
    render(*kf[k], depth, rgb);
    pose_inv16(*kf[k], inv);
    chisel::tf_check(tf_keyframe_cache(v, ids[k], rgb.data(), depth.data()), "cache");
    chisel::tf_check(tf_keyframe_set_pose(v, ids[k], inv), "set pose");
  }
  map.RelocConfigure();
  map.RelocIndexAdd({9, 7});
  int64_t count = 0;
  chisel::tf_check(tf_reloc_index_count(v, &count), "count");
  if (count != 2) { std::printf("index holds %lld rows\n", (long long)count); return 1; }

  render(Q, depth, rgb);
  tf_relocalise_result out;
  const int status = map.Relocalise(depth.data(), rgb.data(), 3, nullptr, &out);
  if (status != TF_RELOC_FOUND || out.kf_id != 7 || out.rank != 0 || out.n_tried != 1 || out.tries[0].track.stage != 2) {
    std::printf("relocalise: status %d, keyframe %d, rank %d, %d tried\n", status, out.kf_id, out.rank, out.n_tried);
    return 1;
  }
  const chisel::Transform truth = as_transform(Q);
  double worst = 0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) worst = std::fmax(worst, std::fabs((double)out.pose[4 * r + c] - truth(r, c)));
  std::printf("relocalise: %g from the true pose, score %g over %d blocks\n", worst, out.tries[0].score, out.tries[0].overlap);
  if (worst > 1e-4) return 1;
  // without the keyframe it came from: the other one is tried
  map.RelocIndexRemove({7});
  map.Relocalise(depth.data(), rgb.data(), 3, nullptr, &out);
  if (out.n_tried != 1 || out.tries[0].kf_id != 9) { std::printf("after the removal: %d tried\n", out.n_tried); return 1; }
  std::printf("mirror ok\n");
  return 0;
}
