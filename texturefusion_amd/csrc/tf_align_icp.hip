// tf_align_icp.hip -- tracking a frame from far off: projective point-to-plane ICP of a depth frame against the model's
// vertex and normal maps (KinectFusion's frame-to-model tracking; the maps are what tf_raycast_device writes).  A pixel is
// associated by projecting its world point into the model camera, so it needs no SDF sample near the point: the capture
// range is that of the distance gate, not of the truncation band as tf_align_frame's.  The levels, the sums, the solve,
// the pose update, the stops, the log record and the result are tf_align_frame's (tf_align.hip); tests/align_icp_ref.py
// restates the rows.
//
//   k_icp_begin  one lane: the caller's pose (f64 and f32) and the model pose into the state block, the control words cleared
//   k_track_start  k_icp_begin for a start in device memory: both poses from a tf_device_pose cell, or the call stopped where
//                the cell holds no pose (the device tracker, tf_devpose.hip)
//   k_icp_rows   one wave per 8 x 8 tile of SAMPLED pixels (lane = 8 y + x, a tile spans 8 * stride image pixels), eight
//                waves per workgroup: association, residual, Jacobian and the wave's share of the normal equations; with map
//                outputs, the maps of tf_align_icp_residuals -- one body
//   k_icp_solve  one workgroup: the partials combined in tile order, the 6 x 6 solve and the pose update by one lane
//                (tf_align_solve.h), a log record, the result
//
// Inputs of an evaluation: the depth image, the current pose [R | t] (P, row-major 3 x 4, f32), the model maps Vm and Nm
// (f32 planar [3][H][W], world frame, of the same camera, Nm = 0 on a miss) and the pose [Rm | tm] (M) they were rendered
// from.  Per sampled pixel (x, y), all f32, every operation rounded on its own (-ffp-contract=off):
//   z = depth[y][x], in range iff finite and min_depth <= z <= max_depth                                       (bit 0)
//   dcx = ((float)x - cxs) / fx, dcy = ((float)y - cys) / fy with the int-truncated intrinsics, cxs = cx + 0.5, cys = cy + 0.5
//   pc = (dcx * z, dcy * z, z);  q_r = (P[r][0] * pc.x + P[r][1] * pc.y) + P[r][2] * z;  pw = t + q           (k_align_rows' text)
//   d = pw - tm;  pm_c = (M[0][c] * d.x + M[1][c] * d.y) + M[2][c] * d.z        (the point in the model camera, Rm^T d)
//   uf = floorf(((fx * pm.x) / pm.z + cxs) + 0.5f), vf = floorf(((fy * pm.y) / pm.z + cys) + 0.5f): the model pixel whose
//   raycast ray is the nearest;  pm.z > min_depth and 0 <= uf < W and 0 <= vf < H (compared as floats)         (bit 1)
//   i = (int)vf * W + (int)uf;  vm = Vm[:][i], nm = Nm[:][i];  (nm.x^2 + nm.y^2) + nm.z^2 > 0.5 (a hit)        (bit 2)
//   e = pw - vm;  r = (nm.x * e.x + nm.y * e.y) + nm.z * e.z
//   (e.x^2 + e.y^2) + e.z^2 <= max_distance * max_distance and |r| <= max_residual                             (bit 3)
//   each bit is set only where the lower ones are; the pixel is valid iff all four are.
//   J = (nm.x, nm.y, nm.z, q.y nm.z - q.z nm.y, q.z nm.x - q.x nm.z, q.x nm.y - q.y nm.x): tf_align_frame's twist about
//   the camera centre with the model normal for the gradient
//   w = 1 if huber == 0 or |r| <= huber, else huber / |r|;  wJ_i = w * J_i,  wr = w * r  (f32)
// Sums, their order, the partial rows and the whole solve launch are tf_align_frame's by the same functions
// (tf_align_rows.h: al_row_sums, al_store_rows, al_solve_pose).
// No atomics, no counters, no polling: a call is 1 + 2 launches per evaluation, all enqueued up front; a launch first
// reads the state word (bit 0: stopped, bits 8..: levels that are finished) and returns if it has nothing to do.  The
// model pose and the maps do not change during a call.
// With a gate set on the handle (tf_align_icp_set_gate) the rows launch is k_gated_rows of tf_align_icp_gate.hip: the same
// association (icp_assoc, tf_align_icp_rows.h) and flag bits 4 and 5 from the frame's own normal; everything else is this file's.
// With a depth pyramid set on the handle (tf_align_icp_set_pyramid) the forms that raycast the model themselves hand the
// rows launch of a level of stride 2^k the level's image, camera and maps (tf_align_icp_pyramid.hip builds the images, this
// file raycasts a map pair per level in the schedule), at stride 1; the kernels and the solve are the same.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_icp_pyramid.h"
#include "tf_align_icp_rows.h"
#include "tf_align_rows.h"
#include "tf_devpose.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct IcpDev {
  AlignCtl* ctl;
  double* pose_d;       // [12] the pose between iterations
  float* pose_f;        // [24] the same rounded, then the model pose: what k_icp_rows reads
  float* pose_r;        // [24] tf_align_icp_residuals' pair (the last alignment's state stays as it is)
  tf_align_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
  double* part;         // [ceil(cap_tiles / kAlWaves)][kAlRow]: a row per workgroup of k_icp_rows
};
struct IcpPoses { float p[12], m[12]; };

struct IcpSolveArgs {
  AlignSolveCommon c;
  tf_align_result* out;
};

__global__ __launch_bounds__(64) void k_icp_begin(IcpDev d, IcpPoses p, int residuals_only) {
  const int i = threadIdx.x;
  if (residuals_only) {
    if (i < 12) { d.pose_r[i] = p.p[i]; d.pose_r[12 + i] = p.m[i]; }
    return;
  }
  if (i < 12) { d.pose_d[i] = (double)p.p[i]; d.pose_f[i] = p.p[i]; d.pose_f[12 + i] = p.m[i]; }
  if (i == 0) {
    AlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    *d.ctl = c;
  }
}

// The begin launch of a call whose start is in device memory (tf_devpose.h): the frame's pose and the model's are the
// cell's.  A cell that holds no pose stops the call before it starts -- bit 0 of the state word, which every rows and
// solve launch tests -- with status -1 in the control words (what the stage behind this one and the finish read) and no
// records; the result is not written then.
__global__ __launch_bounds__(64) void k_track_start(IcpDev d, const tf_device_pose* __restrict__ cell) {
  const int i = threadIdx.x;
  const float p = cell->pose[i < 12 ? i : 0];
  const bool ok = devpose_ok_wave(cell, p);
  if (ok && i < 12) { d.pose_d[i] = (double)p; d.pose_f[i] = p; d.pose_f[12 + i] = p; }
  if (i == 0) {
    AlignCtl c{};
    c.status = ok ? TF_ALIGN_MAX_ITERS : -1;
    c.state = ok ? 0u : 1u;
    *d.ctl = c;
  }
}

// (resources: tests/test_kernel_resources_align_icp.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_icp_rows(IcpRowsArgs a) {
  if (a.state && al_idle(a.state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  uint32_t fl = 0;
  int32_t as = -1;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  AlPoint p{};
  if (px.in) {
    const size_t o = (size_t)px.Y * a.c.W + (size_t)px.X;
    if (al_point(a.c, px, a.depth[o], a.pose, &p)) {
      const IcpAssoc m = icp_assoc(a, p);  // bits 1 to 3: tf_align_icp_rows.h, the gated kernel's too
      fl = m.fl; as = m.as;
      s = m.s; gx = m.gx; gy = m.gy; gz = m.gz;
    }
    if (a.r) a.r[o] = s;
    if (a.flags) a.flags[o] = fl;
    if (a.assoc) a.assoc[o] = as;
  }
  if (!a.part) return;
  // tf_align_frame's twist about the camera centre with the model normal for the gradient
  __shared__ double wsum[kAlWaves][kAlRow];
  al_row_sums(wsum, 0, px, gx, gy, gz, p.qx, p.qy, p.qz, s, a.c.huber, fl == 15u, px.in);
  al_store_rows(wsum, a.part + (size_t)blockIdx.x * kAlRow);
}

__global__ __launch_bounds__(256) void k_icp_solve(IcpDev d, IcpSolveArgs a) {
  al_solve_pose(d.ctl, d.log, d.pose_d, d.pose_f, d.part, a.c, a.out);
}

// the state block as it lies in AlignIcpState::st (base == null: its size)
IcpDev icp_carve(void* base, size_t cap_tiles, size_t* bytes) {
  IcpDev d{};
  Carver c(base);
  c.take(d.ctl, 1);
  c.take(d.pose_d, 12);
  c.take(d.pose_f, 24);
  c.take(d.pose_r, 24);
  c.take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kAlRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = c.L.size;
  return d;
}
int icp_dev(tf_volume* v, IcpDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; icp_carve(nullptr, tiles, &n); return n; };
  AlignBlock& s = v->align_icp.st;
  const int rc = align_ensure(v, s, bytes_of, sizeof(AlignCtl));
  if (rc) return rc;
  *d = icp_carve(s.block.p, s.cap_tiles, nullptr);
  return TF_OK;
}

// the six map planes of the forms that raycast themselves: vertex [3][H][W], then normal [3][H][W]
int icp_ensure_maps(tf_volume* v, float** d_vertex, float** d_normal) {
  const size_t P = align_pixels(v);
  AlignIcpState& s = v->align_icp;
  if (!s.maps || s.map_pixels < P) {
    if (s.maps) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = s.maps.alloc(24 * P);
    if (rc) { s.map_pixels = 0; return rc; }
    s.map_pixels = P;
  }
  *d_vertex = s.maps.as<float>();
  *d_normal = s.maps.as<float>(12 * P);
  return TF_OK;
}

bool ray_params_ok(const tf_align_icp_params* p) {
  if (!(p->ray_near >= 0.f) || !(p->ray_far > p->ray_near) || !isfinite(p->ray_far)) {
    set_error("need 0 <= near < far < inf");
    return false;
  }
  if (p->ray_max_steps <= 0) { set_error("max_steps must be positive"); return false; }
  return true;
}

// everything a call is refused for, but the map and result pointers (they differ by form)
int icp_check(tf_volume* v, const float* depth, const float* pose, const float* model_pose, const tf_align_icp_params* p,
              bool with_iters, bool with_ray) {
  if (!p) { set_error("null argument"); return TF_ERR_INVALID; }
  int rc = align_check(v, depth, pose, &p->geo, with_iters);
  if (rc) return rc;
  if (!(p->max_distance >= 0.f) || !isfinite(p->max_distance)) {
    set_error("align icp: max_distance must be finite and >= 0");
    return TF_ERR_INVALID;
  }
  if (model_pose && !finite_all(model_pose, 12)) { set_error("model pose is not finite"); return TF_ERR_INVALID; }
  if (with_ray && !ray_params_ok(p)) return TF_ERR_INVALID;
  if (with_ray && icp_pyramid_on(v)) return icp_pyramid_check(v, p->geo, p->geo.n_levels);  // the forms that raycast themselves
  return TF_OK;
}

IcpRowsArgs icp_rows_args(const AlignRowsCommon& rc, const tf_align_icp_params& p, const float* d_depth, const float* d_vertex,
                          const float* d_normal) {
  IcpRowsArgs a{};
  a.c = rc;
  a.depth = d_depth; a.vm = d_vertex; a.nm = d_normal;
  a.max_dist2 = p.max_distance * p.max_distance;
  a.plane = (size_t)rc.W * rc.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close.  d_start != null: frame pose
// and model pose are that cell's, read on the device (pose and model_pose are not read).  lv != null: the pyramid is on,
// and a level of stride 2^k evaluates lv's image, camera and maps of level k (d_depth, d_vertex, d_normal are not read).
int icp_enqueue(tf_volume* v, const float* d_depth, const float* pose, const float* d_vertex, const float* d_normal,
                const float* model_pose, const tf_align_icp_params& p, tf_align_result* d_result,
                const tf_device_pose* d_start = nullptr, const IcpLevels* lv = nullptr) {
  IcpDev d;
  int rc = icp_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  if (d_start) {
    hipLaunchKernelGGL(k_track_start, dim3(1), dim3(64), 0, st, d, d_start);
  } else {
    IcpPoses P;
    memcpy(P.p, pose, sizeof(P.p));
    memcpy(P.m, model_pose, sizeof(P.m));
    hipLaunchKernelGGL(k_icp_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  }
  const bool gated = icp_gate_on(v);  // tf_align_icp_set_gate: the rows launch is tf_align_icp_gate.hip's
  align_walk(v, p.geo, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    const int k = lv ? __builtin_ctz((unsigned)sc.stride) : 0;
    IcpRowsArgs ra = lv ? icp_rows_args(c, p, lv->depth[k], lv->vm[k], lv->nm[k]) : icp_rows_args(c, p, d_depth, d_vertex, d_normal);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    if (gated) gated_rows_launch(v, ra, sc.n_rows);
    else hipLaunchKernelGGL(k_icp_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, ra);
    hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(256), 0, st, d, IcpSolveArgs{sc, d_result});
  }, lv ? lv->cam : nullptr);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int icp_residuals_enqueue(tf_volume* v, const float* d_depth, const float* pose, const float* d_vertex,
                          const float* d_normal, const float* model_pose, const tf_align_icp_params& p, float* d_r,
                          uint32_t* d_flags, int32_t* d_assoc, const IcpLevels* lv = nullptr) {
  IcpDev d;
  int rc = icp_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  AlignRowsCommon c;
  AlignSolveCommon sc;
  // lv != null: the pyramid is on, and the evaluation is of level k = log2(stride[0]) -- its image, camera and maps; the
  // rows launch writes level-sized maps of the handle's, which are spread over the caller's behind it
  const int k = lv ? __builtin_ctz((unsigned)p.geo.stride[0]) : 0;
  if (lv) align_level_image(lv->cam[k], p.geo, 0, &c, &sc);
  else align_level(v, p.geo, 0, &c, &sc);
  IcpRowsArgs ra = lv ? icp_rows_args(c, p, lv->depth[k], lv->vm[k], lv->nm[k]) : icp_rows_args(c, p, d_depth, d_vertex, d_normal);
  ra.pose = d.pose_r; ra.r = d_r; ra.flags = d_flags; ra.assoc = d_assoc;
  if (k > 0 && (rc = icp_pyramid_residual_maps(v, k, &ra.r, &ra.flags, &ra.assoc))) return rc;
  if (c.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
    if (d_assoc) TF_HIP(hipMemsetAsync(d_assoc, 0xFF, 4 * ra.plane, st));  // -1
  }
  IcpPoses P;
  memcpy(P.p, pose, sizeof(P.p));
  memcpy(P.m, model_pose, sizeof(P.m));
  hipLaunchKernelGGL(k_icp_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  if (icp_gate_on(v)) gated_rows_launch(v, ra, sc.n_rows);
  else hipLaunchKernelGGL(k_icp_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, ra);
  TF_HIP(hipGetLastError());
  return k > 0 ? icp_pyramid_spread(v, k, d_r, d_flags, d_assoc) : TF_OK;
}

// the model raycast at model_pose into the state block's own maps: tf_raycast_device's launch
int icp_raycast(tf_volume* v, const float* model_pose, const tf_align_icp_params& p, float** d_vertex, float** d_normal) {
  int rc = icp_ensure_maps(v, d_vertex, d_normal);
  if (rc) return rc;
  return tf_raycast_device(v, model_pose, p.ray_near, p.ray_far, p.ray_max_steps, nullptr, *d_normal, nullptr, *d_vertex);
}

// What a call that raycasts the model itself evaluates with the pyramid on: the level images of the strides of the first
// n_levels (one launch), then a raycast per such stride at that level's camera -- at model_pose, or at the pose in
// *d_cell -- level 0's being the raycast of a call with the pyramid off, into the same maps.
int icp_model_levels(tf_volume* v, const float* d_depth, const float* model_pose, const tf_device_pose* d_cell,
                     const tf_align_icp_params& p, int n_levels, IcpLevels* lv) {
  int rc = icp_pyramid_enqueue(v, d_depth, p.geo, n_levels, d_cell, lv);
  for (int k = 0; k < 4 && !rc; ++k) {
    if (!((lv->used >> k) & 1u)) continue;
    if (k > 0) rc = raycast_level(v, model_pose, d_cell, p.ray_near, p.ray_far, p.ray_max_steps, lv->cam[k], lv->nm[k], lv->vm[k]);
    else if (!d_cell) rc = icp_raycast(v, model_pose, p, &lv->vm[0], &lv->nm[0]);
    else if (!(rc = icp_ensure_maps(v, &lv->vm[0], &lv->nm[0])))
      rc = raycast_posed(v, d_cell, p.ray_near, p.ray_far, p.ray_max_steps, lv->nm[0], lv->vm[0]);
  }
  return rc;
}

}  // namespace

void align_icp_release(tf_volume* v) { v->align_icp = AlignIcpState{}; }

int align_icp_check(tf_volume* v, const float* depth, const float* pose, const float* model_pose, const tf_align_icp_params* p,
                    bool with_iters, bool with_ray) {
  return icp_check(v, depth, pose, model_pose, p, with_iters, with_ray);
}

int track_check(tf_volume* v, const float* depth, const float* pose, const tf_align_icp_params* icp_params,
                const tf_align_params* sdf_params) {
  const int rc = icp_check(v, depth, pose, nullptr, icp_params, true, true);
  return rc ? rc : align_check(v, depth, pose, sdf_params, true);
}

// tf_track_frame's first stage with everything in device memory: the model raycast at *d_start into the handle's maps,
// the alignment from *d_start against them, all enqueued, nothing read back (tf_devpose.hip; the caller has checked).
// *d_status: the status word of the state block, the call's status once its launches are through (-1: no pose, not run).
int track_icp_posed(tf_volume* v, const float* d_depth, const tf_device_pose* d_start, const tf_align_icp_params& p,
                    tf_align_result* d_result, const int32_t** d_status) {
  float *d_v = nullptr, *d_n = nullptr;
  int rc;
  if (icp_pyramid_on(v)) {
    IcpLevels lv;
    if ((rc = icp_model_levels(v, d_depth, nullptr, d_start, p, p.geo.n_levels, &lv))) return rc;
    if ((rc = icp_enqueue(v, d_depth, nullptr, nullptr, nullptr, nullptr, p, d_result, d_start, &lv))) return rc;
  } else {
    rc = icp_ensure_maps(v, &d_v, &d_n);
    if (rc || (rc = raycast_posed(v, d_start, p.ray_near, p.ray_far, p.ray_max_steps, d_n, d_v))) return rc;
    if ((rc = icp_enqueue(v, d_depth, nullptr, d_v, d_n, nullptr, p, d_result, d_start))) return rc;
  }
  IcpDev d;
  if ((rc = icp_dev(v, &d))) return rc;
  *d_status = &d.ctl->status;
  return TF_OK;
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_icp_default_params(tf_align_icp_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_align_icp_params p{};
  p.geo.n_levels = 3;
  p.geo.stride[0] = 4; p.geo.stride[1] = 2; p.geo.stride[2] = 1; p.geo.stride[3] = 1;
  p.geo.iters[0] = 6; p.geo.iters[1] = 4; p.geo.iters[2] = 3; p.geo.iters[3] = 0;
  p.geo.min_depth = 0.05f; p.geo.max_depth = 5.0f; p.geo.max_residual = 0.15f; p.geo.huber = 0.02f; p.geo.damping = 0.f;
  p.geo.eps_t = 1e-5f; p.geo.eps_r = 1e-5f;
  p.geo.min_valid = 100;
  p.max_distance = 0.15f;
  p.ray_near = 0.05f; p.ray_far = 5.0f; p.ray_max_steps = 1024;
  *out = p;
  return TF_OK;
}

int tf_align_frame_icp_device(tf_volume* v, const float* d_depth, const float pose[12], const float* d_model_vertex,
                              const float* d_model_normal, const float model_pose[12], const tf_align_icp_params* params,
                              tf_align_result* d_result) {
  int rc = icp_check(v, d_depth, pose, model_pose, params, true, false);
  if (rc) return rc;
  if (!d_model_vertex || !d_model_normal || !model_pose || !d_result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  return icp_enqueue(v, d_depth, pose, d_model_vertex, d_model_normal, model_pose, *params, d_result);
}

int tf_align_frame_icp(tf_volume* v, const float* depth, const float pose[12], const float* model_pose,
                       const tf_align_icp_params* params, tf_align_result* result) {
  int rc = icp_check(v, depth, pose, model_pose, params, true, true);
  if (rc) return rc;
  if (!result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const float* mp = model_pose ? model_pose : pose;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_r = L.take(sizeof(tf_align_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  if (icp_pyramid_on(v)) {
    IcpLevels lv;
    if ((rc = icp_model_levels(v, sg.dp<const float>(o_d), mp, nullptr, *params, params->geo.n_levels, &lv))) return rc;
    rc = icp_enqueue(v, nullptr, pose, nullptr, nullptr, mp, *params, sg.dp<tf_align_result>(o_r), nullptr, &lv);
  } else {
    float *d_v = nullptr, *d_n = nullptr;
    if ((rc = icp_raycast(v, mp, *params, &d_v, &d_n))) return rc;
    rc = icp_enqueue(v, sg.dp<const float>(o_d), pose, d_v, d_n, mp, *params, sg.dp<tf_align_result>(o_r));
  }
  if (rc) return rc;
  return stage_out(v, sg, o_r, sizeof(tf_align_result), result);
}

int tf_align_icp_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  const AlignBlock& s = v->align_icp.st;
  const IcpDev d = s.block ? icp_carve(s.block.p, s.cap_tiles, nullptr) : IcpDev{};
  return align_log(v, d.ctl, d.log, sizeof(tf_align_iter), out, cap, n);
}

int tf_align_icp_residuals_device(tf_volume* v, const float* d_depth, const float pose[12], const float* d_model_vertex,
                                  const float* d_model_normal, const float model_pose[12],
                                  const tf_align_icp_params* params, float* d_r, uint32_t* d_flags, int32_t* d_assoc) {
  int rc = icp_check(v, d_depth, pose, model_pose, params, false, false);
  if (rc) return rc;
  if (!d_model_vertex || !d_model_normal || !model_pose) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!d_r && !d_flags && !d_assoc) return TF_OK;
  return icp_residuals_enqueue(v, d_depth, pose, d_model_vertex, d_model_normal, model_pose, *params, d_r, d_flags, d_assoc);
}

int tf_align_icp_residuals(tf_volume* v, const float* depth, const float pose[12], const float* model_vertex,
                           const float* model_normal, const float* model_pose, const tf_align_icp_params* params, float* r,
                           uint32_t* flags, int32_t* assoc) {
  const bool own = !model_vertex && !model_normal;  // no maps given: raycast them
  int rc = icp_check(v, depth, pose, model_pose, params, false, own);
  if (rc) return rc;
  if (!own && (!model_vertex || !model_normal)) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!r && !flags && !assoc) return TF_OK;
  const float* mp = model_pose ? model_pose : pose;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_v = L.take(own ? 0 : 12 * P), o_n = L.take(own ? 0 : 12 * P);
  const size_t o_r = L.take(r ? 4 * P : 0), o_f = L.take(flags ? 4 * P : 0), o_a = L.take(assoc ? 4 * P : 0);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  float *d_v = nullptr, *d_n = nullptr;
  IcpLevels lv;
  const bool pyr = own && icp_pyramid_on(v);
  if (pyr) {
    if ((rc = icp_model_levels(v, sg.dp<const float>(o_d), mp, nullptr, *params, 1, &lv))) return rc;
  } else if (own) {
    if ((rc = icp_raycast(v, mp, *params, &d_v, &d_n))) return rc;
  } else {
    if ((rc = stage_in(v, sg, o_v, model_vertex, 12 * P)) || (rc = stage_in(v, sg, o_n, model_normal, 12 * P))) return rc;
    d_v = sg.dp<float>(o_v); d_n = sg.dp<float>(o_n);
  }
  rc = icp_residuals_enqueue(v, sg.dp<const float>(o_d), pose, d_v, d_n, mp, *params, r ? sg.dp<float>(o_r) : nullptr,
                             flags ? sg.dp<uint32_t>(o_f) : nullptr, assoc ? sg.dp<int32_t>(o_a) : nullptr, pyr ? &lv : nullptr);
  if (rc) return rc;
  if ((rc = stage_out(v, sg, o_r, L.size - o_r, nullptr))) return rc;
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  if (assoc) memcpy(assoc, sg.h + o_a, 4 * P);
  return TF_OK;
}

int tf_track_frame(tf_volume* v, const float* depth, const float pose[12], const tf_align_icp_params* icp_params,
                   const tf_align_params* sdf_params, tf_track_result* out) {
  int rc = track_check(v, depth, pose, icp_params, sdf_params);
  if (rc) return rc;
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_track_result t{};
  t.sdf.status = -1;  // not run
  memcpy(t.pose, pose, sizeof(t.pose));
  if ((rc = tf_align_frame_icp(v, depth, pose, nullptr, icp_params, &t.icp))) return rc;
  if (t.icp.status <= TF_ALIGN_MAX_ITERS) {
    t.stage = 1;
    memcpy(t.pose, t.icp.pose, sizeof(t.pose));
    if ((rc = tf_align_frame(v, depth, t.icp.pose, sdf_params, &t.sdf))) return rc;
    if (t.sdf.status <= TF_ALIGN_MAX_ITERS) {
      t.stage = 2;
      memcpy(t.pose, t.sdf.pose, sizeof(t.pose));
    }
  }
  *out = t;
  return TF_OK;
}

}  // extern "C"
