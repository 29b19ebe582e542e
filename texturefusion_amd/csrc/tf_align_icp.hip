// tf_align_icp.hip -- tracking a frame from far off: projective point-to-plane ICP of a depth frame against the model's
// vertex and normal maps (KinectFusion's frame-to-model tracking; the maps are what tf_raycast_device writes).  A pixel is
// associated by projecting its world point into the model camera, so it needs no SDF sample near the point: the capture
// range is that of the distance gate, not of the truncation band as tf_align_frame's.  The levels, the sums, the solve,
// the pose update, the stops, the log record and the result are tf_align_frame's (tf_align.hip); tests/align_icp_ref.py
// restates the rows.
//
//   k_icp_begin  one lane: the caller's pose (f64 and f32) and the model pose into the state block, the control words cleared
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
// Sums, their order, the partial rows and the solve launch's additions: tf_align.hip's header, word for word (the wave tree
// of tf_align_tree.h, the eight tiles of a workgroup in wave order, one plain-stored row per workgroup, the rows g, g + 8,
// .. ascending, then the eight groups in order).
// No atomics, no counters, no polling: a call is 1 + 2 launches per evaluation, all enqueued up front; a launch first
// reads the state word (bit 0: stopped, bits 8..: levels that are finished) and returns if it has nothing to do.  The
// model pose and the maps do not change during a call.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <type_traits>

#include "tf_align_solve.h"
#include "tf_align_tree.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct IcpCtl {
  uint32_t state;  // bit 0: stopped (too few / singular), bits 8..: levels finished
  int32_t status;
  int32_t n_eval;
  int32_t n_valid_first;
  float rms_first;
  uint32_t pad[3];
};
struct IcpDev {
  IcpCtl* ctl;
  double* pose_d;       // [12] the pose between iterations
  float* pose_f;        // [24] the same rounded, then the model pose: what k_icp_rows reads
  float* pose_r;        // [24] tf_align_icp_residuals' pair (the last alignment's state stays as it is)
  tf_align_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
  double* part;         // [ceil(cap_tiles / kAlWaves)][kAlRow]: a row per workgroup of k_icp_rows
  uint32_t cap_tiles;   // tiles of the camera at stride 1
};
struct IcpPoses { float p[12], m[12]; };

struct IcpRowsArgs {
  const float* depth;
  const float* vm;        // model vertex map, planar
  const float* nm;        // model normal map, planar
  const float* pose;      // 24 floats in the state block: the frame's pose, the model's
  const uint32_t* state;  // null: always run (tf_align_icp_residuals)
  float fx, fy, cxs, cys;
  int W, H, tiles_x, stride, level;
  float min_depth, max_depth, max_residual, max_dist2, huber;
  size_t plane;
  float* r;
  uint32_t* flags;
  int32_t* assoc;
  double* part;  // null: no sums
};
struct IcpSolveArgs {
  int level, log_level, stride, closing, last_level;
  uint32_t n_rows;  // workgroups of the rows launch
  float damping, eps_t, eps_r;
  int min_valid;
  tf_align_result* out;
};

__device__ __forceinline__ bool icp_idle(const uint32_t* state, int level) {
  const uint32_t st = *state;
  return (st & 1u) || (uint32_t)level < (st >> 8);
}
__global__ __launch_bounds__(64) void k_icp_begin(IcpDev d, IcpPoses p, int residuals_only) {
  const int i = threadIdx.x;
  if (residuals_only) {
    if (i < 12) { d.pose_r[i] = p.p[i]; d.pose_r[12 + i] = p.m[i]; }
    return;
  }
  if (i < 12) { d.pose_d[i] = (double)p.p[i]; d.pose_f[i] = p.p[i]; d.pose_f[12 + i] = p.m[i]; }
  if (i == 0) {
    IcpCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    *d.ctl = c;
  }
}

// (resources: tests/test_kernel_resources_align_icp.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_icp_rows(IcpRowsArgs a) {
  if (a.state && icp_idle(a.state, a.level)) return;
  // (a tile beyond the last one of the level lies below the image: none of its lanes is inside)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kAlWaves + wave;
  const long long X = (long long)((tile % a.tiles_x) * 8 + (lane & 7)) * a.stride;
  const long long Y = (long long)((tile / a.tiles_x) * 8 + (lane >> 3)) * a.stride;
  const bool in = X < a.W && Y < a.H;
  uint32_t fl = 0;
  int32_t as = -1;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  if (in) {
    const size_t o = (size_t)Y * a.W + (size_t)X;
    const float z = a.depth[o];
    if (isfinite(z) && z >= a.min_depth && z <= a.max_depth) {
      fl = 1u;
      const float dcx = ((float)(int)X - a.cxs) / a.fx, dcy = ((float)(int)Y - a.cys) / a.fy;
      const float pcx = dcx * z, pcy = dcy * z;
      const float* P = a.pose;
      const float* M = a.pose + 12;
      qx = (P[0] * pcx + P[1] * pcy) + P[2] * z;
      qy = (P[4] * pcx + P[5] * pcy) + P[6] * z;
      qz = (P[8] * pcx + P[9] * pcy) + P[10] * z;
      const float wx = P[3] + qx, wy = P[7] + qy, wz = P[11] + qz;
      const float dx = wx - M[3], dy = wy - M[7], dz = wz - M[11];
      const float mx = (M[0] * dx + M[4] * dy) + M[8] * dz;
      const float my = (M[1] * dx + M[5] * dy) + M[9] * dz;
      const float mz = (M[2] * dx + M[6] * dy) + M[10] * dz;
      if (mz > a.min_depth) {
        const float uf = floorf(((a.fx * mx) / mz + a.cxs) + 0.5f), vf = floorf(((a.fy * my) / mz + a.cys) + 0.5f);
        // (compared as floats: a NaN or an infinity of a point near the model camera's plane fails here, ahead of the cast)
        if (uf >= 0.f && uf < (float)a.W && vf >= 0.f && vf < (float)a.H) {
          fl |= 2u;
          const size_t i = (size_t)(int)vf * (size_t)a.W + (size_t)(int)uf;  // < W * H
          as = (int32_t)i;
          // the six scattered loads of the pixel, all issued ahead of the first use: one batch in flight
          const float nx = a.nm[i], ny = a.nm[a.plane + i], nz = a.nm[2 * a.plane + i];
          const float vx = a.vm[i], vy = a.vm[a.plane + i], vz = a.vm[2 * a.plane + i];
          // (selects, not a branch on the normal: a branch would let the compiler hold the vertex loads back behind it)
          const bool hit = (nx * nx + ny * ny) + nz * nz > 0.5f;
          const float ex = wx - vx, ey = wy - vy, ez = wz - vz;
          const float rr = (nx * ex + ny * ey) + nz * ez;
          const bool near = (ex * ex + ey * ey) + ez * ez <= a.max_dist2 && fabsf(rr) <= a.max_residual;
          s = hit ? rr : 0.f;
          gx = hit ? nx : 0.f; gy = hit ? ny : 0.f; gz = hit ? nz : 0.f;
          fl |= hit ? (near ? 12u : 4u) : 0u;
        }
      }
    }
    if (a.r) a.r[o] = s;
    if (a.flags) a.flags[o] = fl;
    if (a.assoc) a.assoc[o] = as;
  }
  if (!a.part) return;
  const bool valid = fl == 15u;
  float J[6] = {gx, gy, gz, qy * gz - qz * gy, qz * gx - qx * gz, qx * gy - qy * gx};
  const float ar = fabsf(s);
  float w = (a.huber == 0.f || ar <= a.huber) ? 1.0f : a.huber / ar;
  float r = s;
  if (!valid) {  // an exact zero in every term
    w = 0.f; r = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = 0.f;
  }
  // the 31 sums of the tile through the wave tree (tf_align_tree.h): lane l ends up with entry al_entry(l)
  const double total = al_tile_sum(J, w, r, valid ? 1.0f : 0.0f, in ? 1.0f : 0.0f, lane);
  const int e = al_entry(lane);
  // the workgroup's eight tiles in wave order, one plain-stored row per workgroup
  __shared__ double wsum[kAlWaves][kAlRow];
  if (!(lane & 1)) wsum[wave][e] = total;
  __syncthreads();
  if (threadIdx.x < (unsigned)kAlSums) {
    double t = wsum[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kAlWaves; ++k) t += wsum[k][threadIdx.x];
    a.part[(size_t)blockIdx.x * kAlRow + threadIdx.x] = t;
  }
}

// k_align_solve's text on this file's state block (tf_align.hip stays as it is, so its launch is copied, as
// tf_align_group.hip copied it)
__global__ __launch_bounds__(256) void k_icp_solve(IcpDev d, IcpSolveArgs a) {
  if (icp_idle(&d.ctl->state, a.level)) return;
  // thread (e = tid & 31, g = tid >> 5) adds entry e of the rows g, g + 8, g + 16, .. in ascending order; then the eight
  // groups in order
  __shared__ double red[8][kAlRow];
  const uint32_t tid = threadIdx.x, e = tid & 31u, g = tid >> 5;
  double acc = 0.0;
  if (e < (uint32_t)kAlSums)
#pragma unroll 8
    for (uint32_t t = g; t < a.n_rows; t += 8u) acc += d.part[(size_t)t * kAlRow + e];
  red[g][e] = acc;
  __syncthreads();
  if (tid != 0) return;
  double S[kAlSums];
#pragma unroll
  for (int i = 0; i < kAlSums; ++i) {
    double t = red[0][i];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][i];
    S[i] = t;
  }
  IcpCtl c = *d.ctl;
  const int n_valid = (int)S[kAlNv], n_sampled = (int)S[kAlNs];
  const float rms = n_valid > 0 ? (float)sqrt(S[kAlR2] / (double)n_valid) : 0.f;
  tf_align_iter* rec = d.log + (c.n_eval < TF_ALIGN_MAX_EVALUATIONS ? c.n_eval : TF_ALIGN_MAX_EVALUATIONS - 1);
  rec->level = a.log_level; rec->stride = a.stride; rec->n_sampled = n_sampled; rec->n_valid = n_valid;
  rec->sum_r2 = S[kAlR2]; rec->sum_wr2 = S[kAlWr2];
#pragma unroll
  for (int i = 0; i < 21; ++i) rec->A[i] = S[kAlA + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) { rec->b[i] = S[kAlB + i]; rec->xi[i] = 0.0; }
  double pose[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { pose[i] = d.pose_d[i]; rec->pose[i] = pose[i]; }
  if (c.n_eval == 0) { c.n_valid_first = n_valid; c.rms_first = rms; }
  c.n_eval += 1;
  if (n_valid < a.min_valid) {
    c.status = TF_ALIGN_TOO_FEW;
    c.state |= 1u;
  } else if (!a.closing) {
    double xi[6];
    if (!align_solve6(S + kAlA, S + kAlB, (double)a.damping, xi)) {
      c.status = TF_ALIGN_SINGULAR;
      c.state |= 1u;
    } else {
      align_update(pose, xi);
#pragma unroll
      for (int i = 0; i < 12; ++i) { d.pose_d[i] = pose[i]; d.pose_f[i] = (float)pose[i]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) rec->xi[i] = xi[i];
      const double nt = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
      const double nr = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
      if (nt < (double)a.eps_t && nr < (double)a.eps_r) {
        c.state = (c.state & 0xFFu) | ((uint32_t)(a.level + 1) << 8);
        if (a.last_level) c.status = TF_ALIGN_CONVERGED;
      }
    }
  }
  *d.ctl = c;
  tf_align_result* out = a.out;
  out->status = c.status; out->evaluations = c.n_eval; out->n_sampled = n_sampled;
  out->n_valid_first = c.n_valid_first; out->n_valid_last = n_valid;
  out->rms_first = c.rms_first; out->rms_last = rms;
#pragma unroll
  for (int i = 0; i < 12; ++i) out->pose[i] = (float)pose[i];
}

// the state block as it lies in AlignIcpState::block (base == null: its size)
IcpDev icp_carve(void* base, size_t cap_tiles, size_t* bytes) {
  IcpDev d{};
  d.cap_tiles = (uint32_t)cap_tiles;
  Layout L;
  uint8_t* b = static_cast<uint8_t*>(base);
  const auto take = [&](auto*& p, size_t count) {
    const size_t at = L.take(count * sizeof(*p));
    p = b ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + at) : nullptr;
  };
  take(d.ctl, 1);
  take(d.pose_d, 12);
  take(d.pose_f, 24);
  take(d.pose_r, 24);
  take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  take(d.part, (size_t)kAlRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = L.size;
  return d;
}

size_t icp_pixels(const tf_volume* v) { const AlignCam c = align_cam(v); return (size_t)c.W * (size_t)c.H; }

// first use, or a larger camera since: the block sized for the camera at stride 1
int icp_ensure(tf_volume* v, IcpDev* d) {
  const AlignCam c = align_cam(v);
  const size_t tiles = (size_t)((c.W + 7) / 8) * (size_t)((c.H + 7) / 8);
  AlignIcpState& s = v->align_icp;
  if (!s.block || s.cap_tiles < tiles) {
    size_t bytes = 0;
    icp_carve(nullptr, tiles, &bytes);
    if (s.block) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = s.block.alloc(bytes);
    if (rc) { s.cap_tiles = 0; return rc; }
    TF_HIP(hipMemsetAsync(s.block.p, 0, sizeof(IcpCtl), v->stream));
    s.cap_tiles = tiles;
  }
  *d = icp_carve(s.block.p, s.cap_tiles, nullptr);
  return TF_OK;
}

// the six map planes of the forms that raycast themselves: vertex [3][H][W], then normal [3][H][W]
int icp_ensure_maps(tf_volume* v, float** d_vertex, float** d_normal) {
  const size_t P = icp_pixels(v);
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
  return TF_OK;
}

IcpRowsArgs icp_rows_args(const tf_volume* v, const tf_align_icp_params& p, const float* d_depth, const float* d_vertex,
                          const float* d_normal, int level, uint32_t* n_tiles) {
  IcpRowsArgs a{};
  const tf_align_params& g = p.geo;
  const int s = g.stride[level < g.n_levels ? level : g.n_levels - 1];
  a.depth = d_depth; a.vm = d_vertex; a.nm = d_normal;
  const AlignCam c = align_cam(v);
  a.fx = c.fx; a.fy = c.fy; a.cxs = c.cx + 0.5f; a.cys = c.cy + 0.5f;
  a.W = c.W; a.H = c.H; a.stride = s; a.level = level;
  const int nx = (int)(((long long)a.W + s - 1) / s), ny = (int)(((long long)a.H + s - 1) / s);
  a.tiles_x = (nx + 7) / 8;
  *n_tiles = (uint32_t)a.tiles_x * (uint32_t)((ny + 7) / 8);  // <= the tiles at stride 1
  a.min_depth = g.min_depth; a.max_depth = g.max_depth; a.max_residual = g.max_residual; a.huber = g.huber;
  a.max_dist2 = p.max_distance * p.max_distance;
  a.plane = (size_t)a.W * a.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close
int icp_enqueue(tf_volume* v, const float* d_depth, const float* pose, const float* d_vertex, const float* d_normal,
                const float* model_pose, const tf_align_icp_params& p, tf_align_result* d_result) {
  IcpDev d;
  int rc = icp_ensure(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  IcpPoses P;
  memcpy(P.p, pose, sizeof(P.p));
  memcpy(P.m, model_pose, sizeof(P.m));
  hipLaunchKernelGGL(k_icp_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  const tf_align_params& g = p.geo;
  for (int l = 0; l <= g.n_levels; ++l) {
    const bool closing = l == g.n_levels;
    uint32_t n_tiles = 0;
    IcpRowsArgs ra = icp_rows_args(v, p, d_depth, d_vertex, d_normal, l, &n_tiles);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    IcpSolveArgs sa{};
    sa.level = l; sa.log_level = closing ? g.n_levels - 1 : l; sa.stride = ra.stride; sa.closing = closing;
    sa.last_level = l == g.n_levels - 1; sa.n_rows = (n_tiles + kAlWaves - 1) / kAlWaves;
    sa.damping = g.damping; sa.eps_t = g.eps_t; sa.eps_r = g.eps_r; sa.min_valid = g.min_valid; sa.out = d_result;
    const int n = closing ? 1 : g.iters[l];
    for (int it = 0; it < n; ++it) {
      hipLaunchKernelGGL(k_icp_rows, dim3(sa.n_rows), dim3(kAlWaves * 64), 0, st, ra);
      hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(256), 0, st, d, sa);
    }
  }
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int icp_residuals_enqueue(tf_volume* v, const float* d_depth, const float* pose, const float* d_vertex,
                          const float* d_normal, const float* model_pose, const tf_align_icp_params& p, float* d_r,
                          uint32_t* d_flags, int32_t* d_assoc) {
  IcpDev d;
  int rc = icp_ensure(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  uint32_t n_tiles = 0;
  IcpRowsArgs ra = icp_rows_args(v, p, d_depth, d_vertex, d_normal, 0, &n_tiles);
  ra.pose = d.pose_r; ra.r = d_r; ra.flags = d_flags; ra.assoc = d_assoc;
  if (ra.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
    if (d_assoc) TF_HIP(hipMemsetAsync(d_assoc, 0xFF, 4 * ra.plane, st));  // -1
  }
  IcpPoses P;
  memcpy(P.p, pose, sizeof(P.p));
  memcpy(P.m, model_pose, sizeof(P.m));
  hipLaunchKernelGGL(k_icp_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  hipLaunchKernelGGL(k_icp_rows, dim3((n_tiles + kAlWaves - 1) / kAlWaves), dim3(kAlWaves * 64), 0, st, ra);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// the model raycast at model_pose into the state block's own maps: tf_raycast_device's launch
int icp_raycast(tf_volume* v, const float* model_pose, const tf_align_icp_params& p, float** d_vertex, float** d_normal) {
  int rc = icp_ensure_maps(v, d_vertex, d_normal);
  if (rc) return rc;
  return tf_raycast_device(v, model_pose, p.ray_near, p.ray_far, p.ray_max_steps, nullptr, *d_normal, nullptr, *d_vertex);
}

}  // namespace

void align_icp_release(tf_volume* v) { v->align_icp = AlignIcpState{}; }

int track_check(tf_volume* v, const float* depth, const float* pose, const tf_align_icp_params* icp_params,
                const tf_align_params* sdf_params) {
  const int rc = icp_check(v, depth, pose, nullptr, icp_params, true, true);
  return rc ? rc : align_check(v, depth, pose, sdf_params, true);
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
  const size_t P = icp_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_r = L.take(sizeof(tf_align_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  float *d_v = nullptr, *d_n = nullptr;
  if ((rc = icp_raycast(v, mp, *params, &d_v, &d_n))) return rc;
  if ((rc = icp_enqueue(v, sg.dp<const float>(o_d), pose, d_v, d_n, mp, *params, sg.dp<tf_align_result>(o_r)))) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, sizeof(tf_align_result), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(result, sg.h + o_r, sizeof(tf_align_result));
  return TF_OK;
}

int tf_align_icp_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v || !n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  if (!v->align_icp.block) return TF_OK;
  const IcpDev d = icp_carve(v->align_icp.block.p, v->align_icp.cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  IcpCtl c;
  TF_HIP(hipMemcpy(&c, d.ctl, sizeof(c), hipMemcpyDeviceToHost));
  const int64_t have = c.n_eval < 0 ? 0 : (c.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : c.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0) TF_HIP(hipMemcpy(out, d.log, (size_t)m * sizeof(tf_align_iter), hipMemcpyDeviceToHost));
  return TF_OK;
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
  const size_t P = icp_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_v = L.take(own ? 0 : 12 * P), o_n = L.take(own ? 0 : 12 * P);
  const size_t o_r = L.take(r ? 4 * P : 0), o_f = L.take(flags ? 4 * P : 0), o_a = L.take(assoc ? 4 * P : 0);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  float *d_v = nullptr, *d_n = nullptr;
  if (own) {
    if ((rc = icp_raycast(v, mp, *params, &d_v, &d_n))) return rc;
  } else {
    if ((rc = stage_in(v, sg, o_v, model_vertex, 12 * P)) || (rc = stage_in(v, sg, o_n, model_normal, 12 * P))) return rc;
    d_v = sg.dp<float>(o_v); d_n = sg.dp<float>(o_n);
  }
  rc = icp_residuals_enqueue(v, sg.dp<const float>(o_d), pose, d_v, d_n, mp, *params, r ? sg.dp<float>(o_r) : nullptr,
                             flags ? sg.dp<uint32_t>(o_f) : nullptr, assoc ? sg.dp<int32_t>(o_a) : nullptr);
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, L.size - o_r, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
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
