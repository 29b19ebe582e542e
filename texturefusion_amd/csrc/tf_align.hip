// tf_align.hip -- frame-to-model alignment: the pose at which a depth frame lies on the fused surface, found on the device
// with no host synchronisation inside a call (the step GCFusion/MobileFusion.cpp:322 leaves commented out; the reference
// has no body for it, so the method and its order of operations are defined here and restated in tests/align_ref.py).
//
//   k_align_begin  one lane: the caller's pose into the state block (f64 and f32), the control words cleared
//   k_align_rows   one wave per 8 x 8 tile of SAMPLED pixels (lane = 8 y + x, a tile spans 8 * stride image pixels), eight
//                  waves per workgroup:
//                  residual, gradient, Jacobian and the wave's share of the normal equations; with map outputs, the
//                  residual map of tf_align_residuals -- one body
//   k_align_solve  one workgroup: the partials combined in tile order, the 6 x 6 solve and the pose update by one lane
//                  (tf_align_solve.h), a log record, the result
//
// Per sampled pixel (x, y), all f32, every operation rounded on its own (-ffp-contract=off):
//   z = depth[y][x], in range iff finite and min_depth <= z <= max_depth                                       (bit 0)
//   dcx = ((float)x - cxs) / fx, dcy = ((float)y - cys) / fy with the int-truncated intrinsics, cxs = cx + 0.5, cys = cy + 0.5
//   pc = (dcx * z, dcy * z, z);  q_r = (R[r][0] * pc.x + R[r][1] * pc.y) + R[r][2] * pc.z;  pw = t + q
//   s = tri_sample<false>(pw)                                                                                  (bit 1)
//   sm_a = tri_sample<false>(pw - res e_a), sp_a = tri_sample<false>(pw + res e_a), a = x, y, z                (bit 2: all six)
//   g_a = (sp_a - sm_a) * (0.5f / res);  |s| <= max_residual                                                   (bit 3)
//   each bit is set only where the lower ones are; the pixel is valid iff all four are.  r = s.
//   J = (g.x, g.y, g.z, q.y g.z - q.z g.y, q.z g.x - q.x g.z, q.x g.y - q.y g.x)
//   w = 1 if huber == 0 or |r| <= huber, else huber / |r|;  wJ_i = w * J_i,  wr = w * r  (f32)
// Sums over the valid pixels, every term a product of two f32 values taken in f64 (exact), accumulated in f64:
//   A_ij = sum (double)wJ_i * (double)J_j (i <= j, the 21 upper entries row by row),  b_i = sum (double)wJ_i * (double)r,
//   sum_r2 = sum (double)r * (double)r,  sum_wr2 = sum (double)wr * (double)r,  n_valid, n_sampled (pixels inside the image)
// Order of summation, a function of (W, H, stride) alone: the 64 lanes of a tile by the tree of ccd_wave_sum (xor 32,
// 16, .. 1; each node computed by one lane, tf_align_tree.h), the eight tiles of a workgroup in wave order, one plain-stored
// row per workgroup; in k_align_solve eight threads per sum add the rows g, g + 8, g + 16, .. in ascending order (g = 0..7),
// then the eight in order.
// No atomics, no counters, no polling: the launch boundary between k_align_rows and k_align_solve is the only hand-off.
// Every launch of a call is enqueued up front; a launch first reads the state word (bit 0: stopped, bits 8..: levels that
// are finished) and returns if it has nothing to do.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <type_traits>

#include "tf_align_solve.h"
#include "tf_align_tree.h"
#include "tf_ray_devfn.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

constexpr int kAlignMaxIters = 64;

struct AlignCtl {
  uint32_t state;  // bit 0: stopped (too few / singular), bits 8..: levels finished
  int32_t status;
  int32_t n_eval;
  int32_t n_valid_first;
  float rms_first;
  uint32_t pad[3];
};
struct AlignDev {
  AlignCtl* ctl;
  double* pose_d;       // [12] the pose between iterations
  float* pose_f;        // [12] the same rounded: what k_align_rows samples at
  float* pose_r;        // [12] tf_align_residuals' pose (the last alignment's state stays as it is)
  double* part;         // [ceil(cap_tiles / kAlWaves)][kAlRow]: a row per workgroup of k_align_rows
  tf_align_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
  uint32_t cap_tiles;   // tiles of the camera at stride 1
};
struct AlignPose { float p[12]; };

struct AlignRowsArgs {
  const float* depth;
  const float* pose;      // 12 floats in the state block
  const uint32_t* state;  // null: always run (tf_align_residuals)
  float fx, fy, cxs, cys;
  int W, H, tiles_x, stride, level;
  float min_depth, max_depth, max_residual, huber, res;
  size_t plane;
  float* r;
  float* grad;
  uint32_t* flags;
  double* part;  // null: no sums
};
struct AlignSolveArgs {
  int level, log_level, stride, closing, last_level;
  uint32_t n_rows;  // workgroups of the rows launch
  float damping, eps_t, eps_r;
  int min_valid;
  tf_align_result* out;
};

__device__ __forceinline__ bool al_idle(const uint32_t* state, int level) {
  const uint32_t st = *state;
  return (st & 1u) || (uint32_t)level < (st >> 8);
}
__global__ __launch_bounds__(64) void k_align_begin(AlignDev d, AlignPose p, int residuals_only) {
  const int i = threadIdx.x;
  if (residuals_only) {
    if (i < 12) d.pose_r[i] = p.p[i];
    return;
  }
  if (i < 12) { d.pose_d[i] = (double)p.p[i]; d.pose_f[i] = p.p[i]; }
  if (i == 0) {
    AlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    *d.ctl = c;
  }
}

// (80 VGPRs, six waves per SIMD, no private memory: tests/test_kernel_resources_align.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_align_rows(VolumeDev v, AlignRowsArgs a) {
  if (a.state && al_idle(a.state, a.level)) return;
  // (a tile beyond the last one of the level lies below the image: none of its lanes is inside)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kAlWaves + wave;
  const long long X = (long long)((tile % a.tiles_x) * 8 + (lane & 7)) * a.stride;
  const long long Y = (long long)((tile / a.tiles_x) * 8 + (lane >> 3)) * a.stride;
  const bool in = X < a.W && Y < a.H;
  uint32_t fl = 0;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  if (in) {
    const size_t o = (size_t)Y * a.W + (size_t)X;
    const float z = a.depth[o];
    if (isfinite(z) && z >= a.min_depth && z <= a.max_depth) {
      fl = 1u;
      const float res = a.res, ir = 1.0f / res;
      const float dcx = ((float)(int)X - a.cxs) / a.fx, dcy = ((float)(int)Y - a.cys) / a.fy;
      const float pcx = dcx * z, pcy = dcy * z;
      const float* P = a.pose;
      qx = (P[0] * pcx + P[1] * pcy) + P[2] * z;
      qy = (P[4] * pcx + P[5] * pcy) + P[6] * z;
      qz = (P[8] * pcx + P[9] * pcy) + P[10] * z;
      const float wx = P[3] + qx, wy = P[7] + qy, wz = P[11] + qz;
      ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
      float sc = 0.f;
      if (tri_sample<false>(v, cc, wx, wy, wz, ir, &sc)) {
        fl |= 2u;
        s = sc;
        // tap k: axis k >> 1, minus / plus by k & 1 (as the raycaster's normal; no one-sided fallback here)
        float sp0 = 0.f, sp1 = 0.f, sp2 = 0.f, sm0 = 0.f, sm1 = 0.f, sm2 = 0.f;
        bool ok = true;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
          const int ax = k >> 1;
          float t = 0.f;
          const float h = (k & 1) ? res : -res;  // (a + (-b) is a - b)
          ChunkCache ct = cc;  // every tap starts from the centre's chunk: a tap that leaves it costs one probe, none to come back
          const bool okk = tri_sample<false>(v, ct, ax == 0 ? wx + h : wx, ax == 1 ? wy + h : wy, ax == 2 ? wz + h : wz, ir, &t);
          ok = ok && okk;
          if (k == 0) sm0 = t; else if (k == 1) sp0 = t; else if (k == 2) sm1 = t; else if (k == 3) sp1 = t;
          else if (k == 4) sm2 = t; else sp2 = t;
        }
        if (ok) {
          fl |= 4u;
          const float h2 = 0.5f / res;
          gx = (sp0 - sm0) * h2; gy = (sp1 - sm1) * h2; gz = (sp2 - sm2) * h2;
          if (fabsf(s) <= a.max_residual) fl |= 8u;
        }
      }
    }
    if (a.r) a.r[o] = s;
    if (a.grad) { a.grad[o] = gx; a.grad[a.plane + o] = gy; a.grad[2 * a.plane + o] = gz; }
    if (a.flags) a.flags[o] = fl;
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

__global__ __launch_bounds__(256) void k_align_solve(AlignDev d, AlignSolveArgs a) {
  if (al_idle(&d.ctl->state, a.level)) return;
  // thread (e = tid & 31, g = tid >> 5) adds entry e of the rows g, g + 8, g + 16, .. in ascending order (a row's 32
  // entries lie side by side: the 32 threads of a group read one 256-byte row); then the eight groups in order
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
  AlignCtl c = *d.ctl;
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

// the state block as it lies in AlignState::block (base == null: its size)
AlignDev align_carve(void* base, size_t cap_tiles, size_t* bytes) {
  AlignDev d{};
  d.cap_tiles = (uint32_t)cap_tiles;
  Layout L;
  uint8_t* b = static_cast<uint8_t*>(base);
  const auto take = [&](auto*& p, size_t count) {
    const size_t at = L.take(count * sizeof(*p));
    p = b ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + at) : nullptr;
  };
  take(d.ctl, 1);
  take(d.pose_d, 12);
  take(d.pose_f, 12);
  take(d.pose_r, 12);
  take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  take(d.part, (size_t)kAlRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = L.size;
  return d;
}

size_t align_pixels(const tf_volume* v) { const AlignCam c = align_cam(v); return (size_t)c.W * (size_t)c.H; }
size_t align_tiles(const tf_volume* v) {
  const AlignCam c = align_cam(v);
  return (size_t)((c.W + 7) / 8) * (size_t)((c.H + 7) / 8);
}

// first use, or a larger camera since: the block sized for the camera at stride 1
int align_ensure(tf_volume* v, AlignDev* d) {
  const size_t tiles = align_tiles(v);
  if (!v->align.block || v->align.cap_tiles < tiles) {
    size_t bytes = 0;
    align_carve(nullptr, tiles, &bytes);
    if (v->align.block) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = v->align.block.alloc(bytes);
    if (rc) { v->align.cap_tiles = 0; return rc; }
    TF_HIP(hipMemsetAsync(v->align.block.p, 0, sizeof(AlignCtl), v->stream));
    v->align.cap_tiles = tiles;
  }
  *d = align_carve(v->align.block.p, v->align.cap_tiles, nullptr);
  return TF_OK;
}

}  // namespace

// shared with tf_align_color.hip (tf_volume.h): the camera and the checks of a call's arguments
// the camera of the depth image: the one tf_raycast_camera set (any size), else the handle's -- as the raycaster's
AlignCam align_cam(const tf_volume* v) {
  if (v->ray_w > 0) return {v->ray_fx, v->ray_fy, v->ray_cx, v->ray_cy, v->ray_w, v->ray_h};
  return {v->cam.fxi, v->cam.fyi, v->cam.cxi, v->cam.cyi, v->cam.W, v->cam.H};
}

bool finite_all(const float* p, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(p[i])) return false;
  return true;
}

int align_check(tf_volume* v, const float* depth, const float* pose, const tf_align_params* p, bool with_iters) {
  if (!v || !depth || !pose || !p) { set_error("null argument"); return TF_ERR_INVALID; }
  if (p->n_levels < 1 || p->n_levels > 4) { set_error("align: n_levels must be 1..4"); return TF_ERR_INVALID; }
  int sum = 0;
  for (int l = 0; l < p->n_levels; ++l) {
    if (p->stride[l] < 1) { set_error("align: stride must be >= 1"); return TF_ERR_INVALID; }
    if (with_iters) {
      if (p->iters[l] < 0 || p->iters[l] > kAlignMaxIters) { set_error("align: iters must be 0..64"); return TF_ERR_INVALID; }
      sum += p->iters[l];
    }
  }
  if (sum > kAlignMaxIters) { set_error("align: more than 64 iterations in all"); return TF_ERR_INVALID; }
  const float f[7] = {p->min_depth, p->max_depth, p->max_residual, p->huber, p->damping, p->eps_t, p->eps_r};
  if (!finite_all(f, 7)) { set_error("align: a parameter is not finite"); return TF_ERR_INVALID; }
  if (!finite_all(pose, 12)) { set_error("pose is not finite"); return TF_ERR_INVALID; }
  if (p->min_depth > p->max_depth) { set_error("align: min_depth > max_depth"); return TF_ERR_INVALID; }
  if (p->huber < 0.f || p->damping < 0.f || p->eps_t < 0.f || p->eps_r < 0.f) {
    set_error("align: huber, damping, eps_t, eps_r must be >= 0");
    return TF_ERR_INVALID;
  }
  const AlignCam c = align_cam(v);
  if (c.W <= 0 || c.H <= 0 || !(c.fx > 0.f) || !(c.fy > 0.f)) {
    set_error("no camera (tf_set_camera / tf_raycast_camera)");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

namespace {

AlignRowsArgs rows_args(const tf_volume* v, const AlignDev& d, const tf_align_params& p, const float* d_depth, int level,
                        uint32_t* n_tiles) {
  AlignRowsArgs a{};
  const int s = p.stride[level < p.n_levels ? level : p.n_levels - 1];
  a.depth = d_depth;
  const AlignCam c = align_cam(v);
  a.fx = c.fx; a.fy = c.fy; a.cxs = c.cx + 0.5f; a.cys = c.cy + 0.5f;
  a.W = c.W; a.H = c.H; a.stride = s; a.level = level;
  const int nx = (int)(((long long)a.W + s - 1) / s), ny = (int)(((long long)a.H + s - 1) / s);
  a.tiles_x = (nx + 7) / 8;
  *n_tiles = (uint32_t)a.tiles_x * (uint32_t)((ny + 7) / 8);  // <= the tiles at stride 1
  a.min_depth = p.min_depth; a.max_depth = p.max_depth; a.max_residual = p.max_residual; a.huber = p.huber; a.res = v->res;
  a.plane = (size_t)a.W * a.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close
int align_enqueue(tf_volume* v, const float* d_depth, const float* pose, const tf_align_params& p, tf_align_result* d_result) {
  AlignDev d;
  int rc = align_ensure(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  AlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  hipLaunchKernelGGL(k_align_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  for (int l = 0; l <= p.n_levels; ++l) {
    const bool closing = l == p.n_levels;
    uint32_t n_tiles = 0;
    AlignRowsArgs ra = rows_args(v, d, p, d_depth, l, &n_tiles);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    AlignSolveArgs sa{};
    sa.level = l; sa.log_level = closing ? p.n_levels - 1 : l; sa.stride = ra.stride; sa.closing = closing;
    sa.last_level = l == p.n_levels - 1; sa.n_rows = (n_tiles + kAlWaves - 1) / kAlWaves;
    sa.damping = p.damping; sa.eps_t = p.eps_t; sa.eps_r = p.eps_r; sa.min_valid = p.min_valid; sa.out = d_result;
    const int n = closing ? 1 : p.iters[l];
    for (int it = 0; it < n; ++it) {
      hipLaunchKernelGGL(k_align_rows, dim3((n_tiles + kAlWaves - 1) / kAlWaves), dim3(kAlWaves * 64), 0, st, v->dev, ra);
      hipLaunchKernelGGL(k_align_solve, dim3(1), dim3(256), 0, st, d, sa);
    }
  }
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int residuals_enqueue(tf_volume* v, const float* d_depth, const float* pose, const tf_align_params& p, float* d_r,
                      float* d_grad3, uint32_t* d_flags) {
  AlignDev d;
  int rc = align_ensure(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  uint32_t n_tiles = 0;
  AlignRowsArgs ra = rows_args(v, d, p, d_depth, 0, &n_tiles);
  ra.pose = d.pose_r; ra.r = d_r; ra.grad = d_grad3; ra.flags = d_flags;
  if (ra.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_grad3) TF_HIP(hipMemsetAsync(d_grad3, 0, 12 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
  }
  AlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  hipLaunchKernelGGL(k_align_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  hipLaunchKernelGGL(k_align_rows, dim3((n_tiles + kAlWaves - 1) / kAlWaves), dim3(kAlWaves * 64), 0, st, v->dev, ra);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

void align_release(tf_volume* v) { v->align = AlignState{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_default_params(tf_align_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_align_params p{};
  p.n_levels = 3;
  p.stride[0] = 4; p.stride[1] = 2; p.stride[2] = 1; p.stride[3] = 1;
  p.iters[0] = 4; p.iters[1] = 3; p.iters[2] = 2; p.iters[3] = 0;
  p.min_depth = 0.05f; p.max_depth = 5.0f; p.max_residual = 0.03f; p.huber = 0.01f; p.damping = 0.f;
  p.eps_t = 1e-5f; p.eps_r = 1e-5f;
  p.min_valid = 100;
  *out = p;
  return TF_OK;
}

int tf_align_frame_device(tf_volume* v, const float* d_depth, const float pose[12], const tf_align_params* params,
                          tf_align_result* d_result) {
  int rc = align_check(v, d_depth, pose, params, true);
  if (rc) return rc;
  if (!d_result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  return align_enqueue(v, d_depth, pose, *params, d_result);
}

int tf_align_frame(tf_volume* v, const float* depth, const float pose[12], const tf_align_params* params,
                   tf_align_result* result) {
  int rc = align_check(v, depth, pose, params, true);
  if (rc) return rc;
  if (!result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_r = L.take(sizeof(tf_align_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  if ((rc = align_enqueue(v, sg.dp<const float>(o_d), pose, *params, sg.dp<tf_align_result>(o_r)))) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, sizeof(tf_align_result), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(result, sg.h + o_r, sizeof(tf_align_result));
  return TF_OK;
}

int tf_align_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v || !n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  if (!v->align.block) return TF_OK;
  const AlignDev d = align_carve(v->align.block.p, v->align.cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  AlignCtl c;
  TF_HIP(hipMemcpy(&c, d.ctl, sizeof(c), hipMemcpyDeviceToHost));
  const int64_t have = c.n_eval < 0 ? 0 : (c.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : c.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0) TF_HIP(hipMemcpy(out, d.log, (size_t)m * sizeof(tf_align_iter), hipMemcpyDeviceToHost));
  return TF_OK;
}

int tf_align_residuals_device(tf_volume* v, const float* d_depth, const float pose[12], const tf_align_params* params,
                              float* d_r, float* d_grad3, uint32_t* d_flags) {
  int rc = align_check(v, d_depth, pose, params, false);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (!d_r && !d_grad3 && !d_flags) return TF_OK;
  return residuals_enqueue(v, d_depth, pose, *params, d_r, d_grad3, d_flags);
}

int tf_align_residuals(tf_volume* v, const float* depth, const float pose[12], const tf_align_params* params, float* r,
                       float* grad3, uint32_t* flags) {
  int rc = align_check(v, depth, pose, params, false);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (!r && !grad3 && !flags) return TF_OK;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_r = L.take(r ? 4 * P : 0), o_g = L.take(grad3 ? 12 * P : 0), o_f = L.take(flags ? 4 * P : 0);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  rc = residuals_enqueue(v, sg.dp<const float>(o_d), pose, *params, r ? sg.dp<float>(o_r) : nullptr,
                         grad3 ? sg.dp<float>(o_g) : nullptr, flags ? sg.dp<uint32_t>(o_f) : nullptr);
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, L.size - o_r, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (grad3) memcpy(grad3, sg.h + o_g, 12 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  return TF_OK;
}

}  // extern "C"
