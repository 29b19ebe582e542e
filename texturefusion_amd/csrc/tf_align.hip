// tf_align.hip -- frame-to-model alignment: the pose at which a depth frame lies on the fused surface, found on the device
// with no host synchronisation inside a call (the step GCFusion/MobileFusion.cpp:322 leaves commented out; the reference
// has no body for it, so the method and its order of operations are defined here and restated in tests/align_ref.py).
//
//   k_align_begin  one lane: the caller's pose into the state block (f64 and f32), the control words cleared
//   k_stage2_start k_align_begin for a call chained behind another aligner's on the stream: the start is that call's result
//                  pose, read on the device, where its status holds (the device tracker, tf_devpose.hip)
//   k_align_rows   one wave per 8 x 8 tile of SAMPLED pixels (lane = 8 y + x, a tile spans 8 * stride image pixels), eight
//                  waves per workgroup:
//                  residual, gradient, Jacobian and the wave's share of the normal equations; with map outputs, the
//                  residual map of tf_align_residuals -- one body
//   k_align_solve  one workgroup: the partials combined in tile order, the 6 x 6 solve and the pose update by one lane
//                  (tf_align_solve.h), a log record, the result
// The kernels are calls into tf_align_rows.h, the machinery all four aligners share; what is this file's own is the row of
// a pixel as stated below (al_sdf_row), and the host side every aligner uses (tf_volume.h: align_cam .. align_log).
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
// Order of summation, a function of (W, H, stride) alone, and the stop rules: tf_align_rows.h's header (the tree of
// tf_align_tree.h per tile, the eight tiles of a workgroup in wave order, the rows g, g + 8, .. ascending, then the eight).
// No atomics, no counters, no polling: the launch boundary between k_align_rows and k_align_solve is the only hand-off.
// Every launch of a call is enqueued up front; a launch first reads the state word and returns if it has nothing to do.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_rows.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

constexpr int kAlignMaxIters = 64;

struct AlignDev {
  AlignCtl* ctl;
  double* pose_d;       // [12] the pose between iterations
  float* pose_f;        // [12] the same rounded: what k_align_rows samples at
  float* pose_r;        // [12] tf_align_residuals' pose (the last alignment's state stays as it is)
  double* part;         // [ceil(cap_tiles / kAlWaves)][kAlRow]: a row per workgroup of k_align_rows
  tf_align_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
};

struct AlignRowsArgs {
  AlignRowsCommon c;
  const float* depth;
  const float* pose;      // 12 floats in the state block
  const uint32_t* state;  // null: always run (tf_align_residuals)
  float res;
  size_t plane;
  float* r;
  float* grad;
  uint32_t* flags;
  double* part;  // null: no sums
};
struct AlignSolveArgs {
  AlignSolveCommon c;
  tf_align_result* out;
};

__global__ __launch_bounds__(64) void k_align_begin(AlignDev d, AlignPose p, int residuals_only) {
  al_begin(d.ctl, d.pose_d, d.pose_f, d.pose_r, p, residuals_only);
}

// The begin launch of a call that follows another aligner's on the stream, as the second stage of the device tracker does
// (tf_devpose.hip): the start is the f32 pose of that call's result, read from device memory.  It runs only where that
// call's status holds (0 <= *prev_status <= TF_ALIGN_MAX_ITERS).  Otherwise bit 0 of the state word stops every launch of
// this call: the result is not written and the log stays the last call's.
__global__ __launch_bounds__(64) void k_stage2_start(AlignDev d, const int32_t* __restrict__ prev_status,
                                                     const AlignPose* __restrict__ prev_pose) {
  const int32_t s = *prev_status;
  if (!(s >= 0 && s <= TF_ALIGN_MAX_ITERS)) {
    if (threadIdx.x == 0) d.ctl->state |= 1u;
    return;
  }
  al_begin(d.ctl, d.pose_d, d.pose_f, d.pose_r, *prev_pose, 0);
}

// (six waves per SIMD, no private memory: tests/test_kernel_resources_align.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_align_rows(VolumeDev v, AlignRowsArgs a) {
  if (a.state && al_idle(a.state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  AlSdfRow row{};
  if (px.in) {
    const size_t o = (size_t)px.Y * a.c.W + (size_t)px.X;
    row = al_sdf_row<false>(v, a.c, a.res, px, a.depth[o], a.pose);
    if (a.r) a.r[o] = row.s;
    if (a.grad) { a.grad[o] = row.gx; a.grad[a.plane + o] = row.gy; a.grad[2 * a.plane + o] = row.gz; }
    if (a.flags) a.flags[o] = row.fl;
  }
  if (!a.part) return;
  __shared__ double wsum[kAlWaves][kAlRow];
  al_row_sums(wsum, 0, px, row.gx, row.gy, row.gz, row.qx, row.qy, row.qz, row.s, a.c.huber, row.fl == 15u, px.in);
  al_store_rows(wsum, a.part + (size_t)blockIdx.x * kAlRow);
}

__global__ __launch_bounds__(256) void k_align_solve(AlignDev d, AlignSolveArgs a) {
  al_solve_pose(d.ctl, d.log, d.pose_d, d.pose_f, d.part, a.c, a.out);
}

// the state block as it lies in tf_volume::align (base == null: its size)
AlignDev align_carve(void* base, size_t cap_tiles, size_t* bytes) {
  AlignDev d{};
  Carver c(base);
  c.take(d.ctl, 1);
  c.take(d.pose_d, 12);
  c.take(d.pose_f, 12);
  c.take(d.pose_r, 12);
  c.take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kAlRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = c.L.size;
  return d;
}
int align_dev(tf_volume* v, AlignDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; align_carve(nullptr, tiles, &n); return n; };
  const int rc = align_ensure(v, v->align, bytes_of, sizeof(AlignCtl));
  if (rc) return rc;
  *d = align_carve(v->align.block.p, v->align.cap_tiles, nullptr);
  return TF_OK;
}

}  // namespace

// ---- what the four aligners' host sides share (tf_volume.h) ----

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

size_t align_pixels(const tf_volume* v) { const AlignCam c = align_cam(v); return (size_t)c.W * (size_t)c.H; }
size_t align_tiles(const tf_volume* v) {
  const AlignCam c = align_cam(v);
  return (size_t)((c.W + 7) / 8) * (size_t)((c.H + 7) / 8);
}

int align_ensure(tf_volume* v, AlignBlock& b, size_t (*bytes_of)(size_t tiles), size_t clear_bytes) {
  const size_t tiles = align_tiles(v);
  if (b.block && b.cap_tiles >= tiles) return TF_OK;
  if (b.block) TF_HIP(hipStreamSynchronize(v->stream));
  const int rc = b.block.alloc(bytes_of(tiles));
  if (rc) { b.cap_tiles = 0; return rc; }
  TF_HIP(hipMemsetAsync(b.block.p, 0, clear_bytes, v->stream));
  b.cap_tiles = tiles;
  return TF_OK;
}

namespace {
// a level's blocks: the rows walk an image of camera c at rows_stride, the solve's block names block_stride
void level_fill(const AlignCam& c, int rows_stride, int block_stride, const tf_align_params& p, int level, AlignRowsCommon* rc,
                AlignSolveCommon* sc) {
  const bool closing = level == p.n_levels;
  const int s = rows_stride;
  AlignRowsCommon r{};
  r.fx = c.fx; r.fy = c.fy; r.cxs = c.cx + 0.5f; r.cys = c.cy + 0.5f;
  r.W = c.W; r.H = c.H; r.stride = s; r.level = level;
  const int nx = (int)(((long long)r.W + s - 1) / s), ny = (int)(((long long)r.H + s - 1) / s);
  r.tiles_x = (nx + 7) / 8;
  const uint32_t n_tiles = (uint32_t)r.tiles_x * (uint32_t)((ny + 7) / 8);  // <= the tiles at stride 1
  r.min_depth = p.min_depth; r.max_depth = p.max_depth; r.max_residual = p.max_residual; r.huber = p.huber;
  AlignSolveCommon q{};
  q.level = level; q.log_level = closing ? p.n_levels - 1 : level; q.stride = block_stride; q.closing = closing;
  q.last_level = level == p.n_levels - 1; q.n_rows = (n_tiles + kAlWaves - 1) / kAlWaves;
  q.damping = p.damping; q.eps_t = p.eps_t; q.eps_r = p.eps_r; q.min_valid = p.min_valid;
  *rc = r;
  *sc = q;
}
int level_stride(const tf_align_params& p, int level) { return p.stride[level == p.n_levels ? p.n_levels - 1 : level]; }
}  // namespace

void align_level(const tf_volume* v, const tf_align_params& p, int level, AlignRowsCommon* rc, AlignSolveCommon* sc) {
  const int s = level_stride(p, level);
  level_fill(align_cam(v), s, s, p, level, rc, sc);
}

void align_level_image(const AlignCam& cam, const tf_align_params& p, int level, AlignRowsCommon* rc, AlignSolveCommon* sc) {
  level_fill(cam, 1, level_stride(p, level), p, level, rc, sc);
}

void align_walk(const tf_volume* v, const tf_align_params& p,
                const std::function<void(const AlignRowsCommon&, const AlignSolveCommon&)>& evaluate,
                const AlignCam* level_cams) {
  for (int l = 0; l <= p.n_levels; ++l) {
    AlignRowsCommon rc;
    AlignSolveCommon sc;
    if (level_cams) align_level_image(level_cams[__builtin_ctz((unsigned)level_stride(p, l))], p, l, &rc, &sc);
    else align_level(v, p, l, &rc, &sc);
    const int n = sc.closing ? 1 : p.iters[l];
    for (int it = 0; it < n; ++it) evaluate(rc, sc);
  }
}

int align_log(tf_volume* v, const void* d_ctl, const void* d_log, size_t rec_bytes, void* out, int64_t cap, int64_t* n) {
  if (!n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  if (!d_ctl) return TF_OK;
  TF_HIP(hipStreamSynchronize(v->stream));
  AlignCtl c;
  TF_HIP(hipMemcpy(&c, d_ctl, sizeof(c), hipMemcpyDeviceToHost));
  const int64_t have = c.n_eval < 0 ? 0 : (c.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : c.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0) TF_HIP(hipMemcpy(out, d_log, (size_t)m * rec_bytes, hipMemcpyDeviceToHost));
  return TF_OK;
}

int stage_out(tf_volume* v, const Stage& st, size_t at, size_t bytes, void* out) {
  TF_HIP(hipMemcpyAsync(st.h + at, st.d + at, bytes, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (out) memcpy(out, st.h + at, bytes);
  return TF_OK;
}

void align_release(tf_volume* v) { v->align = AlignBlock{}; }

namespace {

AlignRowsArgs rows_args(const tf_volume* v, const AlignRowsCommon& rc, const float* d_depth) {
  AlignRowsArgs a{};
  a.c = rc;
  a.depth = d_depth;
  a.res = v->res;
  a.plane = (size_t)rc.W * rc.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close.  d_prev_status != null: the
// start is the pose at d_prev_pose, read on the device, where that status holds (k_stage2_start; pose is not read).
int align_enqueue(tf_volume* v, const float* d_depth, const float* pose, const tf_align_params& p, tf_align_result* d_result,
                  const int32_t* d_prev_status = nullptr, const float* d_prev_pose = nullptr) {
  AlignDev d;
  int rc = align_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  if (d_prev_status) {
    hipLaunchKernelGGL(k_stage2_start, dim3(1), dim3(64), 0, st, d, d_prev_status, reinterpret_cast<const AlignPose*>(d_prev_pose));
  } else {
    AlignPose P;
    memcpy(P.p, pose, sizeof(P.p));
    hipLaunchKernelGGL(k_align_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  }
  align_walk(v, p, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    AlignRowsArgs ra = rows_args(v, c, d_depth);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    hipLaunchKernelGGL(k_align_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra);
    hipLaunchKernelGGL(k_align_solve, dim3(1), dim3(256), 0, st, d, AlignSolveArgs{sc, d_result});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int residuals_enqueue(tf_volume* v, const float* d_depth, const float* pose, const tf_align_params& p, float* d_r,
                      float* d_grad3, uint32_t* d_flags) {
  AlignDev d;
  int rc = align_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  AlignRowsCommon c;
  AlignSolveCommon sc;
  align_level(v, p, 0, &c, &sc);
  AlignRowsArgs ra = rows_args(v, c, d_depth);
  ra.pose = d.pose_r; ra.r = d_r; ra.grad = d_grad3; ra.flags = d_flags;
  if (c.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_grad3) TF_HIP(hipMemsetAsync(d_grad3, 0, 12 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
  }
  AlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  hipLaunchKernelGGL(k_align_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  hipLaunchKernelGGL(k_align_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

// tf_align_frame_device from the 12 floats at d_prev_pose where *d_prev_status holds, all enqueued (tf_devpose.hip; the
// caller has checked)
int track_sdf_posed(tf_volume* v, const float* d_depth, const int32_t* d_prev_status, const float* d_prev_pose,
                    const tf_align_params& p, tf_align_result* d_result) {
  return align_enqueue(v, d_depth, nullptr, p, d_result, d_prev_status, d_prev_pose);
}

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
  return stage_out(v, sg, o_r, sizeof(tf_align_result), result);
}

int tf_align_log(tf_volume* v, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  const AlignDev d = v->align.block ? align_carve(v->align.block.p, v->align.cap_tiles, nullptr) : AlignDev{};
  return align_log(v, d.ctl, d.log, sizeof(tf_align_iter), out, cap, n);
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
  if ((rc = stage_out(v, sg, o_r, L.size - o_r, nullptr))) return rc;
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (grad3) memcpy(grad3, sg.h + o_g, 12 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  return TF_OK;
}

}  // extern "C"
