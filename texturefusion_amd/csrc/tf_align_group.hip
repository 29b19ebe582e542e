// tf_align_group.hip -- a keyframe group aligned to the fused volume in one call: up to seven depth frames of one camera,
// partitioned into rigid bodies, every body's pose corrected by tf_align_frame's Gauss-Newton on the sum of its frames'
// normal equations (OptimizeKeyframeVoxelDomain at GCFusion/MobileFusion.cpp:322 for the group ReIntegrateKeyframe takes;
// the reference has no body for it, the method is this library's own and tests/align_group_ref.py restates it).
//
//   k_galign_begin  one workgroup: every frame's pose into the state block (f64 and f32), every body's control words
//                   cleared, the result cleared but for n_frames and n_bodies
//   k_galign_rows   grid (workgroups of a frame, frames): k_align_rows' tile for frame blockIdx.y -- one wave per 8 x 8 tile
//                   of sampled pixels, eight waves per workgroup, one plain-stored row of partial sums per workgroup
//   k_galign_solve  one workgroup per body: each of its frames' partials combined in tile order, frame after frame,
//                   the frames added in ascending order, the 6 x 6 solve by one lane (tf_align_solve.h), the update of
//                   every frame of the body (tf_align_group_solve.h), a log record, the result
//
// Per sampled pixel of frame k everything up to g, q and the flags is k_align_rows' row (al_sdf_row, tf_align_rows.h;
// tf_align.hip's header comment is the specification; -ffp-contract=off).  The one difference is the lever of the
// rotational part: the twist of a body is taken about its anchor's camera centre (the
// anchor is the body's first frame).
//   anchor:        J = [g, q x g]                                             -- tf_align_frame's row
//   another frame: a = (t_k - t_anchor) + q componentwise in f32, from the two f32 poses the rows are sampled at,
//                  J = (g.x, g.y, g.z, a.y g.z - a.z g.y, a.z g.x - a.x g.z, a.x g.y - a.y g.x)
//   w, wJ, wr as tf_align.hip's.
// Sums: a frame's 31 sums are formed by the functions k_align_rows and k_align_solve form them with (tf_align_rows.h); a body's
// sums are its frames' sums added in ascending frame order, starting from the first frame's.  A body of one frame has
// tf_align_frame's sums, steps, log and result bit for bit.
// Step of a body with anchor centre c (the anchor's t before the step), xi = -(A + damping diag A)^-1 b = (v, w),
// E = exp([w]x): every frame of the body gets R_k <- E R_k, t_k <- (c + E (t_k - c)) + v in f64 (align_update_about); for
// the anchor that is align_update.  Each frame's pose is carried in f64 and rounded to f32 for the rows.
// Stops are per body and follow tf_align_frame's rules with the body's total n_valid; a body that has stopped or finished
// a level costs the other bodies nothing but a workgroup that reads one word and returns.
// No atomics, no counters, no polling: every launch of a call is enqueued up front, 1 + 2 per evaluation as
// tf_align_frame; a workgroup first reads the state word of its body and returns if that body has nothing to do.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_group_solve.h"
#include "tf_align_rows.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

constexpr int kGaMax = TF_ALIGN_GROUP_MAX_FRAMES;
constexpr int kGaResultWords = (int)(sizeof(tf_align_group_result) / 4);
static_assert(sizeof(tf_align_group_result) % 4 == 0 && kGaResultWords <= 256 && 12 * kGaMax <= 256, "k_galign_begin");

struct GAlignDev {
  AlignCtl* ctl;                // [kGaMax], one per body
  double* pose_d;               // [kGaMax][12] every frame's pose between iterations
  float* pose_f;                // [kGaMax][12] the same rounded: what k_galign_rows samples at
  tf_align_group_result* res;   // the result of tf_align_unit_group (the other forms bring their own)
  tf_align_iter* log;           // [kGaMax][TF_ALIGN_MAX_EVALUATIONS], a body's records side by side
  double* part;                 // [kGaMax][rows_cap][kAlRow]: a row per workgroup of k_galign_rows
  uint32_t rows_cap;            // workgroups of a frame at stride 1
};
// the partition: body[k] of frame k, anchor[k] = the first frame of that body, first[b] = the anchor of body b
struct GAlignTable {
  int32_t n_frames, n_bodies;
  uint8_t body[8], anchor[8], first[8];
};
struct GAlignPoses { float p[kGaMax * 12]; };

struct GAlignRowsArgs {
  AlignRowsCommon c;
  const float* depth[kGaMax];
  GAlignTable tab;
  const float* pose;      // pose_f of the state block
  const AlignCtl* ctl;
  float res;
  double* part;
  uint32_t rows_cap;
};
struct GAlignSolveArgs {
  AlignSolveCommon c;  // n_rows: workgroups of a frame in the rows launch
  GAlignTable tab;
  tf_align_group_result* out;
};

__global__ __launch_bounds__(256) void k_galign_begin(GAlignDev d, GAlignPoses p, GAlignTable tab, tf_align_group_result* out) {
  const int i = threadIdx.x;
  if (i < 12 * tab.n_frames) { const float x = p.p[i]; d.pose_d[i] = (double)x; d.pose_f[i] = x; }
  if (i < kGaMax) {
    AlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    d.ctl[i] = c;
  }
  // n_frames and n_bodies are the result's first two words
  if (i < kGaResultWords) reinterpret_cast<int32_t*>(out)[i] = i == 0 ? tab.n_frames : (i == 1 ? tab.n_bodies : 0);
}

// (resources: tests/test_kernel_resources_align_group.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_galign_rows(VolumeDev v, GAlignRowsArgs a) {
  const int fk = blockIdx.y, fa = a.tab.anchor[fk];
  if (al_idle(&a.ctl[a.tab.body[fk]].state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  const float* P = a.pose + 12 * fk;
  AlSdfRow row{};
  if (px.in) row = al_sdf_row<false>(v, a.c, a.res, px, a.depth[fk][(size_t)px.Y * a.c.W + (size_t)px.X], P);
  // the lever: q for the anchor, (t_k - t_anchor) + q for a later frame of the body (uniform over the workgroup)
  float lx = row.qx, ly = row.qy, lz = row.qz;
  if (fa != fk) {
    const float* PA = a.pose + 12 * fa;
    lx = (P[3] - PA[3]) + row.qx; ly = (P[7] - PA[7]) + row.qy; lz = (P[11] - PA[11]) + row.qz;
  }
  __shared__ double wsum[kAlWaves][kAlRow];
  al_row_sums(wsum, 0, px, row.gx, row.gy, row.gz, lx, ly, lz, row.s, a.c.huber, row.fl == 15u, px.in);
  al_store_rows(wsum, a.part + ((size_t)fk * a.rows_cap + blockIdx.x) * kAlRow);
}

__global__ __launch_bounds__(256) void k_galign_solve(GAlignDev d, GAlignSolveArgs a) {
  const int body = blockIdx.x;
  AlignCtl* ctl = d.ctl + body;
  if (al_idle(&ctl->state, a.c.level)) return;
  const bool first_eval = ctl->n_eval == 0;  // (read by every thread ahead of the barriers; lane 0 writes behind them)
  // per frame of the body, in ascending order: the frame's rows through k_align_solve's additions, thread e then adds the
  // frame's sum to the body's.  (One frame after the other: seven accumulators side by side in one loop over the rows
  // were measured slower, 66 against 47 us for an evaluation of one frame at stride 1.)
  __shared__ double red[8][kAlRow];
  __shared__ double tot[kAlRow];
  const uint32_t tid = threadIdx.x;
  double sum = 0.0;
  bool have = false;
#pragma unroll 1
  for (int k = 0; k < a.tab.n_frames; ++k) {
    if (a.tab.body[k] != body) continue;
    al_add_rows(d.part + (size_t)k * d.rows_cap * kAlRow, a.c.n_rows, red);
    if (tid < (uint32_t)kAlSums) {
      const double t = al_total(red, (int)tid);
      sum = have ? sum + t : t;
      if (tid == (uint32_t)kAlNv) {
        a.out->frame_valid_last[k] = (int)t;
        if (first_eval) a.out->frame_valid_first[k] = (int)t;
      }
    }
    have = true;
    __syncthreads();
  }
  if (tid < (uint32_t)kAlRow) tot[tid] = sum;
  __syncthreads();
  if (tid != 0) return;
  AlignCtl c = *ctl;
  tf_align_iter* rec = al_record(d.log + (size_t)body * TF_ALIGN_MAX_EVALUATIONS, c);
  const int anchor = a.tab.first[body];
  const double* pa = d.pose_d + 12 * anchor;
  const double cen[3] = {pa[3], pa[7], pa[11]};
  double A[21], b[6], xi[6], E[9];
  const AlEval ev = al_fill_iter(rec, a.c, [&](int i) { return tot[i]; }, pa, A, b);
  al_count(c, ev);
  const bool step = al_decide(c, a.c, ev.n_valid, A, b, rec, xi);
  if (step) align_rodrigues(xi + 3, E);
  *ctl = c;
  tf_align_result* out = a.out->body + body;
  al_fill_result(out, c, ev);
  // every frame of the body: the step about the anchor's centre of before the step, the pose to the result
#pragma unroll 1
  for (int k = anchor; k < a.tab.n_frames; ++k) {
    if (a.tab.body[k] != body) continue;
    double pose[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = d.pose_d[12 * k + i];
    if (step) {
      align_update_about(pose, E, cen, xi);
      al_keep_pose(d.pose_d + 12 * k, d.pose_f + 12 * k, pose);
    }
    al_put_pose(a.out->pose[k], pose);
    if (k == anchor) al_put_pose(out->pose, pose);
  }
}

// the state block as it lies in tf_volume::align_group (base == null: its size)
GAlignDev galign_carve(void* base, size_t cap_tiles, size_t* bytes) {
  GAlignDev d{};
  d.rows_cap = (uint32_t)((cap_tiles + kAlWaves - 1) / kAlWaves);
  Carver c(base);
  c.take(d.ctl, kGaMax);
  c.take(d.pose_d, 12 * kGaMax);
  c.take(d.pose_f, 12 * kGaMax);
  c.take(d.res, 1);
  c.take(d.log, (size_t)kGaMax * TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kGaMax * d.rows_cap * kAlRow);
  if (bytes) *bytes = c.L.size;
  return d;
}
// the block sized for seven frames of the camera at stride 1
int galign_ensure(tf_volume* v, GAlignDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; galign_carve(nullptr, tiles, &n); return n; };
  const int rc = align_ensure(v, v->align_group, bytes_of, kGaMax * sizeof(AlignCtl));
  if (rc) return rc;
  *d = galign_carve(v->align_group.block.p, v->align_group.cap_tiles, nullptr);
  return TF_OK;
}

// everything a call is refused for, and the partition as the kernels read it
int galign_check(tf_volume* v, int32_t n_frames, const float* const* depth, const float* poses12, const int32_t* body,
                 const tf_align_params* p, const void* result, GAlignTable* tab) {
  if (!v || !depth || !poses12 || !p || !result) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n_frames < 1 || n_frames > kGaMax) { set_error("align group: n_frames must be 1..7"); return TF_ERR_INVALID; }
  GAlignTable t{};
  t.n_frames = n_frames;
  for (int k = 0; k < n_frames; ++k) {
    const int rc = align_check(v, depth[k], poses12 + 12 * k, p, true);
    if (rc) return rc;
    const int32_t b = body ? body[k] : 0;
    if (b < 0 || b > t.n_bodies) {
      set_error("align group: bodies are numbered by first appearance (body[0] == 0, body[k] <= 1 + max(body[0..k-1]))");
      return TF_ERR_INVALID;
    }
    if (b == t.n_bodies) { t.first[b] = (uint8_t)k; t.n_bodies += 1; }
    t.body[k] = (uint8_t)b;
    t.anchor[k] = t.first[b];
  }
  *tab = t;
  return TF_OK;
}

// every launch of one call: begin, then (rows, solve) per step and once more to close
int galign_enqueue(tf_volume* v, const GAlignDev& d, const GAlignTable& tab, const float* const* d_depth, const float* poses12,
                   const tf_align_params& p, tf_align_group_result* d_result) {
  hipStream_t st = v->stream;
  GAlignPoses P{};
  memcpy(P.p, poses12, sizeof(float) * 12 * (size_t)tab.n_frames);
  hipLaunchKernelGGL(k_galign_begin, dim3(1), dim3(256), 0, st, d, P, tab, d_result);
  GAlignRowsArgs ra{};
  for (int k = 0; k < tab.n_frames; ++k) ra.depth[k] = d_depth[k];
  ra.tab = tab; ra.pose = d.pose_f; ra.ctl = d.ctl; ra.res = v->res; ra.part = d.part; ra.rows_cap = d.rows_cap;
  align_walk(v, p, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    ra.c = c;
    hipLaunchKernelGGL(k_galign_rows, dim3(sc.n_rows, (uint32_t)tab.n_frames), dim3(kAlWaves * 64), 0, st, v->dev, ra);
    hipLaunchKernelGGL(k_galign_solve, dim3((uint32_t)tab.n_bodies), dim3(256), 0, st, d, GAlignSolveArgs{sc, tab, d_result});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

void align_group_release(tf_volume* v) { v->align_group = AlignBlock{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_group_device(tf_volume* v, int32_t n_frames, const float* const* d_depth, const float* poses12,
                          const int32_t* body, const tf_align_params* params, tf_align_group_result* d_result) {
  GAlignTable tab;
  int rc = galign_check(v, n_frames, d_depth, poses12, body, params, d_result, &tab);
  if (rc) return rc;
  TF_DEV_READER(v);
  GAlignDev d;
  if ((rc = galign_ensure(v, &d))) return rc;
  return galign_enqueue(v, d, tab, d_depth, poses12, *params, d_result);
}

int tf_align_group(tf_volume* v, int32_t n_frames, const float* const* depth, const float* poses12, const int32_t* body,
                   const tf_align_params* params, tf_align_group_result* result) {
  GAlignTable tab;
  int rc = galign_check(v, n_frames, depth, poses12, body, params, result, &tab);
  if (rc) return rc;
  TF_DEV_READER(v);
  const size_t P = align_pixels(v);
  Layout L;
  size_t o_d[kGaMax] = {};
  for (int k = 0; k < n_frames; ++k) o_d[k] = L.take(4 * P);
  const size_t o_r = L.take(sizeof(tf_align_group_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg))) return rc;
  const float* d_depth[kGaMax] = {};
  for (int k = 0; k < n_frames; ++k) {
    if ((rc = stage_in(v, sg, o_d[k], depth[k], 4 * P))) return rc;
    d_depth[k] = sg.dp<const float>(o_d[k]);
  }
  GAlignDev d;
  if ((rc = galign_ensure(v, &d))) return rc;
  if ((rc = galign_enqueue(v, d, tab, d_depth, poses12, *params, sg.dp<tf_align_group_result>(o_r)))) return rc;
  return stage_out(v, sg, o_r, sizeof(tf_align_group_result), result);
}

int tf_align_group_log(tf_volume* v, int32_t body, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  if (body < 0 || body >= kGaMax) { set_error("align group: body must be 0..6"); return TF_ERR_INVALID; }
  const AlignBlock& s = v->align_group;
  if (!s.block) return align_log(v, nullptr, nullptr, 0, out, cap, n);
  const GAlignDev d = galign_carve(s.block.p, s.cap_tiles, nullptr);
  // (a body the last call did not have was cleared by its begin: no records)
  return align_log(v, d.ctl + body, d.log + (size_t)body * TF_ALIGN_MAX_EVALUATIONS, sizeof(tf_align_iter), out, cap, n);
}

int tf_align_unit_group(tf_volume* v, tf_unit_group* group, int rigid, const tf_align_params* params,
                        tf_align_group_result* result) {
  if (!v || !group || !result) { set_error("null argument"); return TF_ERR_INVALID; }
  if (group->n_local < 0 || group->n_local > kGaMax - 1) { set_error("align group: n_local must be 0..6"); return TF_ERR_INVALID; }
  const int32_t n_frames = 1 + group->n_local;
  const float* d_depth[kGaMax] = {};
  float poses[kGaMax * 12];
  int32_t body[kGaMax];
  for (int k = 0; k < n_frames; ++k) {
    const tf_unit_frame& f = k == 0 ? group->keyframe : group->local[k - 1];
    d_depth[k] = f.d_depth;
    memcpy(poses + 12 * k, f.pose, sizeof(f.pose));
    body[k] = rigid ? 0 : k;
  }
  GAlignTable tab;
  int rc = galign_check(v, n_frames, d_depth, poses, body, params, result, &tab);
  if (rc) return rc;
  TF_DEV_READER(v);
  GAlignDev d;
  if ((rc = galign_ensure(v, &d))) return rc;
  if ((rc = galign_enqueue(v, d, tab, d_depth, poses, *params, d.res))) return rc;
  tf_align_group_result got;
  TF_HIP(hipMemcpyAsync(&got, d.res, sizeof(got), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  *result = got;
  for (int k = 0; k < n_frames; ++k) {
    if (got.body[tab.body[k]].status > TF_ALIGN_MAX_ITERS) continue;
    tf_unit_frame& f = k == 0 ? group->keyframe : group->local[k - 1];
    memcpy(f.pose, got.pose[k], sizeof(f.pose));
  }
  return TF_OK;
}

}  // extern "C"
