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
// Per sampled pixel of frame k everything up to g, q and the flags is k_align_rows' text, operation for operation (the
// per-pixel body is copied from tf_align.hip, whose header comment is the specification; -ffp-contract=off).  The one
// difference is the lever of the rotational part: the twist of a body is taken about its anchor's camera centre (the
// anchor is the body's first frame).
//   anchor:        J = [g, q x g]                                             -- tf_align_frame's row
//   another frame: a = (t_k - t_anchor) + q componentwise in f32, from the two f32 poses the rows are sampled at,
//                  J = (g.x, g.y, g.z, a.y g.z - a.z g.y, a.z g.x - a.x g.z, a.x g.y - a.y g.x)
//   w, wJ, wr as tf_align.hip's.
// Sums: a frame's 31 sums are formed exactly as k_align_rows + k_align_solve form them (the wave tree of tf_align_tree.h,
// the eight tiles of a workgroup in wave order, the rows g, g + 8, .. ascending, then the eight groups in order); a body's
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

#include <type_traits>

#include "tf_align_group_solve.h"
#include "tf_align_tree.h"
#include "tf_ray_devfn.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

constexpr int kGaMax = TF_ALIGN_GROUP_MAX_FRAMES;
constexpr int kGaResultWords = (int)(sizeof(tf_align_group_result) / 4);
static_assert(sizeof(tf_align_group_result) % 4 == 0 && kGaResultWords <= 256 && 12 * kGaMax <= 256, "k_galign_begin");

struct GAlignCtl {  // one per body
  uint32_t state;   // bit 0: stopped (too few / singular), bits 8..: levels finished
  int32_t status;
  int32_t n_eval;
  int32_t n_valid_first;
  float rms_first;
  uint32_t pad[3];
};
struct GAlignDev {
  GAlignCtl* ctl;               // [kGaMax]
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
  const float* depth[kGaMax];
  GAlignTable tab;
  const float* pose;      // pose_f of the state block
  const GAlignCtl* ctl;
  float fx, fy, cxs, cys;
  int W, H, tiles_x, stride, level;
  float min_depth, max_depth, max_residual, huber, res;
  double* part;
  uint32_t rows_cap;
};
struct GAlignSolveArgs {
  GAlignTable tab;
  int level, log_level, stride, closing, last_level;
  uint32_t n_rows;  // workgroups of a frame in the rows launch
  float damping, eps_t, eps_r;
  int min_valid;
  tf_align_group_result* out;
};

__device__ __forceinline__ bool gal_idle(const uint32_t* state, int level) {
  const uint32_t st = *state;
  return (st & 1u) || (uint32_t)level < (st >> 8);
}

__global__ __launch_bounds__(256) void k_galign_begin(GAlignDev d, GAlignPoses p, GAlignTable tab, tf_align_group_result* out) {
  const int i = threadIdx.x;
  if (i < 12 * tab.n_frames) { const float x = p.p[i]; d.pose_d[i] = (double)x; d.pose_f[i] = x; }
  if (i < kGaMax) {
    GAlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    d.ctl[i] = c;
  }
  // n_frames and n_bodies are the result's first two words
  if (i < kGaResultWords) reinterpret_cast<int32_t*>(out)[i] = i == 0 ? tab.n_frames : (i == 1 ? tab.n_bodies : 0);
}

// (resources: tests/test_kernel_resources_align_group.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_galign_rows(VolumeDev v, GAlignRowsArgs a) {
  const int fk = blockIdx.y, fa = a.tab.anchor[fk];
  if (gal_idle(&a.ctl[a.tab.body[fk]].state, a.level)) return;
  // (a tile beyond the last one of the level lies below the image: none of its lanes is inside)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kAlWaves + wave;
  const long long X = (long long)((tile % a.tiles_x) * 8 + (lane & 7)) * a.stride;
  const long long Y = (long long)((tile / a.tiles_x) * 8 + (lane >> 3)) * a.stride;
  const bool in = X < a.W && Y < a.H;
  const float* P = a.pose + 12 * fk;
  uint32_t fl = 0;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  if (in) {
    const float z = a.depth[fk][(size_t)Y * a.W + (size_t)X];
    if (isfinite(z) && z >= a.min_depth && z <= a.max_depth) {
      fl = 1u;
      const float res = a.res, ir = 1.0f / res;
      const float dcx = ((float)(int)X - a.cxs) / a.fx, dcy = ((float)(int)Y - a.cys) / a.fy;
      const float pcx = dcx * z, pcy = dcy * z;
      qx = (P[0] * pcx + P[1] * pcy) + P[2] * z;
      qy = (P[4] * pcx + P[5] * pcy) + P[6] * z;
      qz = (P[8] * pcx + P[9] * pcy) + P[10] * z;
      const float wx = P[3] + qx, wy = P[7] + qy, wz = P[11] + qz;
      ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
      float sc = 0.f;
      if (tri_sample<false>(v, cc, wx, wy, wz, ir, &sc)) {
        fl |= 2u;
        s = sc;
        // tap k: axis k >> 1, minus / plus by k & 1, as k_align_rows
        float sp0 = 0.f, sp1 = 0.f, sp2 = 0.f, sm0 = 0.f, sm1 = 0.f, sm2 = 0.f;
        bool ok = true;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
          const int ax = k >> 1;
          float t = 0.f;
          const float h = (k & 1) ? res : -res;  // (a + (-b) is a - b)
          ChunkCache ct = cc;  // every tap starts from the centre's chunk
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
  }
  const bool valid = fl == 15u;
  // the lever: q for the anchor, (t_k - t_anchor) + q for a later frame of the body (uniform over the workgroup)
  float lx = qx, ly = qy, lz = qz;
  if (fa != fk) {
    const float* PA = a.pose + 12 * fa;
    lx = (P[3] - PA[3]) + qx; ly = (P[7] - PA[7]) + qy; lz = (P[11] - PA[11]) + qz;
  }
  float J[6] = {gx, gy, gz, ly * gz - lz * gy, lz * gx - lx * gz, lx * gy - ly * gx};
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
    a.part[((size_t)fk * a.rows_cap + blockIdx.x) * kAlRow + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void k_galign_solve(GAlignDev d, GAlignSolveArgs a) {
  const int body = blockIdx.x;
  GAlignCtl* ctl = d.ctl + body;
  if (gal_idle(&ctl->state, a.level)) return;
  const bool first_eval = ctl->n_eval == 0;  // (read by every thread ahead of the barriers; lane 0 writes behind them)
  // per frame of the body, in ascending order: thread (e = tid & 31, g = tid >> 5) adds entry e of the frame's rows g, g + 8,
  // g + 16, .. in ascending order, thread e then the eight groups in order -- k_align_solve's additions -- and adds the
  // frame's sum to the body's.  (One frame after the other: seven accumulators side by side in one loop over the rows
  // were measured slower, 66 against 47 us for an evaluation of one frame at stride 1.)
  __shared__ double red[8][kAlRow];
  __shared__ double tot[kAlRow];
  const uint32_t tid = threadIdx.x, e = tid & 31u, g = tid >> 5;
  double sum = 0.0;
  bool have = false;
#pragma unroll 1
  for (int k = 0; k < a.tab.n_frames; ++k) {
    if (a.tab.body[k] != body) continue;
    const double* part = d.part + (size_t)k * d.rows_cap * kAlRow;
    double acc = 0.0;
    if (e < (uint32_t)kAlSums)
#pragma unroll 8
      for (uint32_t t = g; t < a.n_rows; t += 8u) acc += part[(size_t)t * kAlRow + e];
    red[g][e] = acc;
    __syncthreads();
    if (tid < (uint32_t)kAlSums) {
      double t = red[0][tid];
#pragma unroll
      for (int j = 1; j < 8; ++j) t += red[j][tid];
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
  double S[kAlSums];
#pragma unroll
  for (int i = 0; i < kAlSums; ++i) S[i] = tot[i];
  GAlignCtl c = *ctl;
  const int n_valid = (int)S[kAlNv], n_sampled = (int)S[kAlNs];
  const float rms = n_valid > 0 ? (float)sqrt(S[kAlR2] / (double)n_valid) : 0.f;
  tf_align_iter* rec = d.log + (size_t)body * TF_ALIGN_MAX_EVALUATIONS +
                       (c.n_eval < TF_ALIGN_MAX_EVALUATIONS ? c.n_eval : TF_ALIGN_MAX_EVALUATIONS - 1);
  rec->level = a.log_level; rec->stride = a.stride; rec->n_sampled = n_sampled; rec->n_valid = n_valid;
  rec->sum_r2 = S[kAlR2]; rec->sum_wr2 = S[kAlWr2];
#pragma unroll
  for (int i = 0; i < 21; ++i) rec->A[i] = S[kAlA + i];
#pragma unroll
  for (int i = 0; i < 6; ++i) { rec->b[i] = S[kAlB + i]; rec->xi[i] = 0.0; }
  const int anchor = a.tab.first[body];
  double cen[3];
  {
    const double* pa = d.pose_d + 12 * anchor;
#pragma unroll
    for (int i = 0; i < 12; ++i) rec->pose[i] = pa[i];
    cen[0] = pa[3]; cen[1] = pa[7]; cen[2] = pa[11];
  }
  if (c.n_eval == 0) { c.n_valid_first = n_valid; c.rms_first = rms; }
  c.n_eval += 1;
  bool step = false;
  double xi[6], E[9];
  if (n_valid < a.min_valid) {
    c.status = TF_ALIGN_TOO_FEW;
    c.state |= 1u;
  } else if (!a.closing) {
    if (!align_solve6(S + kAlA, S + kAlB, (double)a.damping, xi)) {
      c.status = TF_ALIGN_SINGULAR;
      c.state |= 1u;
    } else {
      step = true;
      align_rodrigues(xi + 3, E);
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
  *ctl = c;
  tf_align_result* out = a.out->body + body;
  out->status = c.status; out->evaluations = c.n_eval; out->n_sampled = n_sampled;
  out->n_valid_first = c.n_valid_first; out->n_valid_last = n_valid;
  out->rms_first = c.rms_first; out->rms_last = rms;
  // every frame of the body: the step about the anchor's centre of before the step, the pose to the result
#pragma unroll 1
  for (int k = anchor; k < a.tab.n_frames; ++k) {
    if (a.tab.body[k] != body) continue;
    double pose[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = d.pose_d[12 * k + i];
    if (step) {
      align_update_about(pose, E, cen, xi);
#pragma unroll
      for (int i = 0; i < 12; ++i) { d.pose_d[12 * k + i] = pose[i]; d.pose_f[12 * k + i] = (float)pose[i]; }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) a.out->pose[k][i] = (float)pose[i];
    if (k == anchor)
#pragma unroll
      for (int i = 0; i < 12; ++i) out->pose[i] = (float)pose[i];
  }
}

// the state block as it lies in AlignGroupState::block (base == null: its size)
GAlignDev galign_carve(void* base, size_t cap_tiles, size_t* bytes) {
  GAlignDev d{};
  d.rows_cap = (uint32_t)((cap_tiles + kAlWaves - 1) / kAlWaves);
  Layout L;
  uint8_t* b = static_cast<uint8_t*>(base);
  const auto take = [&](auto*& p, size_t count) {
    const size_t at = L.take(count * sizeof(*p));
    p = b ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + at) : nullptr;
  };
  take(d.ctl, kGaMax);
  take(d.pose_d, 12 * kGaMax);
  take(d.pose_f, 12 * kGaMax);
  take(d.res, 1);
  take(d.log, (size_t)kGaMax * TF_ALIGN_MAX_EVALUATIONS);
  take(d.part, (size_t)kGaMax * d.rows_cap * kAlRow);
  if (bytes) *bytes = L.size;
  return d;
}

size_t galign_pixels(const tf_volume* v) { const AlignCam c = align_cam(v); return (size_t)c.W * (size_t)c.H; }

// first use, or a larger camera since: the block sized for seven frames of the camera at stride 1
int galign_ensure(tf_volume* v, GAlignDev* d) {
  const AlignCam c = align_cam(v);
  const size_t tiles = (size_t)((c.W + 7) / 8) * (size_t)((c.H + 7) / 8);
  AlignGroupState& s = v->align_group;
  if (!s.block || s.cap_tiles < tiles) {
    size_t bytes = 0;
    galign_carve(nullptr, tiles, &bytes);
    if (s.block) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = s.block.alloc(bytes);
    if (rc) { s.cap_tiles = 0; return rc; }
    TF_HIP(hipMemsetAsync(s.block.p, 0, kGaMax * sizeof(GAlignCtl), v->stream));
    s.cap_tiles = tiles;
  }
  *d = galign_carve(s.block.p, s.cap_tiles, nullptr);
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
  const AlignCam c = align_cam(v);
  for (int l = 0; l <= p.n_levels; ++l) {
    const bool closing = l == p.n_levels;
    GAlignRowsArgs ra{};
    for (int k = 0; k < tab.n_frames; ++k) ra.depth[k] = d_depth[k];
    ra.tab = tab; ra.pose = d.pose_f; ra.ctl = d.ctl; ra.part = d.part; ra.rows_cap = d.rows_cap;
    const int s = p.stride[closing ? p.n_levels - 1 : l];
    ra.fx = c.fx; ra.fy = c.fy; ra.cxs = c.cx + 0.5f; ra.cys = c.cy + 0.5f;
    ra.W = c.W; ra.H = c.H; ra.stride = s; ra.level = l;
    const int nx = (int)(((long long)ra.W + s - 1) / s), ny = (int)(((long long)ra.H + s - 1) / s);
    ra.tiles_x = (nx + 7) / 8;
    const uint32_t n_tiles = (uint32_t)ra.tiles_x * (uint32_t)((ny + 7) / 8);  // <= the tiles at stride 1
    ra.min_depth = p.min_depth; ra.max_depth = p.max_depth; ra.max_residual = p.max_residual; ra.huber = p.huber;
    ra.res = v->res;
    GAlignSolveArgs sa{};
    sa.tab = tab;
    sa.level = l; sa.log_level = closing ? p.n_levels - 1 : l; sa.stride = s; sa.closing = closing;
    sa.last_level = l == p.n_levels - 1; sa.n_rows = (n_tiles + kAlWaves - 1) / kAlWaves;
    sa.damping = p.damping; sa.eps_t = p.eps_t; sa.eps_r = p.eps_r; sa.min_valid = p.min_valid; sa.out = d_result;
    const int n = closing ? 1 : p.iters[l];
    for (int it = 0; it < n; ++it) {
      hipLaunchKernelGGL(k_galign_rows, dim3(sa.n_rows, (uint32_t)tab.n_frames), dim3(kAlWaves * 64), 0, st, v->dev, ra);
      hipLaunchKernelGGL(k_galign_solve, dim3((uint32_t)tab.n_bodies), dim3(256), 0, st, d, sa);
    }
  }
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

void align_group_release(tf_volume* v) { v->align_group = AlignGroupState{}; }

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
  const size_t P = galign_pixels(v);
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
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, sizeof(tf_align_group_result), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(result, sg.h + o_r, sizeof(tf_align_group_result));
  return TF_OK;
}

int tf_align_group_log(tf_volume* v, int32_t body, tf_align_iter* out, int64_t cap, int64_t* n) {
  if (!v || !n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  if (body < 0 || body >= kGaMax) { set_error("align group: body must be 0..6"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  if (!v->align_group.block) return TF_OK;
  const GAlignDev d = galign_carve(v->align_group.block.p, v->align_group.cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  GAlignCtl c;  // (a body the last call did not have was cleared by its begin: no records)
  TF_HIP(hipMemcpy(&c, d.ctl + body, sizeof(c), hipMemcpyDeviceToHost));
  const int64_t have = c.n_eval < 0 ? 0 : (c.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : c.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0)
    TF_HIP(hipMemcpy(out, d.log + (size_t)body * TF_ALIGN_MAX_EVALUATIONS, (size_t)m * sizeof(tf_align_iter),
                     hipMemcpyDeviceToHost));
  return TF_OK;
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
