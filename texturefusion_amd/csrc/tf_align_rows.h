// tf_align_rows.h -- the Gauss-Newton machinery the four aligners share (tf_align.hip, tf_align_color.hip,
// tf_align_group.hip, tf_align_icp.hip) and the colour ICP (tf_align_icp_color.hip), beside the tile's tree (tf_align_tree.h) and the 6 x 6 step (tf_align_solve.h).
// Device only; every function is forced inline into the kernel that calls it and every operation is rounded on its own.
// An aligner keeps what is its own: the row of a pixel, the lever of the twist, how a step is applied.  This file is the
// one place for the rest, and with tf_align_tree.h it fixes the order of every addition:
//
//   rows launch   one wave per 8 x 8 tile of SAMPLED pixels (lane = 8 y + x, a tile spans 8 * stride image pixels), eight
//                 waves per workgroup (al_pixel).  A pixel's row J = [g, l x g] with gradient g and lever l, its Huber
//                 weight, an exact zero in every term where the pixel is not valid (al_row_sums); the 64 lanes of a tile
//                 by the tree of al_tile_sum, the eight tiles of a workgroup in wave order, one plain-stored row of
//                 partial sums per workgroup (al_store_rows).
//   solve launch  eight threads per sum add the rows g, g + 8, g + 16, .. in ascending order, g = 0..7 (al_add_rows), then
//                 the eight in order (al_total).  Lane 0: the log record (al_fill_iter), the first evaluation's figures
//                 (al_count), the stop rules (al_decide), the result (al_fill_result).
//   stop rules    n_valid < min_valid: TF_ALIGN_TOO_FEW, the call stops.  Else, unless this is the closing evaluation, the
//                 damped solve: a failed pivot is TF_ALIGN_SINGULAR and the call stops; a step with |v| < eps_t and
//                 |w| < eps_r finishes the level, and on the last level the status is TF_ALIGN_CONVERGED.
//   exposure      with tf_align_set_exposure on, the photometric aligners add a third row of sums (al_exposure_row_sums) and
//                 their solve launch is al_solve_color_exposure: the pair eliminated ahead of the join, stepped after al_decide.
//   state word    bit 0: stopped, bits 8..: levels that are finished.  Every launch of a call is enqueued up front and
//                 reads this word first (al_idle); there are no atomics, no counters and no polling.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "tf_align_exposure_solve.h"
#include "tf_align_solve.h"
#include "tf_align_tree.h"
#include "../../include/tf_fusion.h"
#include "tf_ray_devfn.h"

#pragma clang fp contract(off)

namespace tf {

// the control words of one pose being aligned (tf_align_group.hip: one per body)
struct AlignCtl {
  uint32_t state;  // bit 0: stopped (too few / singular), bits 8..: levels finished
  int32_t status;
  int32_t n_eval;
  int32_t n_valid_first;
  float rms_first;
  int32_t n_photo_first;  // these two: tf_align_color.hip's
  float rms_photo_first;
  uint32_t pad;
};
static_assert(sizeof(AlignCtl) == 32, "AlignCtl");
struct AlignPose { float p[12]; };

// what every rows kernel and every solve kernel is told about its level: the first member of their argument structs, filled
// by align_level (tf_volume.h)
struct AlignRowsCommon {
  float fx, fy, cxs, cys;
  int W, H, tiles_x, stride, level;
  float min_depth, max_depth, max_residual, huber;
};
struct AlignSolveCommon {
  int level, log_level, stride, closing, last_level;
  uint32_t n_rows;  // workgroups (of a frame) in the rows launch
  float damping, eps_t, eps_r;
  int min_valid;
};

__device__ __forceinline__ bool al_idle(const uint32_t* state, int level) {
  const uint32_t st = *state;
  return (st & 1u) || (uint32_t)level < (st >> 8);
}

// the begin launch of an aligner with one pose: the caller's pose into the state block (f64 and f32) and the control words
// cleared, or for the residual maps the pose alone (the last alignment's state stays as it is)
__device__ __forceinline__ void al_begin(AlignCtl* ctl, double* pose_d, float* pose_f, float* pose_r, const AlignPose& p,
                                         int residuals_only) {
  const int i = threadIdx.x;
  if (residuals_only) {
    if (i < 12) pose_r[i] = p.p[i];
    return;
  }
  if (i < 12) { pose_d[i] = (double)p.p[i]; pose_f[i] = p.p[i]; }
  if (i == 0) {
    AlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    *ctl = c;
  }
}

// the thread's pixel.  (A tile beyond the last one of the level lies below the image: none of its lanes is inside.)
struct AlPixel {
  int lane, wave;
  long long X, Y;
  bool in;
};
__device__ __forceinline__ AlPixel al_pixel(const AlignRowsCommon& c) {
  AlPixel p;
  p.lane = threadIdx.x & 63; p.wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kAlWaves + p.wave;
  p.X = (long long)((tile % c.tiles_x) * 8 + (p.lane & 7)) * c.stride;
  p.Y = (long long)((tile / c.tiles_x) * 8 + (p.lane >> 3)) * c.stride;
  p.in = p.X < c.W && p.Y < c.H;
  return p;
}

// the pixel's point at pose P (12 f32, row-major [R | t]): q = R pc, pw = t + q.  False where z is out of range.
struct AlPoint { float qx, qy, qz, wx, wy, wz; };
__device__ __forceinline__ bool al_point(const AlignRowsCommon& c, const AlPixel& px, float z, const float* P, AlPoint* p) {
  if (!(isfinite(z) && z >= c.min_depth && z <= c.max_depth)) return false;
  const float dcx = ((float)(int)px.X - c.cxs) / c.fx, dcy = ((float)(int)px.Y - c.cys) / c.fy;
  const float pcx = dcx * z, pcy = dcy * z;
  p->qx = (P[0] * pcx + P[1] * pcy) + P[2] * z;
  p->qy = (P[4] * pcx + P[5] * pcy) + P[6] * z;
  p->qz = (P[8] * pcx + P[9] * pcy) + P[10] * z;
  p->wx = P[3] + p->qx; p->wy = P[7] + p->qy; p->wz = P[11] + p->qz;
  return true;
}

// The SDF row of a pixel inside the image (tf_align.hip's header states it): flag bits 0..3, s, g and q, zero where the
// bit that guards them is not set.  kLum: every sample also gives the model intensity (tri_sample_lum) -- lc at the
// centre, valid iff okl; the central differences cx, cy, cz (times 0.5f / res) of the six taps, valid iff okt.
struct AlSdfRow {
  uint32_t fl;
  float s, gx, gy, gz, qx, qy, qz;
};
struct AlLumRow {
  float lc, cx, cy, cz;
  bool okl, okt;
};
template <bool kLum>
__device__ __forceinline__ AlSdfRow al_sdf_row(const VolumeDev& v, const AlignRowsCommon& c, float res, const AlPixel& px,
                                               float z, const float* P, AlLumRow* lum = nullptr) {
  AlSdfRow r{};
  AlPoint p;
  if (!al_point(c, px, z, P, &p)) return r;
  r.fl = 1u;
  r.qx = p.qx; r.qy = p.qy; r.qz = p.qz;
  const float ir = 1.0f / res;
  const float wx = p.wx, wy = p.wy, wz = p.wz;
  ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
  float sc = 0.f, lc = 0.f;
  bool okl = false;
  const bool okc = kLum ? tri_sample_lum(v, cc, wx, wy, wz, ir, &sc, &lc, &okl) : tri_sample<false>(v, cc, wx, wy, wz, ir, &sc);
  if (!okc) return r;
  r.fl |= 2u;
  r.s = sc;
  // tap k: axis k >> 1, minus / plus by k & 1 (as the raycaster's normal; no one-sided fallback here)
  float sp0 = 0.f, sp1 = 0.f, sp2 = 0.f, sm0 = 0.f, sm1 = 0.f, sm2 = 0.f;
  float lp0 = 0.f, lp1 = 0.f, lp2 = 0.f, lm0 = 0.f, lm1 = 0.f, lm2 = 0.f;
  bool ok = true, okt = true;
#pragma unroll 1
  for (int k = 0; k < 6; ++k) {
    const int ax = k >> 1;
    float t = 0.f, l = 0.f;
    bool okk_l = false;
    const float h = (k & 1) ? res : -res;  // (a + (-b) is a - b)
    ChunkCache ct = cc;  // every tap starts from the centre's chunk: a tap that leaves it costs one probe, none to come back
    const float tx = ax == 0 ? wx + h : wx, ty = ax == 1 ? wy + h : wy, tz = ax == 2 ? wz + h : wz;
    const bool okk = kLum ? tri_sample_lum(v, ct, tx, ty, tz, ir, &t, &l, &okk_l) : tri_sample<false>(v, ct, tx, ty, tz, ir, &t);
    ok = ok && okk;
    okt = okt && okk_l;
    if (k == 0) { sm0 = t; lm0 = l; } else if (k == 1) { sp0 = t; lp0 = l; } else if (k == 2) { sm1 = t; lm1 = l; }
    else if (k == 3) { sp1 = t; lp1 = l; } else if (k == 4) { sm2 = t; lm2 = l; } else { sp2 = t; lp2 = l; }
  }
  if (!ok) return r;
  r.fl |= 4u;
  const float h2 = 0.5f / res;
  r.gx = (sp0 - sm0) * h2; r.gy = (sp1 - sm1) * h2; r.gz = (sp2 - sm2) * h2;
  if (fabsf(r.s) <= c.max_residual) r.fl |= 8u;
  if (kLum) {
    lum->lc = lc; lum->okl = okl; lum->okt = okt;
    lum->cx = (lp0 - lm0) * h2; lum->cy = (lp1 - lm1) * h2; lum->cz = (lp2 - lm2) * h2;
  }
  return r;
}

// The luma Lf of a frame pixel's RGBA8 word (r in the low byte), in [0, 1]: the photometric rows' (tf_align_color.hip's
// header), and what the exposure pair of tf_align_set_exposure compensates: Lfe = gain * Lf + offset.
__device__ __forceinline__ float al_luma(uint32_t c8) {
  const float r8 = (float)(c8 & 255u), g8 = (float)((c8 >> 8) & 255u), b8 = (float)((c8 >> 16) & 255u);
  return ((0.299f * r8 + 0.587f * g8) + 0.114f * b8) * (1.0f / 255.0f);
}
__device__ __forceinline__ float al_luma_exposed(float lf, const float* pair) { return pair[0] * lf + pair[1]; }

// The argument block of the rows launch of tf_align_frame_color (k_calign_rows, and k_ealign_rows of tf_align_exposure.hip)
struct CAlignRowsArgs {
  AlignRowsCommon c;
  const float* depth;
  const uint32_t* rgba;   // RGBA8, one word per pixel (r in the low byte)
  const float* pose;      // 12 floats in the state block
  const uint32_t* state;  // null: always run (tf_align_color_residuals)
  float res, max_photo_residual, huber_photo;
  size_t plane;
  float* r;
  float* grad;
  float* rc;
  float* gradc;
  uint32_t* flags;
  double* part;  // null: no sums
};

// A row's share of the sums: J = [g, l x g] with gradient g and lever l, the Huber weight of the residual r, an exact zero
// in every term where the pixel is not valid, the tile's sums through the wave tree (lane l ends up with entry
// al_entry(l)) into the wave's line of `wsum`, `at` doubles in.  al_store_rows follows, once for all rows of the pixel.
template <int kRow>
__device__ __forceinline__ void al_row_sums(double (&wsum)[kAlWaves][kRow], int at, const AlPixel& px, float gx, float gy,
                                            float gz, float lx, float ly, float lz, float r, float huber, bool valid,
                                            bool in) {
  float J[6] = {gx, gy, gz, ly * gz - lz * gy, lz * gx - lx * gz, lx * gy - ly * gx};
  const float ar = fabsf(r);
  float w = (huber == 0.f || ar <= huber) ? 1.0f : huber / ar;
  if (!valid) {
    w = 0.f; r = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = 0.f;
  }
  const double total = al_tile_sum(J, w, r, valid ? 1.0f : 0.0f, in ? 1.0f : 0.0f, px.lane);
  if (!(px.lane & 1)) wsum[px.wave][at + al_entry(px.lane)] = total;
}
// The exposure row's share (tf_align_set_exposure): the photometric row's own operands wJc_i = wc * Jc_i, wc, rc and the
// frame's uncompensated luma lf, an exact zero in every term where the pixel is not photometrically valid, through the
// same tree with the second pair table (tf_align_tree.h states the 17 sums and their order) into `at` of the wave's line.
template <int kRow>
__device__ __forceinline__ void al_exposure_row_sums(double (&wsum)[kAlWaves][kRow], int at, const AlPixel& px, float gx,
                                                     float gy, float gz, float lx, float ly, float lz, float rc, float lf,
                                                     float huber, bool valid) {
  // (J, w and the zeroing are al_row_sums' own lines: the compiler forms them once for both rows)
  float J[6] = {gx, gy, gz, ly * gz - lz * gy, lz * gx - lx * gz, lx * gy - ly * gx};
  const float ar = fabsf(rc);
  float w = (huber == 0.f || ar <= huber) ? 1.0f : huber / ar;
  if (!valid) {
    w = 0.f; rc = 0.f; lf = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) J[i] = 0.f;
  }
  float wJ[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) wJ[i] = w * J[i];
  const double total = al_exposure_tile_sum(wJ, w, lf, rc, valid ? 1.0f : 0.0f, px.lane);
  if (!(px.lane & 1)) wsum[px.wave][at + al_entry(px.lane)] = total;
}
// the workgroup's eight tiles in wave order, one plain-stored row of kRow doubles per workgroup
template <int kRow>
__device__ __forceinline__ void al_store_rows(const double (&wsum)[kAlWaves][kRow], double* row) {
  __syncthreads();
  if (threadIdx.x < (unsigned)kRow) {  // (a row's 32nd entry is padding, never read)
    double t = wsum[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kAlWaves; ++k) t += wsum[k][threadIdx.x];
    row[threadIdx.x] = t;
  }
}

// The solve launch's additions over n_rows partial rows of kRow doubles (kRow / 32 rows of sums side by side): thread
// (e = tid & 31, g = tid >> 5) adds entry e of the rows g, g + 8, g + 16, .. in ascending order into red[g] (a row's
// entries lie side by side: the 32 threads of a group read one 256-byte row).  Ends at a barrier.
template <int kRow>
__device__ __forceinline__ void al_add_rows(const double* part, uint32_t n_rows, double (&red)[8][kRow]) {
  constexpr int kSets = kRow / kAlRow, kUnroll = 8 / kSets;
  const uint32_t tid = threadIdx.x, e = tid & 31u, g = tid >> 5;
  double acc[kSets];
#pragma unroll
  for (int j = 0; j < kSets; ++j) acc[j] = 0.0;
  if (e < (uint32_t)kAlSums)
#pragma unroll kUnroll
    for (uint32_t t = g; t < n_rows; t += 8u)
#pragma unroll
      for (int j = 0; j < kSets; ++j) acc[j] += part[(size_t)t * kRow + j * kAlRow + e];
#pragma unroll
  for (int j = 0; j < kSets; ++j) red[g][j * kAlRow + e] = acc[j];
  __syncthreads();
}
// entry i: the eight groups in order
template <int kRow>
__device__ __forceinline__ double al_total(const double (&red)[8][kRow], int i) {
  double t = red[0][i];
#pragma unroll
  for (int k = 1; k < 8; ++k) t += red[k][i];
  return t;
}

// ---- lane 0 of a solve launch.  `sum(i)` gives entry i of the 31 sums (kAlA.. of tf_align_tree.h). ----
struct AlEval {
  int n_valid, n_sampled;
  float rms;
};
// the record of this evaluation in a log of TF_ALIGN_MAX_EVALUATIONS records (further evaluations overwrite the last)
template <class Rec>
__device__ __forceinline__ Rec* al_record(Rec* log, const AlignCtl& c) {
  return log + (c.n_eval < TF_ALIGN_MAX_EVALUATIONS ? c.n_eval : TF_ALIGN_MAX_EVALUATIONS - 1);
}
// the log record of an evaluation at `pose` (xi = 0 until al_decide takes a step), and the system A, b for the solve
template <class Sum>
__device__ __forceinline__ AlEval al_fill_iter(tf_align_iter* rec, const AlignSolveCommon& a, const Sum& sum,
                                               const double* pose, double (&A)[21], double (&b)[6]) {
  const double sum_r2 = sum(kAlR2);
  AlEval ev;
  ev.n_valid = (int)sum(kAlNv); ev.n_sampled = (int)sum(kAlNs);
  ev.rms = ev.n_valid > 0 ? (float)sqrt(sum_r2 / (double)ev.n_valid) : 0.f;
  rec->level = a.log_level; rec->stride = a.stride; rec->n_sampled = ev.n_sampled; rec->n_valid = ev.n_valid;
  rec->sum_r2 = sum_r2; rec->sum_wr2 = sum(kAlWr2);
#pragma unroll
  for (int i = 0; i < 21; ++i) { A[i] = sum(kAlA + i); rec->A[i] = A[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { b[i] = sum(kAlB + i); rec->b[i] = b[i]; rec->xi[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 12; ++i) rec->pose[i] = pose[i];
  return ev;
}
// the first evaluation's figures are kept for the result; every evaluation is counted
__device__ __forceinline__ void al_count(AlignCtl& c, const AlEval& ev) {
  if (c.n_eval == 0) { c.n_valid_first = ev.n_valid; c.rms_first = ev.rms; }
  c.n_eval += 1;
}
// the stop rules (this file's header).  True where the step xi is to be applied; it is in the record then.
__device__ __forceinline__ bool al_decide(AlignCtl& c, const AlignSolveCommon& a, int n_valid, const double (&A)[21],
                                          const double (&b)[6], tf_align_iter* rec, double (&xi)[6]) {
  if (n_valid < a.min_valid) {
    c.status = TF_ALIGN_TOO_FEW;
    c.state |= 1u;
    return false;
  }
  if (a.closing) return false;
  if (!align_solve6(A, b, (double)a.damping, xi)) {
    c.status = TF_ALIGN_SINGULAR;
    c.state |= 1u;
    return false;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) rec->xi[i] = xi[i];
  const double nt = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
  const double nr = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
  if (nt < (double)a.eps_t && nr < (double)a.eps_r) {
    c.state = (c.state & 0xFFu) | ((uint32_t)(a.level + 1) << 8);
    if (a.last_level) c.status = TF_ALIGN_CONVERGED;
  }
  return true;
}
// a pose between iterations: f64, and rounded to f32 for the rows
__device__ __forceinline__ void al_keep_pose(double* pose_d, float* pose_f, const double (&pose)[12]) {
#pragma unroll
  for (int i = 0; i < 12; ++i) { pose_d[i] = pose[i]; pose_f[i] = (float)pose[i]; }
}
__device__ __forceinline__ void al_put_pose(float* out, const double (&pose)[12]) {
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = (float)pose[i];
}
// the result but for its pose
__device__ __forceinline__ void al_fill_result(tf_align_result* out, const AlignCtl& c, const AlEval& ev) {
  out->status = c.status; out->evaluations = c.n_eval; out->n_sampled = ev.n_sampled;
  out->n_valid_first = c.n_valid_first; out->n_valid_last = ev.n_valid;
  out->rms_first = c.rms_first; out->rms_last = ev.rms;
}

// A whole solve launch of an aligner with one pose, one row of sums and the twist about the camera centre (k_align_solve,
// k_icp_solve): one workgroup of 256 threads.
__device__ __forceinline__ void al_solve_pose(AlignCtl* ctl, tf_align_iter* log, double* pose_d, float* pose_f,
                                              const double* part, const AlignSolveCommon& a, tf_align_result* out) {
  if (al_idle(&ctl->state, a.level)) return;
  __shared__ double red[8][kAlRow];
  al_add_rows(part, a.n_rows, red);
  if (threadIdx.x != 0) return;
  AlignCtl c = *ctl;
  tf_align_iter* rec = al_record(log, c);
  double pose[12], A[21], b[6], xi[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = pose_d[i];
  const AlEval ev = al_fill_iter(rec, a, [&](int i) { return al_total(red, i); }, pose, A, b);
  al_count(c, ev);
  if (al_decide(c, a, ev.n_valid, A, b, rec, xi)) {
    align_update(pose, xi);
    al_keep_pose(pose_d, pose_f, pose);
  }
  *ctl = c;
  al_fill_result(out, c, ev);
  al_put_pose(out->pose, pose);
}

// A whole solve launch of an aligner with one pose and two rows of sums, a geometric and a photometric one, joined as
// M = A_g + l2 A_c, b = b_g + l2 b_c (k_calign_solve, k_cicp_solve): one workgroup of 256 threads.
constexpr int kCaRow = 2 * kAlRow;   // doubles of a workgroup's partial sums: the geometric row, then the photometric one
// the photometric row's counts of an evaluation into its record (the first evaluation's are kept for the result), and the
// result of a call with a photometric row
struct AlPhotoEval {
  int n_photo;
  float rms;
};
template <int kRow>
__device__ __forceinline__ AlPhotoEval al_fill_photo(tf_align_color_iter* rec, const double (&red)[8][kRow], AlignCtl& c) {
  const double sum_rc2 = al_total(red, kAlRow + kAlR2);
  AlPhotoEval ph;
  ph.n_photo = (int)al_total(red, kAlRow + kAlNv);
  ph.rms = ph.n_photo > 0 ? (float)sqrt(sum_rc2 / (double)ph.n_photo) : 0.f;
  rec->n_photo = ph.n_photo; rec->pad = 0;
  rec->sum_rc2 = sum_rc2; rec->sum_wrc2 = al_total(red, kAlRow + kAlWr2);
  if (c.n_eval == 0) { c.n_photo_first = ph.n_photo; c.rms_photo_first = ph.rms; }
  return ph;
}
__device__ __forceinline__ void al_fill_color_result(tf_align_color_result* out, const AlignCtl& c, const AlEval& ev,
                                                     const AlPhotoEval& ph, const double (&pose)[12]) {
  al_fill_result(&out->geo, c, ev);
  al_put_pose(out->geo.pose, pose);
  out->n_photo_first = c.n_photo_first; out->n_photo_last = ph.n_photo;
  out->rms_photo_first = c.rms_photo_first; out->rms_photo_last = ph.rms;
}
__device__ __forceinline__ void al_solve_color(AlignCtl* ctl, tf_align_color_iter* log, double* pose_d, float* pose_f,
                                               const double* part, const AlignSolveCommon& a, double l2,
                                               tf_align_color_result* out) {
  if (al_idle(&ctl->state, a.level)) return;
  // both rows of every workgroup through k_align_solve's additions; the photometric sums go to the record, the joined
  // system stays in registers
  __shared__ double red[8][kCaRow];
  al_add_rows(part, a.n_rows, red);
  if (threadIdx.x != 0) return;
  AlignCtl c = *ctl;
  tf_align_color_iter* rec = al_record(log, c);
  double pose[12], M[21], bb[6], xi[6];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = pose_d[i];
  const AlEval ev = al_fill_iter(&rec->geo, a, [&](int i) { return al_total(red, i); }, pose, M, bb);
#pragma unroll
  for (int i = 0; i < 21; ++i) {
    const double tc = al_total(red, kAlRow + kAlA + i);
    rec->Ac[i] = tc;
    M[i] = M[i] + l2 * tc;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double tc = al_total(red, kAlRow + kAlB + i);
    rec->bc[i] = tc;
    bb[i] = bb[i] + l2 * tc;
  }
  const AlPhotoEval ph = al_fill_photo(rec, red, c);
  al_count(c, ev);
  if (al_decide(c, a, ev.n_valid, M, bb, &rec->geo, xi)) {
    align_update(pose, xi);
    al_keep_pose(pose_d, pose_f, pose);
  }
  *ctl = c;
  al_fill_color_result(out, c, ev, ph, pose);
}

// The same launch with the exposure pair (tf_align_set_exposure): three rows of sums per workgroup, the pair eliminated
// from the photometric system ahead of the join and stepped after al_decide (tf_align_exposure_solve.h states every
// operation).  k_ealign_solve of tf_align_exposure.hip, for both photometric aligners.
constexpr int kCeRow = 3 * kAlRow;  // the geometric row, the photometric one, the exposure row (tf_align_tree.h: kAlExp*)
struct AlExposureCtl {   // the pair of a call, in the exposure state block
  double pair_d[2];      // (gain, offset) between iterations
  float pair_f[2];       // the same rounded: what the rows kernels compensate with
  float pair_r[2];       // the residual maps' pair (the last alignment's state stays as it is)
  int32_t valid, n_eval; // the last call ended with status <= TF_ALIGN_MAX_ITERS; its evaluations
};
struct AlExposureArgs {
  AlExposureCtl* x;
  tf_align_exposure_iter* log;
  double* cell;          // the handle's start pair
  int unknowns, carry;
  double min_gain, max_gain;
};
__device__ __forceinline__ void al_solve_color_exposure(AlignCtl* ctl, tf_align_color_iter* log, double* pose_d, float* pose_f,
                                                        const double* part, const AlignSolveCommon& a, double l2,
                                                        tf_align_color_result* out, const AlExposureArgs& e) {
  if (al_idle(&ctl->state, a.level)) return;
  __shared__ double red[8][kCeRow];
  al_add_rows(part, a.n_rows, red);
  if (threadIdx.x != 0) return;
  AlignCtl c = *ctl;
  tf_align_color_iter* rec = al_record(log, c);
  tf_align_exposure_iter* xrec = al_record(e.log, c);
  double pose[12], M[21], bb[6], xi[6], Ac[21], bc[6], S[kExpSums], pair[2], de[2];
#pragma unroll
  for (int i = 0; i < 12; ++i) pose[i] = pose_d[i];
  pair[0] = e.x->pair_d[0]; pair[1] = e.x->pair_d[1];
  const AlEval ev = al_fill_iter(&rec->geo, a, [&](int i) { return al_total(red, i); }, pose, M, bb);
#pragma unroll
  for (int i = 0; i < 21; ++i) { Ac[i] = al_total(red, kAlRow + kAlA + i); rec->Ac[i] = Ac[i]; }
#pragma unroll
  for (int i = 0; i < 6; ++i) { bc[i] = al_total(red, kAlRow + kAlB + i); rec->bc[i] = bc[i]; }
#pragma unroll
  for (int i = 0; i < kExpSums; ++i) S[i] = al_total(red, 2 * kAlRow + i);
  const AlPhotoEval ph = al_fill_photo(rec, red, c);
  ExposureElim el;
  exposure_eliminate(S, e.unknowns, Ac, bc, &el);
#pragma unroll
  for (int i = 0; i < 21; ++i) M[i] = M[i] + l2 * Ac[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) bb[i] = bb[i] + l2 * bc[i];
  xrec->gain = pair[0]; xrec->offset = pair[1]; xrec->rank = el.rank; xrec->n_photo = ph.n_photo;
#pragma unroll
  for (int i = 0; i < 6; ++i) { xrec->P[i] = S[kExpP + i]; xrec->Q[i] = S[kExpQ + i]; }
  xrec->S_w = S[kExpSw]; xrec->S_l = S[kExpSl]; xrec->S_ll = S[kExpSll]; xrec->S_r = S[kExpSr]; xrec->S_lr = S[kExpSlr];
  xrec->d_offset = 0.0; xrec->d_gain = 0.0;
  al_count(c, ev);
  if (al_decide(c, a, ev.n_valid, M, bb, &rec->geo, xi)) {
    align_update(pose, xi);
    al_keep_pose(pose_d, pose_f, pose);
    exposure_step(S, el, xi, de);
    exposure_apply(pair, el.rank, de, e.min_gain, e.max_gain);
    xrec->d_offset = de[0]; xrec->d_gain = de[1];
    e.x->pair_d[0] = pair[0]; e.x->pair_d[1] = pair[1];
    e.x->pair_f[0] = (float)pair[0]; e.x->pair_f[1] = (float)pair[1];
  }
  *ctl = c;
  const bool held = c.status <= TF_ALIGN_MAX_ITERS;
  e.x->valid = held ? 1 : 0; e.x->n_eval = c.n_eval;
  if (a.closing && e.carry && held) { e.cell[0] = pair[0]; e.cell[1] = pair[1]; }
  al_fill_color_result(out, c, ev, ph, pose);
}

}  // namespace tf
