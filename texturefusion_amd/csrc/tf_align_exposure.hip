// tf_align_exposure.hip -- exposure compensation in the two photometric aligners (tf_align_frame_color,
// tf_align_frame_icp_color): the frame's luma is compensated by a gain and an offset before it is compared with the model's
// intensity, and the pair is estimated with the pose.  A setting of the handle (tf_align_set_exposure), off by default; with
// it on, the calls of tf_align_color.hip and tf_align_icp_color.hip enqueue this file's launches in place of their own begin,
// rows and solve (tf_align_exposure.h), their state blocks and logs staying theirs.  The method is this library's own;
// tests/align_exposure_ref.py restates it.
//
//   k_ealign_cell       one lane: a pair into the handle's cell (tf_align_set_exposure, and tf_track_frame_color's end)
//   k_ealign_begin      the caller's pose(s) into the aligner's state block, the control words cleared, and the call's start
//                       pair read from the cell (for the residual maps: the poses and the pair alone)
//   k_ealign_rows       k_calign_rows' row with the compensated luma and a third row of sums
//   k_ealign_proj_rows  k_cicp_rows' row the same way, the gated variant a template flag of it
//   k_ealign_solve      one workgroup: al_solve_color_exposure of tf_align_rows.h, for both aligners
//
// Per sampled pixel, all f32, every operation rounded on its own (-ffp-contract=off): the geometric row, flag bits, L, the
// gradient and the Jacobian Jc are the aligner's own (tf_align_color.hip's and tf_align_icp_color.hip's headers state them),
// Lf is formed exactly as there (al_luma), and
//   Lfe = gain_f * Lf + offset_f
//   rc = L(pw) - Lfe                              (the SDF form)
//   rc = (L[i] + (Gu[i] * du + Gv[i] * dv)) - Lfe (the projective form)
// with (gain_f, offset_f) the f32 roundings of the pair carried in f64 beside the pose.  The bound |rc| <= max_photo_residual
// (bit 6, bit 9 of the projective form) and the Huber weight wc use this rc.  With gain 1 and offset 0, Lfe is Lf bit for bit.
// Sums: the geometric and the photometric row's as before, and a third row of 32 doubles per tile and per workgroup through
// the same tree (al_exposure_row_sums): with wJc_i = wc * Jc_i and wl = wc * Lf (the uncompensated luma: the residual's
// derivative by the gain is -Lf), every operand an exact zero where the pixel is not photometrically valid, each entry the
// f64 product of two f32 operands:
//   P_i = wJc_i * 1, Q_i = wJc_i * Lf (i = 0..5), S_w = wc * 1, S_l = wc * Lf, S_ll = wl * Lf, S_r = wc * rc, S_lr = wl * rc
// (tf_align_tree.h states the entry order; entry 17 repeats n_photo).
// Solve: tf_align_exposure_solve.h -- the pair eliminated from the photometric system, then M = A_g + l2 Ac', b = b_g + l2 bc',
// damping, align_solve6 and al_decide exactly as without the setting; where a step is taken the pair moves by
// de = F^-1 (h + C^T xi) and the gain is clamped.  TF_ALIGN_TOO_FEW by the geometric count, the convergence test on the twist
// alone and the closing evaluation are unchanged; with photo_weight == 0 or on a volume without colour the photometric term
// is an exact zero, so pose, status and geometric sums are the plain call's bit for bit.
// The cell: two f64 (gain, offset) in device memory the handle owns.  The setter writes (gain0, offset0) there on the handle's
// stream; a call's begin launch reads its start from it; with carry on, the closing solve launch of a call that ended with
// status <= TF_ALIGN_MAX_ITERS writes its estimate there.  Nothing is read back by a call.
// LDS: the rows kernels' 8 x 96 doubles (6144 B), the solve's 8 x 96.  No atomics, no counters, no polling; every launch of a
// call is enqueued up front and reads one state word at its start.
//
// Not here: per-channel gains, vignetting, response curves, the group aligner, the depth pyramid, use of the estimate when
// the frame is integrated or in CompensateColor.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_exposure.h"
#include "tf_align_icp_normal.h"
#include "tf_align_icp_rows.h"
#include "tf_align_rows.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct EalignDev {
  AlExposureCtl* x;
  tf_align_exposure_iter* log;  // [TF_ALIGN_MAX_EVALUATIONS]
  double* part;                 // [ceil(cap_tiles / kAlWaves)][kCeRow]: three rows per workgroup of the rows kernels
};
struct EalignPoses {
  AlignPose p;
  float m[12];
  int has_model;
};
struct EalignSolveArgs {
  AlignSolveCommon c;
  double l2;  // photo_weight squared
  tf_align_color_result* out;
  AlExposureArgs e;
};

__global__ __launch_bounds__(64) void k_ealign_cell(double* cell, double gain, double offset) {
  if (threadIdx.x == 0) { cell[0] = gain; cell[1] = offset; }
}

__global__ __launch_bounds__(64) void k_ealign_begin(ExposureOwn o, AlExposureCtl* x, const double* cell, EalignPoses p,
                                                     int residuals_only) {
  al_begin(o.ctl, o.pose_d, o.pose_f, o.pose_r, p.p, residuals_only);
  const int i = threadIdx.x;
  if (p.has_model && i < 12) (residuals_only ? o.pose_r : o.pose_f)[12 + i] = p.m[i];
  if (i == 0) {
    const double g = cell[0], f = cell[1];
    if (residuals_only) {
      x->pair_r[0] = (float)g; x->pair_r[1] = (float)f;
    } else {
      x->pair_d[0] = g; x->pair_d[1] = f;
      x->pair_f[0] = (float)g; x->pair_f[1] = (float)f;
      x->valid = 0; x->n_eval = 0;
    }
  }
}

// (resources of every kernel here: tests/test_kernel_resources_align_exposure.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_ealign_rows(VolumeDev v, CAlignRowsArgs a, const float* pair) {
  if (a.state && al_idle(a.state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  AlSdfRow row{};
  uint32_t fl = 0;
  float rc = 0.f, lf = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  if (px.in) {
    const size_t o = (size_t)px.Y * a.c.W + (size_t)px.X;
    const float z = a.depth[o];
    const uint32_t c8 = a.rgba[o];
    AlLumRow lum{};
    row = al_sdf_row<true>(v, a.c, a.res, px, z, a.pose, &lum);
    fl = row.fl;
    if (fl == 15u && (c8 >> 24) != 0u && lum.okl) {
      fl |= 16u;
      lf = al_luma(c8);
      rc = lum.lc - al_luma_exposed(lf, pair);
      if (lum.okt) {
        fl |= 32u;
        cx = lum.cx; cy = lum.cy; cz = lum.cz;
        if (fabsf(rc) <= a.max_photo_residual) fl |= 64u;
      }
    }
    if (a.r) a.r[o] = row.s;
    if (a.grad) { a.grad[o] = row.gx; a.grad[a.plane + o] = row.gy; a.grad[2 * a.plane + o] = row.gz; }
    if (a.rc) a.rc[o] = rc;
    if (a.gradc) { a.gradc[o] = cx; a.gradc[a.plane + o] = cy; a.gradc[2 * a.plane + o] = cz; }
    if (a.flags) a.flags[o] = fl;
  }
  if (!a.part) return;
  __shared__ double wsum[kAlWaves][kCeRow];
  const bool photo = fl == 127u;
  al_row_sums(wsum, 0, px, row.gx, row.gy, row.gz, row.qx, row.qy, row.qz, row.s, a.c.huber, (fl & 15u) == 15u, px.in);
  al_row_sums(wsum, kAlRow, px, cx, cy, cz, row.qx, row.qy, row.qz, rc, a.huber_photo, photo, photo);
  al_exposure_row_sums(wsum, 2 * kAlRow, px, cx, cy, cz, row.qx, row.qy, row.qz, rc, lf, a.huber_photo, photo);
  al_store_rows(wsum, a.part + (size_t)blockIdx.x * kCeRow);
}

template <bool kGate>
__global__ __launch_bounds__(kAlWaves * 64) void k_ealign_proj_rows(CicpRowsArgs a, const float* pair) {
  const IcpRowsArgs& g = a.icp;
  if (g.state && al_idle(g.state, g.c.level)) return;
  const AlPixel px = al_pixel(g.c);
  uint32_t fl = 0;
  int32_t as = -1;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  float rc = 0.f, lf = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  AlPoint p{};
  if (px.in) {
    const size_t o = (size_t)px.Y * g.c.W + (size_t)px.X;
    FnTaps t{};
    if (kGate) t = fn_taps(g.c, px, g.depth, o);
    else t.z0 = g.depth[o];
    const uint32_t c8 = a.rgba[o];
    if (al_point(g.c, px, t.z0, g.pose, &p)) {
      IcpPhoto ph;
      ph.L = a.L; ph.Gu = a.Gu; ph.Gv = a.Gv;
      const IcpAssoc m = icp_assoc(g, p, &ph);
      fl = m.fl; as = m.as;
      s = m.s; gx = m.gx; gy = m.gy; gz = m.gz;
      if (kGate) fl |= fn_gate_bits(fl, frame_normal(g.c, px, t, a.max_jump), g.pose, gx, gy, gz, m.m2, a.c2);
      const bool usable = ph.l >= 0.f && ph.gu == ph.gu && ph.gv == ph.gv;
      if (fl == (kGate ? 63u : 15u) && (c8 >> 24) != 0u && usable) {
        fl |= 256u;
        lf = al_luma(c8);
        const float du = ph.uc - ph.uf, dv = ph.vc - ph.vf;
        rc = (ph.l + (ph.gu * du + ph.gv * dv)) - al_luma_exposed(lf, pair);
        const float ja = (g.c.fx * ph.gu) / ph.mz, jb = (g.c.fy * ph.gv) / ph.mz;
        const float jc = -((ja * ph.mx + jb * ph.my) / ph.mz);
        const float* M = g.pose + 12;
        cx = (M[0] * ja + M[1] * jb) + M[2] * jc;
        cy = (M[4] * ja + M[5] * jb) + M[6] * jc;
        cz = (M[8] * ja + M[9] * jb) + M[10] * jc;
        if (fabsf(rc) <= a.max_photo_residual) fl |= 512u;
      }
    }
    if (g.r) g.r[o] = s;
    if (a.rc) a.rc[o] = rc;
    if (g.flags) g.flags[o] = fl;
    if (g.assoc) g.assoc[o] = as;
    if (a.gradc) { a.gradc[o] = cx; a.gradc[g.plane + o] = cy; a.gradc[2 * g.plane + o] = cz; }
  }
  if (!g.part) return;
  __shared__ double wsum[kAlWaves][kCeRow];
  const bool photo = (fl & 512u) != 0u;
  al_row_sums(wsum, 0, px, gx, gy, gz, p.qx, p.qy, p.qz, s, g.c.huber, (fl & 255u) == (kGate ? 63u : 15u), px.in);
  al_row_sums(wsum, kAlRow, px, cx, cy, cz, p.qx, p.qy, p.qz, rc, a.huber_photo, photo, photo);
  al_exposure_row_sums(wsum, 2 * kAlRow, px, cx, cy, cz, p.qx, p.qy, p.qz, rc, lf, a.huber_photo, photo);
  al_store_rows(wsum, g.part + (size_t)blockIdx.x * kCeRow);
}

__global__ __launch_bounds__(256) void k_ealign_solve(ExposureOwn o, const double* part, EalignSolveArgs a) {
  al_solve_color_exposure(o.ctl, o.log, o.pose_d, o.pose_f, part, a.c, a.l2, a.out, a.e);
}

// the state block as it lies in AlignExposureState::st[which] (base == null: its size)
EalignDev ealign_carve(void* base, size_t cap_tiles, size_t* bytes) {
  EalignDev d{};
  Carver c(base);
  c.take(d.x, 1);
  c.take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kCeRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = c.L.size;
  return d;
}
int ealign_dev(tf_volume* v, int which, EalignDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; ealign_carve(nullptr, tiles, &n); return n; };
  AlignBlock& s = v->align_exposure.st[which];
  const int rc = align_ensure(v, s, bytes_of, sizeof(AlExposureCtl));
  if (rc) return rc;
  *d = ealign_carve(s.block.p, s.cap_tiles, nullptr);
  return TF_OK;
}

bool exposure_ok(const tf_align_exposure* e) {
  const float f[4] = {e->gain0, e->offset0, e->min_gain, e->max_gain};
  if (e->unknowns < 0 || e->unknowns > 2) { set_error("align exposure: unknowns must be 0, 1 or 2"); return false; }
  if (!finite_all(f, 4) || !(e->min_gain > 0.f) || e->min_gain > e->max_gain || e->gain0 < e->min_gain || e->gain0 > e->max_gain) {
    set_error("align exposure: fields must be finite, 0 < min_gain <= gain0 <= max_gain");
    return false;
  }
  return true;
}

EalignPoses poses_of(const float* pose, const float* model_pose) {
  EalignPoses P{};
  memcpy(P.p.p, pose, sizeof(P.p.p));
  if (model_pose) { memcpy(P.m, model_pose, sizeof(P.m)); P.has_model = 1; }
  return P;
}

AlExposureArgs solve_exposure_args(const tf_volume* v, const EalignDev& d) {
  const AlignExposureState& s = v->align_exposure;
  AlExposureArgs e{};
  e.x = d.x; e.log = d.log; e.cell = s.cell.as<double>();
  e.unknowns = s.e.unknowns; e.carry = (s.e.carry != 0 || s.hold_carry) ? 1 : 0;
  e.min_gain = (double)s.e.min_gain; e.max_gain = (double)s.e.max_gain;
  return e;
}

void proj_rows_launch(tf_volume* v, const CicpRowsArgs& a, const float* pair, uint32_t n_rows) {
  if (icp_gate_on(v)) hipLaunchKernelGGL(k_ealign_proj_rows<true>, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, a, pair);
  else hipLaunchKernelGGL(k_ealign_proj_rows<false>, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, a, pair);
}

}  // namespace

bool exposure_on(const tf_volume* v) { return v->align_exposure.on; }
void exposure_not_run(tf_volume* v, int which) { v->align_exposure.ran[which] = false; }

int exposure_sdf_enqueue(tf_volume* v, const ExposureOwn& o, const AlignPose& start, CAlignRowsArgs ra, const tf_align_params& geo,
                         double l2, tf_align_color_result* d_result) {
  EalignDev d;
  const int rc = ealign_dev(v, 0, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  v->align_exposure.ran[0] = true;
  hipLaunchKernelGGL(k_ealign_begin, dim3(1), dim3(64), 0, st, o, d.x, v->align_exposure.cell.as<const double>(),
                     poses_of(start.p, nullptr), 0);
  const AlExposureArgs ea = solve_exposure_args(v, d);
  ra.pose = o.pose_f; ra.state = &o.ctl->state; ra.part = d.part;
  align_walk(v, geo, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    ra.c = c;
    ra.plane = (size_t)c.W * c.H;
    hipLaunchKernelGGL(k_ealign_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra, d.x->pair_f);
    hipLaunchKernelGGL(k_ealign_solve, dim3(1), dim3(256), 0, st, o, d.part, EalignSolveArgs{sc, l2, d_result, ea});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int exposure_proj_enqueue(tf_volume* v, const ExposureOwn& o, const float* pose, const float* model_pose, CicpRowsArgs ra,
                          const tf_align_params& geo, double l2, tf_align_color_result* d_result) {
  EalignDev d;
  const int rc = ealign_dev(v, 1, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  v->align_exposure.ran[1] = true;
  hipLaunchKernelGGL(k_ealign_begin, dim3(1), dim3(64), 0, st, o, d.x, v->align_exposure.cell.as<const double>(),
                     poses_of(pose, model_pose), 0);
  const AlExposureArgs ea = solve_exposure_args(v, d);
  ra.icp.pose = o.pose_f; ra.icp.state = &o.ctl->state; ra.icp.part = d.part;
  align_walk(v, geo, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    ra.icp.c = c;
    ra.icp.plane = (size_t)c.W * c.H;
    proj_rows_launch(v, ra, d.x->pair_f, sc.n_rows);
    hipLaunchKernelGGL(k_ealign_solve, dim3(1), dim3(256), 0, st, o, d.part, EalignSolveArgs{sc, l2, d_result, ea});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int exposure_sdf_residuals(tf_volume* v, const ExposureOwn& o, const AlignPose& pose, CAlignRowsArgs ra, uint32_t n_rows) {
  EalignDev d;
  const int rc = ealign_dev(v, 0, &d);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ealign_begin, dim3(1), dim3(64), 0, v->stream, o, d.x, v->align_exposure.cell.as<const double>(),
                     poses_of(pose.p, nullptr), 1);
  ra.pose = o.pose_r;
  hipLaunchKernelGGL(k_ealign_rows, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, v->dev, ra, d.x->pair_r);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int exposure_proj_residuals(tf_volume* v, const ExposureOwn& o, const float* pose, const float* model_pose, CicpRowsArgs ra,
                            uint32_t n_rows) {
  EalignDev d;
  const int rc = ealign_dev(v, 1, &d);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ealign_begin, dim3(1), dim3(64), 0, v->stream, o, d.x, v->align_exposure.cell.as<const double>(),
                     poses_of(pose, model_pose), 1);
  ra.icp.pose = o.pose_r;
  proj_rows_launch(v, ra, d.x->pair_r, n_rows);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int exposure_track_stage(tf_volume* v, int stage) {
  AlignExposureState& s = v->align_exposure;
  if (!s.on) return TF_OK;
  s.hold_carry = stage == 1;
  if (stage == 2 && s.e.carry == 0) {
    hipLaunchKernelGGL(k_ealign_cell, dim3(1), dim3(64), 0, v->stream, s.cell.as<double>(), (double)s.e.gain0, (double)s.e.offset0);
    TF_HIP(hipGetLastError());
  }
  return TF_OK;
}

void align_exposure_release(tf_volume* v) { v->align_exposure = AlignExposureState{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_exposure_default(tf_align_exposure* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_align_exposure e{};
  e.unknowns = 2; e.carry = 0;
  e.gain0 = 1.0f; e.offset0 = 0.0f;
  e.min_gain = 0.25f; e.max_gain = 4.0f;  // not tuned on recorded data
  *out = e;
  return TF_OK;
}

int tf_align_set_exposure(tf_volume* v, const tf_align_exposure* e) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  if (e && !exposure_ok(e)) return TF_ERR_INVALID;
  TF_DEV(v);
  AlignExposureState& s = v->align_exposure;
  if (!e) {
    s.on = false;
    s.e = tf_align_exposure{};
    return TF_OK;
  }
  if (!s.cell) {
    const int rc = s.cell.alloc(2 * sizeof(double));
    if (rc) return rc;
  }
  s.on = true;
  s.e = *e;
  hipLaunchKernelGGL(k_ealign_cell, dim3(1), dim3(64), 0, v->stream, s.cell.as<double>(), (double)e->gain0, (double)e->offset0);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int tf_align_get_exposure(tf_volume* v, tf_align_exposure* out, int32_t* on) {
  if (!v || !out || !on) { set_error("null argument"); return TF_ERR_INVALID; }
  *out = v->align_exposure.e;
  *on = v->align_exposure.on ? 1 : 0;
  return TF_OK;
}

int tf_align_exposure_log(tf_volume* v, int32_t which, tf_align_exposure_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  if (which < 0 || which > 1) { set_error("align exposure: which must be 0 or 1"); return TF_ERR_INVALID; }
  if (!n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  const AlignExposureState& s = v->align_exposure;
  if (!s.st[which].block || !s.ran[which]) return TF_OK;
  const EalignDev d = ealign_carve(s.st[which].block.p, s.st[which].cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  AlExposureCtl x;
  TF_HIP(hipMemcpy(&x, d.x, sizeof(x), hipMemcpyDeviceToHost));
  const int64_t have = x.n_eval < 0 ? 0 : (x.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : x.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0) TF_HIP(hipMemcpy(out, d.log, (size_t)m * sizeof(tf_align_exposure_iter), hipMemcpyDeviceToHost));
  return TF_OK;
}

int tf_align_exposure_estimate(tf_volume* v, int32_t which, double gain_offset[2], int32_t* valid) {
  if (!v || !gain_offset || !valid) { set_error("null argument"); return TF_ERR_INVALID; }
  if (which < 0 || which > 1) { set_error("align exposure: which must be 0 or 1"); return TF_ERR_INVALID; }
  gain_offset[0] = 1.0; gain_offset[1] = 0.0;
  *valid = 0;
  TF_DEV_READER(v);
  const AlignExposureState& s = v->align_exposure;
  if (!s.st[which].block || !s.ran[which]) return TF_OK;
  const EalignDev d = ealign_carve(s.st[which].block.p, s.st[which].cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  AlExposureCtl x;
  TF_HIP(hipMemcpy(&x, d.x, sizeof(x), hipMemcpyDeviceToHost));
  gain_offset[0] = x.pair_d[0]; gain_offset[1] = x.pair_d[1];
  *valid = x.valid;
  return TF_OK;
}

}  // extern "C"
