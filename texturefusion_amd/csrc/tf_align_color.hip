// tf_align_color.hip -- frame-to-model alignment by colour as well as depth: tf_align.hip's geometric rows with a
// photometric row beside each, so that the pose is held inside a surface too (a wall, a floor, a table top, where the SDF's
// gradient is blind).  The method is this library's own; tests/align_color_ref.py restates it.
//
//   k_calign_begin  one lane: the caller's pose into the state block (f64 and f32), the control words cleared
//   k_calign_rows   one wave per 8 x 8 tile of sampled pixels, eight waves per workgroup, as k_align_rows: the geometric and
//                   the photometric row of each pixel and the wave's share of both sets of sums; with map outputs, the maps
//                   of tf_align_color_residuals -- one body
//   k_calign_solve  one workgroup: the partials combined in tile order, the two systems joined, the 6 x 6 solve and the pose
//                   update by one lane (tf_align_solve.h), a log record, the result: al_solve_color of tf_align_rows.h,
//                   which the projective aligner with a photometric row runs too
//
// Per sampled pixel (x, y), all f32, every operation rounded on its own (-ffp-contract=off).  The geometric row is
// k_align_rows' row unchanged: z, pc, q, pw = t + q, the seven sample points pw and pw -+ res e_a, flag bits 0 to 3, r = s,
// g, J = [g, q x g], the Huber weight w (tf_align.hip's header).  On top of it, with tri_sample_lum (tf_ray_devfn.h) giving
// the SDF and the model intensity L of a point from the same eight corners:
//   (r8, g8, b8, a8) = the pixel's RGBA8;  Lf = ((0.299f * r8 + 0.587f * g8) + 0.114f * b8) * (1.0f / 255.0f)
//   bits 0..3 all set, a8 != 0 and L(pw) valid                                                                  (bit 4)
//   L(pw -+ res e_a) valid for a = x, y, z                                                                      (bit 5: all six)
//   rc = L(pw) - Lf;  gc_a = (L(pw + res e_a) - L(pw - res e_a)) * (0.5f / res);  |rc| <= max_photo_residual    (bit 6)
//   each bit is set only where the lower ones are; the pixel is photometrically valid iff flags == 127, geometrically valid
//   iff (flags & 15) == 15.
//   Jc = (gc.x, gc.y, gc.z, q.y gc.z - q.z gc.y, q.z gc.x - q.x gc.z, q.x gc.y - q.y gc.x)
//   wc = 1 if huber_photo == 0 or |rc| <= huber_photo, else huber_photo / |rc|;  wJc_i = wc * Jc_i,  wrc = wc * rc
// Sums: the 31 geometric ones as tf_align.hip's; over the photometrically valid pixels A_c[21], b_c[6], sum_rc2, sum_wrc2 and
// n_photo by the same products in f64 through the same functions (tf_align_rows.h: al_row_sums twice, al_add_rows over
// rows of 64 doubles): a second row of 32 doubles per tile and per workgroup (entry 30 repeats n_photo).
// Solve: M = A_g + l2 * A_c and b = b_g + l2 * b_c entry by entry in f64 with l2 = (double)photo_weight * (double)photo_weight,
// then tf_align_frame's damping, solve, update and stop rules (al_decide).  TF_ALIGN_TOO_FEW goes by the geometric n_valid.
// With photo_weight == 0 or on a volume without colour the second term is an exact zero: pose, status and every geometric
// sum are tf_align_frame's bit for bit.
// With tf_align_set_exposure on, Lf is compensated by a gain and an offset that are estimated with the pose: the launches of
// a call are tf_align_exposure.hip's then (its header states them), this file's state block and log stay the call's.
// No atomics, no counters, no polling; every launch of a call is enqueued up front and reads one state word at its start.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_exposure.h"
#include "tf_align_rows.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct CAlignDev {
  AlignCtl* ctl;
  double* pose_d;             // [12] the pose between iterations
  float* pose_f;              // [12] the same rounded: what k_calign_rows samples at
  float* pose_r;              // [12] tf_align_color_residuals' pose (the last alignment's state stays as it is)
  double* part;               // [ceil(cap_tiles / kAlWaves)][kCaRow]: two rows per workgroup of k_calign_rows
  tf_align_color_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
};

struct CAlignSolveArgs {
  AlignSolveCommon c;
  double l2;  // photo_weight squared
  tf_align_color_result* out;
};

__global__ __launch_bounds__(64) void k_calign_begin(CAlignDev d, AlignPose p, int residuals_only) {
  al_begin(d.ctl, d.pose_d, d.pose_f, d.pose_r, p, residuals_only);
}

// (resources: tests/test_kernel_resources_align_color.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_calign_rows(VolumeDev v, CAlignRowsArgs a) {
  if (a.state && al_idle(a.state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  AlSdfRow row{};
  uint32_t fl = 0;
  float rc = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  if (px.in) {
    const size_t o = (size_t)px.Y * a.c.W + (size_t)px.X;
    const float z = a.depth[o];
    const uint32_t c8 = a.rgba[o];
    AlLumRow lum{};
    row = al_sdf_row<true>(v, a.c, a.res, px, z, a.pose, &lum);
    fl = row.fl;
    if (fl == 15u && (c8 >> 24) != 0u && lum.okl) {
      fl |= 16u;
      const float lf = al_luma(c8);
      rc = lum.lc - lf;
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
  // the geometric row's sums, exactly as k_align_rows forms them, and the photometric row's through the same tree: n_photo
  // takes the place of both counts
  __shared__ double wsum[kAlWaves][kCaRow];
  al_row_sums(wsum, 0, px, row.gx, row.gy, row.gz, row.qx, row.qy, row.qz, row.s, a.c.huber, (fl & 15u) == 15u, px.in);
  al_row_sums(wsum, kAlRow, px, cx, cy, cz, row.qx, row.qy, row.qz, rc, a.huber_photo, fl == 127u, fl == 127u);
  al_store_rows(wsum, a.part + (size_t)blockIdx.x * kCaRow);
}

__global__ __launch_bounds__(256) void k_calign_solve(CAlignDev d, CAlignSolveArgs a) {
  al_solve_color(d.ctl, d.log, d.pose_d, d.pose_f, d.part, a.c, a.l2, a.out);
}

// the state block as it lies in tf_volume::align_color (base == null: its size)
CAlignDev calign_carve(void* base, size_t cap_tiles, size_t* bytes) {
  CAlignDev d{};
  Carver c(base);
  c.take(d.ctl, 1);
  c.take(d.pose_d, 12);
  c.take(d.pose_f, 12);
  c.take(d.pose_r, 12);
  c.take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kCaRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = c.L.size;
  return d;
}
int calign_dev(tf_volume* v, CAlignDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; calign_carve(nullptr, tiles, &n); return n; };
  const int rc = align_ensure(v, v->align_color, bytes_of, sizeof(AlignCtl));
  if (rc) return rc;
  *d = calign_carve(v->align_color.block.p, v->align_color.cap_tiles, nullptr);
  return TF_OK;
}

int calign_check(tf_volume* v, const float* depth, const void* rgba, const float* pose, const tf_align_color_params* p,
                 bool with_iters) {
  if (!p || !rgba) { set_error("null argument"); return TF_ERR_INVALID; }
  const int rc = align_check(v, depth, pose, &p->geo, with_iters);
  if (rc) return rc;
  const float f[3] = {p->photo_weight, p->max_photo_residual, p->huber_photo};
  if (!finite_all(f, 3) || p->photo_weight < 0.f || p->max_photo_residual < 0.f || p->huber_photo < 0.f) {
    set_error("align: photo_weight, max_photo_residual, huber_photo must be finite and >= 0");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

CAlignRowsArgs crows_args(const tf_volume* v, const AlignRowsCommon& rc, const tf_align_color_params& cp, const float* d_depth,
                          const uint8_t* d_rgba) {
  CAlignRowsArgs a{};
  a.c = rc;
  a.depth = d_depth;
  a.rgba = reinterpret_cast<const uint32_t*>(d_rgba);
  a.res = v->res; a.max_photo_residual = cp.max_photo_residual; a.huber_photo = cp.huber_photo;
  a.plane = (size_t)rc.W * rc.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close
int calign_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose,
                   const tf_align_color_params& cp, tf_align_color_result* d_result) {
  CAlignDev d;
  int rc = calign_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  AlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  const double l2 = (double)cp.photo_weight * (double)cp.photo_weight;
  if (exposure_on(v))  // tf_align_set_exposure: the launches are tf_align_exposure.hip's, state and log stay this file's
    return exposure_sdf_enqueue(v, ExposureOwn{d.ctl, d.pose_d, d.pose_f, d.pose_r, d.log}, P,
                                crows_args(v, AlignRowsCommon{}, cp, d_depth, d_rgba), cp.geo, l2, d_result);
  exposure_not_run(v, 0);
  hipLaunchKernelGGL(k_calign_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  align_walk(v, cp.geo, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    CAlignRowsArgs ra = crows_args(v, c, cp, d_depth, d_rgba);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    hipLaunchKernelGGL(k_calign_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra);
    hipLaunchKernelGGL(k_calign_solve, dim3(1), dim3(256), 0, st, d, CAlignSolveArgs{sc, l2, d_result});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int cresiduals_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose,
                       const tf_align_color_params& cp, float* d_r, float* d_grad3, float* d_rc, float* d_gradc3,
                       uint32_t* d_flags) {
  CAlignDev d;
  int rc = calign_dev(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  AlignRowsCommon c;
  AlignSolveCommon sc;
  align_level(v, cp.geo, 0, &c, &sc);
  CAlignRowsArgs ra = crows_args(v, c, cp, d_depth, d_rgba);
  ra.pose = d.pose_r; ra.r = d_r; ra.grad = d_grad3; ra.rc = d_rc; ra.gradc = d_gradc3; ra.flags = d_flags;
  if (c.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_grad3) TF_HIP(hipMemsetAsync(d_grad3, 0, 12 * ra.plane, st));
    if (d_rc) TF_HIP(hipMemsetAsync(d_rc, 0, 4 * ra.plane, st));
    if (d_gradc3) TF_HIP(hipMemsetAsync(d_gradc3, 0, 12 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
  }
  AlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  if (exposure_on(v))
    return exposure_sdf_residuals(v, ExposureOwn{d.ctl, d.pose_d, d.pose_f, d.pose_r, d.log}, P, ra, sc.n_rows);
  hipLaunchKernelGGL(k_calign_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  hipLaunchKernelGGL(k_calign_rows, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

void align_color_release(tf_volume* v) { v->align_color = AlignBlock{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_color_default_params(tf_align_color_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_align_color_params p{};
  const int rc = tf_align_default_params(&p.geo);
  if (rc) return rc;
  p.photo_weight = 0.1f; p.max_photo_residual = 0.25f; p.huber_photo = 0.05f;
  *out = p;
  return TF_OK;
}

int tf_align_frame_color_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                const tf_align_color_params* params, tf_align_color_result* d_result) {
  int rc = calign_check(v, d_depth, d_rgba, pose, params, true);
  if (rc) return rc;
  if (!d_result) { set_error("null argument"); return TF_ERR_INVALID; }
  if (reinterpret_cast<uintptr_t>(d_rgba) & 3u) { set_error("device rgba image must be 4-byte aligned"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  return calign_enqueue(v, d_depth, d_rgba, pose, *params, d_result);
}

int tf_align_frame_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                         const tf_align_color_params* params, tf_align_color_result* result) {
  int rc = calign_check(v, depth, rgba, pose, params, true);
  if (rc) return rc;
  if (!result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take(4 * P), o_r = L.take(sizeof(tf_align_color_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgba, 4 * P)))
    return rc;
  if ((rc = calign_enqueue(v, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), pose, *params,
                           sg.dp<tf_align_color_result>(o_r))))
    return rc;
  return stage_out(v, sg, o_r, sizeof(tf_align_color_result), result);
}

int tf_align_color_log(tf_volume* v, tf_align_color_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  const AlignBlock& s = v->align_color;
  const CAlignDev d = s.block ? calign_carve(s.block.p, s.cap_tiles, nullptr) : CAlignDev{};
  return align_log(v, d.ctl, d.log, sizeof(tf_align_color_iter), out, cap, n);
}

int tf_align_color_residuals_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                    const tf_align_color_params* params, float* d_r, float* d_grad3, float* d_rc,
                                    float* d_gradc3, uint32_t* d_flags) {
  int rc = calign_check(v, d_depth, d_rgba, pose, params, false);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_rgba) & 3u) { set_error("device rgba image must be 4-byte aligned"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!d_r && !d_grad3 && !d_rc && !d_gradc3 && !d_flags) return TF_OK;
  return cresiduals_enqueue(v, d_depth, d_rgba, pose, *params, d_r, d_grad3, d_rc, d_gradc3, d_flags);
}

int tf_align_color_residuals(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                             const tf_align_color_params* params, float* r, float* grad3, float* rc_map, float* gradc3,
                             uint32_t* flags) {
  int rc = calign_check(v, depth, rgba, pose, params, false);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (!r && !grad3 && !rc_map && !gradc3 && !flags) return TF_OK;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take(4 * P), o_r = L.take(r ? 4 * P : 0), o_g = L.take(grad3 ? 12 * P : 0),
               o_rc = L.take(rc_map ? 4 * P : 0), o_gc = L.take(gradc3 ? 12 * P : 0), o_f = L.take(flags ? 4 * P : 0);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgba, 4 * P)))
    return rc;
  rc = cresiduals_enqueue(v, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), pose, *params,
                          r ? sg.dp<float>(o_r) : nullptr, grad3 ? sg.dp<float>(o_g) : nullptr,
                          rc_map ? sg.dp<float>(o_rc) : nullptr, gradc3 ? sg.dp<float>(o_gc) : nullptr,
                          flags ? sg.dp<uint32_t>(o_f) : nullptr);
  if (rc) return rc;
  if ((rc = stage_out(v, sg, o_r, L.size - o_r, nullptr))) return rc;
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (grad3) memcpy(grad3, sg.h + o_g, 12 * P);
  if (rc_map) memcpy(rc_map, sg.h + o_rc, 4 * P);
  if (gradc3) memcpy(gradc3, sg.h + o_gc, 12 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  return TF_OK;
}

}  // extern "C"
