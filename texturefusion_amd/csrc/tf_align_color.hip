// tf_align_color.hip -- frame-to-model alignment by colour as well as depth: tf_align.hip's geometric rows with a
// photometric row beside each, so that the pose is held inside a surface too (a wall, a floor, a table top, where the SDF's
// gradient is blind).  The method is this library's own; tests/align_color_ref.py restates it.
//
//   k_calign_begin  one lane: the caller's pose into the state block (f64 and f32), the control words cleared
//   k_calign_rows   one wave per 8 x 8 tile of sampled pixels, eight waves per workgroup, as k_align_rows: the geometric and
//                   the photometric row of each pixel and the wave's share of both sets of sums; with map outputs, the maps
//                   of tf_align_color_residuals -- one body
//   k_calign_solve  one workgroup: the partials combined in tile order, the two systems joined, the 6 x 6 solve and the pose
//                   update by one lane (tf_align_solve.h), a log record, the result
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
// n_photo by the same products in f64, through the same tree (tf_align_tree.h) in the same order: a second row of 32 doubles
// per tile and per workgroup (entry 30 repeats n_photo).  k_calign_solve adds the rows g, g + 8, g + 16, .. in ascending
// order (g = 0..7), then the eight in order, for both rows alike.
// Solve: M = A_g + l2 * A_c and b = b_g + l2 * b_c entry by entry in f64 with l2 = (double)photo_weight * (double)photo_weight,
// then tf_align_frame's damping, align_solve6, align_update and stop rules.  TF_ALIGN_TOO_FEW goes by the geometric n_valid.
// With photo_weight == 0 or on a volume without colour the second term is an exact zero: pose, status and every geometric
// sum are tf_align_frame's bit for bit.
// No atomics, no counters, no polling; every launch of a call is enqueued up front and reads one state word at its start.
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

constexpr int kCaRow = 2 * kAlRow;   // doubles of a workgroup's partial sums: the geometric row, then the photometric one

struct CAlignCtl {
  uint32_t state;  // bit 0: stopped (too few / singular), bits 8..: levels finished
  int32_t status;
  int32_t n_eval;
  int32_t n_valid_first;
  float rms_first;
  int32_t n_photo_first;
  float rms_photo_first;
  uint32_t pad;
};
struct CAlignDev {
  CAlignCtl* ctl;
  double* pose_d;             // [12] the pose between iterations
  float* pose_f;              // [12] the same rounded: what k_calign_rows samples at
  float* pose_r;              // [12] tf_align_color_residuals' pose (the last alignment's state stays as it is)
  double* part;               // [ceil(cap_tiles / kAlWaves)][kCaRow]: two rows per workgroup of k_calign_rows
  tf_align_color_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
  uint32_t cap_tiles;         // tiles of the camera at stride 1
};
struct CAlignPose { float p[12]; };

struct CAlignRowsArgs {
  const float* depth;
  const uint32_t* rgba;   // RGBA8, one word per pixel (r in the low byte)
  const float* pose;      // 12 floats in the state block
  const uint32_t* state;  // null: always run (tf_align_color_residuals)
  float fx, fy, cxs, cys;
  int W, H, tiles_x, stride, level;
  float min_depth, max_depth, max_residual, huber, res, max_photo_residual, huber_photo;
  size_t plane;
  float* r;
  float* grad;
  float* rc;
  float* gradc;
  uint32_t* flags;
  double* part;  // null: no sums
};
struct CAlignSolveArgs {
  int level, log_level, stride, closing, last_level;
  uint32_t n_rows;  // workgroups of the rows launch
  float damping, eps_t, eps_r;
  int min_valid;
  double l2;  // photo_weight squared
  tf_align_color_result* out;
};

__device__ __forceinline__ bool cal_idle(const uint32_t* state, int level) {
  const uint32_t st = *state;
  return (st & 1u) || (uint32_t)level < (st >> 8);
}

__global__ __launch_bounds__(64) void k_calign_begin(CAlignDev d, CAlignPose p, int residuals_only) {
  const int i = threadIdx.x;
  if (residuals_only) {
    if (i < 12) d.pose_r[i] = p.p[i];
    return;
  }
  if (i < 12) { d.pose_d[i] = (double)p.p[i]; d.pose_f[i] = p.p[i]; }
  if (i == 0) {
    CAlignCtl c{};
    c.status = TF_ALIGN_MAX_ITERS;
    *d.ctl = c;
  }
}

// (resources: tests/test_kernel_resources_align_color.py)
__global__ __launch_bounds__(kAlWaves * 64) void k_calign_rows(VolumeDev v, CAlignRowsArgs a) {
  if (a.state && cal_idle(a.state, a.level)) return;
  // (a tile beyond the last one of the level lies below the image: none of its lanes is inside)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x * kAlWaves + wave;
  const long long X = (long long)((tile % a.tiles_x) * 8 + (lane & 7)) * a.stride;
  const long long Y = (long long)((tile / a.tiles_x) * 8 + (lane >> 3)) * a.stride;
  const bool in = X < a.W && Y < a.H;
  uint32_t fl = 0;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
  float rc = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  if (in) {
    const size_t o = (size_t)Y * a.W + (size_t)X;
    const float z = a.depth[o];
    if (isfinite(z) && z >= a.min_depth && z <= a.max_depth) {
      fl = 1u;
      const uint32_t px = a.rgba[o];
      const float res = a.res, ir = 1.0f / res;
      const float dcx = ((float)(int)X - a.cxs) / a.fx, dcy = ((float)(int)Y - a.cys) / a.fy;
      const float pcx = dcx * z, pcy = dcy * z;
      const float* P = a.pose;
      qx = (P[0] * pcx + P[1] * pcy) + P[2] * z;
      qy = (P[4] * pcx + P[5] * pcy) + P[6] * z;
      qz = (P[8] * pcx + P[9] * pcy) + P[10] * z;
      const float wx = P[3] + qx, wy = P[7] + qy, wz = P[11] + qz;
      ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
      float sc = 0.f, lc = 0.f;
      bool okl = false;
      if (tri_sample_lum(v, cc, wx, wy, wz, ir, &sc, &lc, &okl)) {
        fl |= 2u;
        s = sc;
        // tap k: axis k >> 1, minus / plus by k & 1, as k_align_rows
        float sp0 = 0.f, sp1 = 0.f, sp2 = 0.f, sm0 = 0.f, sm1 = 0.f, sm2 = 0.f;
        float lp0 = 0.f, lp1 = 0.f, lp2 = 0.f, lm0 = 0.f, lm1 = 0.f, lm2 = 0.f;
        bool ok = true, okt = true;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
          const int ax = k >> 1;
          float t = 0.f, l = 0.f;
          bool okk_l = false;
          const float h = (k & 1) ? res : -res;  // (a + (-b) is a - b)
          ChunkCache ct = cc;  // every tap starts from the centre's chunk
          const bool okk = tri_sample_lum(v, ct, ax == 0 ? wx + h : wx, ax == 1 ? wy + h : wy, ax == 2 ? wz + h : wz, ir, &t, &l,
                                          &okk_l);
          ok = ok && okk;
          okt = okt && okk_l;
          if (k == 0) { sm0 = t; lm0 = l; } else if (k == 1) { sp0 = t; lp0 = l; } else if (k == 2) { sm1 = t; lm1 = l; }
          else if (k == 3) { sp1 = t; lp1 = l; } else if (k == 4) { sm2 = t; lm2 = l; } else { sp2 = t; lp2 = l; }
        }
        if (ok) {
          fl |= 4u;
          const float h2 = 0.5f / res;
          gx = (sp0 - sm0) * h2; gy = (sp1 - sm1) * h2; gz = (sp2 - sm2) * h2;
          if (fabsf(s) <= a.max_residual) fl |= 8u;
          if (fl == 15u && (px >> 24) != 0u && okl) {
            fl |= 16u;
            const float r8 = (float)(px & 255u), g8 = (float)((px >> 8) & 255u), b8 = (float)((px >> 16) & 255u);
            const float lf = ((0.299f * r8 + 0.587f * g8) + 0.114f * b8) * (1.0f / 255.0f);
            rc = lc - lf;
            if (okt) {
              fl |= 32u;
              cx = (lp0 - lm0) * h2; cy = (lp1 - lm1) * h2; cz = (lp2 - lm2) * h2;
              if (fabsf(rc) <= a.max_photo_residual) fl |= 64u;
            }
          }
        }
      }
    }
    if (a.r) a.r[o] = s;
    if (a.grad) { a.grad[o] = gx; a.grad[a.plane + o] = gy; a.grad[2 * a.plane + o] = gz; }
    if (a.rc) a.rc[o] = rc;
    if (a.gradc) { a.gradc[o] = cx; a.gradc[a.plane + o] = cy; a.gradc[2 * a.plane + o] = cz; }
    if (a.flags) a.flags[o] = fl;
  }
  if (!a.part) return;
  const int e = al_entry(lane);
  __shared__ double wsum[kAlWaves][kCaRow];
  {  // the geometric row's sums, exactly as k_align_rows forms them (an exact zero in every term where not valid)
    const bool valid = (fl & 15u) == 15u;
    const float ar = fabsf(s);
    const float w = !valid ? 0.f : (a.huber == 0.f || ar <= a.huber) ? 1.0f : a.huber / ar;
    const float J[6] = {valid ? gx : 0.f, valid ? gy : 0.f, valid ? gz : 0.f, valid ? qy * gz - qz * gy : 0.f,
                        valid ? qz * gx - qx * gz : 0.f, valid ? qx * gy - qy * gx : 0.f};
    const double total = al_tile_sum(J, w, valid ? s : 0.f, valid ? 1.0f : 0.0f, in ? 1.0f : 0.0f, lane);
    if (!(lane & 1)) wsum[wave][e] = total;
  }
  {  // the photometric row's, through the same tree
    const bool valid = fl == 127u;
    const float ar = fabsf(rc);
    const float w = !valid ? 0.f : (a.huber_photo == 0.f || ar <= a.huber_photo) ? 1.0f : a.huber_photo / ar;
    const float J[6] = {valid ? cx : 0.f, valid ? cy : 0.f, valid ? cz : 0.f, valid ? qy * cz - qz * cy : 0.f,
                        valid ? qz * cx - qx * cz : 0.f, valid ? qx * cy - qy * cx : 0.f};
    const float pf = valid ? 1.0f : 0.0f;
    const double total = al_tile_sum(J, w, valid ? rc : 0.f, pf, pf, lane);
    if (!(lane & 1)) wsum[wave][kAlRow + e] = total;
  }
  // the workgroup's eight tiles in wave order, two plain-stored rows per workgroup
  __syncthreads();
  if (threadIdx.x < (unsigned)kCaRow) {
    double t = wsum[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kAlWaves; ++k) t += wsum[k][threadIdx.x];
    a.part[(size_t)blockIdx.x * kCaRow + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void k_calign_solve(CAlignDev d, CAlignSolveArgs a) {
  if (cal_idle(&d.ctl->state, a.level)) return;
  // thread (e = tid & 31, g = tid >> 5) adds entry e of both rows of the workgroups g, g + 8, g + 16, .. in ascending order,
  // then the eight groups in order: per geometric entry the additions of k_align_solve
  __shared__ double red[8][kCaRow];
  const uint32_t tid = threadIdx.x, e = tid & 31u, g = tid >> 5;
  double acc = 0.0, acc_c = 0.0;
  if (e < (uint32_t)kAlSums)
#pragma unroll 4
    for (uint32_t t = g; t < a.n_rows; t += 8u) {
      acc += d.part[(size_t)t * kCaRow + e];
      acc_c += d.part[(size_t)t * kCaRow + kAlRow + e];
    }
  red[g][e] = acc;
  red[g][kAlRow + e] = acc_c;
  __syncthreads();
  if (tid != 0) return;
  CAlignCtl c = *d.ctl;
  tf_align_color_iter* rec = d.log + (c.n_eval < TF_ALIGN_MAX_EVALUATIONS ? c.n_eval : TF_ALIGN_MAX_EVALUATIONS - 1);
  // entry i of both rows: the eight groups in order; the sums go to the record, the joined system stays in registers
  const auto total = [&](int i) {
    double t = red[0][i];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][i];
    return t;
  };
  double M[21], bb[6];
#pragma unroll
  for (int i = 0; i < 21; ++i) {
    const double tg = total(kAlA + i), tc = total(kAlRow + kAlA + i);
    rec->geo.A[i] = tg; rec->Ac[i] = tc;
    M[i] = tg + a.l2 * tc;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double tg = total(kAlB + i), tc = total(kAlRow + kAlB + i);
    rec->geo.b[i] = tg; rec->bc[i] = tc; rec->geo.xi[i] = 0.0;
    bb[i] = tg + a.l2 * tc;
  }
  const double sum_r2 = total(kAlR2), sum_rc2 = total(kAlRow + kAlR2);
  const int n_valid = (int)total(kAlNv), n_sampled = (int)total(kAlNs), n_photo = (int)total(kAlRow + kAlNv);
  const float rms = n_valid > 0 ? (float)sqrt(sum_r2 / (double)n_valid) : 0.f;
  const float rms_c = n_photo > 0 ? (float)sqrt(sum_rc2 / (double)n_photo) : 0.f;
  rec->geo.level = a.log_level; rec->geo.stride = a.stride; rec->geo.n_sampled = n_sampled; rec->geo.n_valid = n_valid;
  rec->geo.sum_r2 = sum_r2; rec->geo.sum_wr2 = total(kAlWr2);
  rec->n_photo = n_photo; rec->pad = 0;
  rec->sum_rc2 = sum_rc2; rec->sum_wrc2 = total(kAlRow + kAlWr2);
  double pose[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) { pose[i] = d.pose_d[i]; rec->geo.pose[i] = pose[i]; }
  if (c.n_eval == 0) { c.n_valid_first = n_valid; c.rms_first = rms; c.n_photo_first = n_photo; c.rms_photo_first = rms_c; }
  c.n_eval += 1;
  if (n_valid < a.min_valid) {
    c.status = TF_ALIGN_TOO_FEW;
    c.state |= 1u;
  } else if (!a.closing) {
    double xi[6];
    if (!align_solve6(M, bb, (double)a.damping, xi)) {
      c.status = TF_ALIGN_SINGULAR;
      c.state |= 1u;
    } else {
      align_update(pose, xi);
#pragma unroll
      for (int i = 0; i < 12; ++i) { d.pose_d[i] = pose[i]; d.pose_f[i] = (float)pose[i]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) rec->geo.xi[i] = xi[i];
      const double nt = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
      const double nr = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
      if (nt < (double)a.eps_t && nr < (double)a.eps_r) {
        c.state = (c.state & 0xFFu) | ((uint32_t)(a.level + 1) << 8);
        if (a.last_level) c.status = TF_ALIGN_CONVERGED;
      }
    }
  }
  *d.ctl = c;
  tf_align_color_result* out = a.out;
  out->geo.status = c.status; out->geo.evaluations = c.n_eval; out->geo.n_sampled = n_sampled;
  out->geo.n_valid_first = c.n_valid_first; out->geo.n_valid_last = n_valid;
  out->geo.rms_first = c.rms_first; out->geo.rms_last = rms;
#pragma unroll
  for (int i = 0; i < 12; ++i) out->geo.pose[i] = (float)pose[i];
  out->n_photo_first = c.n_photo_first; out->n_photo_last = n_photo;
  out->rms_photo_first = c.rms_photo_first; out->rms_photo_last = rms_c;
}

// the state block as it lies in AlignColorState::block (base == null: its size)
CAlignDev calign_carve(void* base, size_t cap_tiles, size_t* bytes) {
  CAlignDev d{};
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
  take(d.part, (size_t)kCaRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = L.size;
  return d;
}

size_t calign_pixels(const tf_volume* v) { const AlignCam c = align_cam(v); return (size_t)c.W * (size_t)c.H; }

// first use, or a larger camera since: the block sized for the camera at stride 1
int calign_ensure(tf_volume* v, CAlignDev* d) {
  const AlignCam c = align_cam(v);
  const size_t tiles = (size_t)((c.W + 7) / 8) * (size_t)((c.H + 7) / 8);
  AlignColorState& s = v->align_color;
  if (!s.block || s.cap_tiles < tiles) {
    size_t bytes = 0;
    calign_carve(nullptr, tiles, &bytes);
    if (s.block) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = s.block.alloc(bytes);
    if (rc) { s.cap_tiles = 0; return rc; }
    TF_HIP(hipMemsetAsync(s.block.p, 0, sizeof(CAlignCtl), v->stream));
    s.cap_tiles = tiles;
  }
  *d = calign_carve(s.block.p, s.cap_tiles, nullptr);
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

CAlignRowsArgs crows_args(const tf_volume* v, const tf_align_color_params& cp, const float* d_depth, const uint8_t* d_rgba,
                          int level, uint32_t* n_tiles) {
  CAlignRowsArgs a{};
  const tf_align_params& p = cp.geo;
  const int s = p.stride[level < p.n_levels ? level : p.n_levels - 1];
  a.depth = d_depth;
  a.rgba = reinterpret_cast<const uint32_t*>(d_rgba);
  const AlignCam c = align_cam(v);
  a.fx = c.fx; a.fy = c.fy; a.cxs = c.cx + 0.5f; a.cys = c.cy + 0.5f;
  a.W = c.W; a.H = c.H; a.stride = s; a.level = level;
  const int nx = (int)(((long long)a.W + s - 1) / s), ny = (int)(((long long)a.H + s - 1) / s);
  a.tiles_x = (nx + 7) / 8;
  *n_tiles = (uint32_t)a.tiles_x * (uint32_t)((ny + 7) / 8);  // <= the tiles at stride 1
  a.min_depth = p.min_depth; a.max_depth = p.max_depth; a.max_residual = p.max_residual; a.huber = p.huber; a.res = v->res;
  a.max_photo_residual = cp.max_photo_residual; a.huber_photo = cp.huber_photo;
  a.plane = (size_t)a.W * a.H;
  return a;
}

// every launch of one alignment: begin, then (rows, solve) per step and once more to close
int calign_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose,
                   const tf_align_color_params& cp, tf_align_color_result* d_result) {
  CAlignDev d;
  int rc = calign_ensure(v, &d);
  if (rc) return rc;
  const tf_align_params& p = cp.geo;
  hipStream_t st = v->stream;
  CAlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  hipLaunchKernelGGL(k_calign_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  for (int l = 0; l <= p.n_levels; ++l) {
    const bool closing = l == p.n_levels;
    uint32_t n_tiles = 0;
    CAlignRowsArgs ra = crows_args(v, cp, d_depth, d_rgba, l, &n_tiles);
    ra.pose = d.pose_f; ra.state = &d.ctl->state; ra.part = d.part;
    CAlignSolveArgs sa{};
    sa.level = l; sa.log_level = closing ? p.n_levels - 1 : l; sa.stride = ra.stride; sa.closing = closing;
    sa.last_level = l == p.n_levels - 1; sa.n_rows = (n_tiles + kAlWaves - 1) / kAlWaves;
    sa.damping = p.damping; sa.eps_t = p.eps_t; sa.eps_r = p.eps_r; sa.min_valid = p.min_valid;
    sa.l2 = (double)cp.photo_weight * (double)cp.photo_weight;
    sa.out = d_result;
    const int n = closing ? 1 : p.iters[l];
    for (int it = 0; it < n; ++it) {
      hipLaunchKernelGGL(k_calign_rows, dim3(sa.n_rows), dim3(kAlWaves * 64), 0, st, v->dev, ra);
      hipLaunchKernelGGL(k_calign_solve, dim3(1), dim3(256), 0, st, d, sa);
    }
  }
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int cresiduals_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose,
                       const tf_align_color_params& cp, float* d_r, float* d_grad3, float* d_rc, float* d_gradc3,
                       uint32_t* d_flags) {
  CAlignDev d;
  int rc = calign_ensure(v, &d);
  if (rc) return rc;
  hipStream_t st = v->stream;
  uint32_t n_tiles = 0;
  CAlignRowsArgs ra = crows_args(v, cp, d_depth, d_rgba, 0, &n_tiles);
  ra.pose = d.pose_r; ra.r = d_r; ra.grad = d_grad3; ra.rc = d_rc; ra.gradc = d_gradc3; ra.flags = d_flags;
  if (ra.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.plane, st));
    if (d_grad3) TF_HIP(hipMemsetAsync(d_grad3, 0, 12 * ra.plane, st));
    if (d_rc) TF_HIP(hipMemsetAsync(d_rc, 0, 4 * ra.plane, st));
    if (d_gradc3) TF_HIP(hipMemsetAsync(d_gradc3, 0, 12 * ra.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.plane, st));
  }
  CAlignPose P;
  memcpy(P.p, pose, sizeof(P.p));
  hipLaunchKernelGGL(k_calign_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  hipLaunchKernelGGL(k_calign_rows, dim3((n_tiles + kAlWaves - 1) / kAlWaves), dim3(kAlWaves * 64), 0, st, v->dev, ra);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

void align_color_release(tf_volume* v) { v->align_color = AlignColorState{}; }

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
  const size_t P = calign_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take(4 * P), o_r = L.take(sizeof(tf_align_color_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgba, 4 * P)))
    return rc;
  if ((rc = calign_enqueue(v, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), pose, *params,
                           sg.dp<tf_align_color_result>(o_r))))
    return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, sizeof(tf_align_color_result), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(result, sg.h + o_r, sizeof(tf_align_color_result));
  return TF_OK;
}

int tf_align_color_log(tf_volume* v, tf_align_color_iter* out, int64_t cap, int64_t* n) {
  if (!v || !n || cap < 0 || (cap > 0 && !out)) { set_error("null argument"); return TF_ERR_INVALID; }
  *n = 0;
  TF_DEV_READER(v);
  if (!v->align_color.block) return TF_OK;
  const CAlignDev d = calign_carve(v->align_color.block.p, v->align_color.cap_tiles, nullptr);
  TF_HIP(hipStreamSynchronize(v->stream));
  CAlignCtl c;
  TF_HIP(hipMemcpy(&c, d.ctl, sizeof(c), hipMemcpyDeviceToHost));
  const int64_t have = c.n_eval < 0 ? 0 : (c.n_eval > TF_ALIGN_MAX_EVALUATIONS ? TF_ALIGN_MAX_EVALUATIONS : c.n_eval);
  *n = have;
  const int64_t m = have < cap ? have : cap;
  if (m > 0) TF_HIP(hipMemcpy(out, d.log, (size_t)m * sizeof(tf_align_color_iter), hipMemcpyDeviceToHost));
  return TF_OK;
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
  const size_t P = calign_pixels(v);
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
  TF_HIP(hipMemcpyAsync(sg.h + o_r, sg.d + o_r, L.size - o_r, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (grad3) memcpy(grad3, sg.h + o_g, 12 * P);
  if (rc_map) memcpy(rc_map, sg.h + o_rc, 4 * P);
  if (gradc3) memcpy(gradc3, sg.h + o_gc, 12 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  return TF_OK;
}

}  // extern "C"
