// tf_align_icp_color.hip -- the projective ICP held inside a plane: tf_align_icp.hip's point-to-plane row with a photometric
// row from the model beside it, so that a wall, a floor or a table top seen from far off the truncation band (where
// tf_align_frame_color cannot capture) fixes the three degrees of freedom its geometry leaves open.  The method is this
// library's own; tests/align_icp_color_ref.py restates it.
//
//   k_cicp_begin  one lane: the caller's pose (f64 and f32) and the model pose into the state block, the control words cleared
//   k_cicp_lum    once per call, a lane per MODEL pixel: the model intensity L at the pixel's vertex and its depth Z
//   k_cicp_grad   once per call, a lane per model pixel: the image gradients Gu, Gv of L (no LDS in either map kernel)
//   k_cicp_rows   one wave per 8 x 8 tile of sampled pixels, eight waves per workgroup, as k_icp_rows: the geometric and the
//                 photometric row of each pixel and the wave's share of both sets of sums; with map outputs, the maps of
//                 tf_align_icp_color_residuals -- one body, the gated variant (tf_align_icp_set_gate) a template flag of it
//   k_cicp_solve  one workgroup: k_calign_solve's function (al_solve_color, tf_align_rows.h)
//
// All f32, every operation rounded on its own (-ffp-contract=off).
// Model maps, from the call's vertex and normal maps Vm, Nm (f32 planar [3][H][W]) and M = [Rm | tm], per model pixel
// i = (u, v), i = v W + u:
//   hit(i) iff (nm.x^2 + nm.y^2) + nm.z^2 > 0.5 (icp_assoc's test)
//   L[i] = tri_sample_lum's intensity at vm (tf_ray_devfn.h, with ir = 1.0f / res: tf_align_frame_color's definition) where
//   hit(i) and that intensity is valid (all eight corners have a colour count > 0), else -1
//   d = vm - tm;  Z[i] = (M[0][2] * d.x + M[1][2] * d.y) + M[2][2] * d.z  (icp_assoc's product order; formed for every pixel)
//   Gu[i] = (L[u + 1, v] - L[u - 1, v]) * 0.5f where it exists: 1 <= u, u + 1 < W, both neighbours n have L[n] >= 0 and
//   fabsf(Z[n] - Z[i]) <= max_depth_jump; Gv the same along v.  A gradient that does not exist is stored as a quiet NaN
//   (0x7FC00000): the three planes L, Gu, Gv say everything the row needs.
//   usable(i) iff L[i] >= 0 and neither gradient is a NaN
// The intensity is sampled from the volume at the model's vertex, not taken from the raycaster's RGBA map: that one writes
// (0, 0, 0, 255) for a hit without colour, which cannot be told from black, and is rounded to u8.
// Row of a sampled pixel: flag bits 0 to 3 (and 4, 5 with the gate), r, assoc and J are the same call's without colour
// (icp_assoc, tf_align_icp_rows.h; fn_gate_bits, tf_align_icp_normal.h); the pixel is geometrically valid iff those low bits
// are 15 (gate on: 63).  With icp_assoc's (mx, my, mz) = the point in the model camera, uc = (fx * mx) / mz + cxs,
// vc = (fy * my) / mz + cys, uf = floorf(uc + 0.5f), vf = floorf(vc + 0.5f), i the associated model pixel:
//   (r8, g8, b8, a8) = the frame pixel's RGBA8;  Lf = ((0.299f * r8 + 0.587f * g8) + 0.114f * b8) * (1.0f / 255.0f)
//   geometrically valid, a8 != 0 and usable(i)                                                                 (bit 8, 256)
//   du = uc - uf, dv = vc - vf;  rc = (L[i] + (Gu[i] * du + Gv[i] * dv)) - Lf   (first order about the nearest pixel)
//   a = (fx * Gu[i]) / mz, b = (fy * Gv[i]) / mz, c = -((a * mx + b * my) / mz)
//   gc_r = (M[r][0] * a + M[r][1] * b) + M[r][2] * c                            (the image gradient in the world frame)
//   Jc = (gc.x, gc.y, gc.z, q.y gc.z - q.z gc.y, q.z gc.x - q.x gc.z, q.x gc.y - q.y gc.x)
//   wc = 1 if huber_photo == 0 or |rc| <= huber_photo, else huber_photo / |rc|
//   bit 8 and |rc| <= max_photo_residual                                                                       (bit 9, 512)
//   rc and gc are 0 without bit 8; the pixel is photometrically valid iff bit 9 is set.
// Sums and solve are tf_align_color.hip's: al_row_sums twice into a row of 2 * kAlRow doubles, al_store_rows, al_add_rows,
// M = A_g + l2 A_c, b = b_g + l2 b_c with l2 = (double)photo_weight^2, al_decide; TF_ALIGN_TOO_FEW goes by the geometric
// count.  With photo_weight == 0 or on a volume without colour the second term is an exact zero: pose, status and every
// geometric sum are tf_align_frame_icp's bit for bit, gate off or on.
// LDS: the rows kernel's 8 x 64 doubles (4096 B), the solve's 8 x 64; the map kernels none.  No atomics, no counters, no
// polling; every launch of a call is enqueued up front, the map launches once per call ahead of the first rows launch.
//
// With tf_align_set_exposure on, Lf is compensated by a gain and an offset that are estimated with the pose: begin, rows
// and solve of a call are tf_align_exposure.hip's then, the map kernels and this file's state block and log stay the call's.
//
// Not here: the depth pyramid (tf_align_icp_set_pyramid is not read by these calls; a level samples by stride); a
// device-pose form (tf_track_*_device); a tf_relocalise hook; blurred images; a multi-rank form.
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

struct CicpDev {
  AlignCtl* ctl;
  double* pose_d;             // [12] the pose between iterations
  float* pose_f;              // [24] the same rounded, then the model pose: what k_cicp_rows reads
  float* pose_r;              // [24] tf_align_icp_color_residuals' pair (the last alignment's state stays as it is)
  double* part;               // [ceil(cap_tiles / kAlWaves)][kCaRow]: two rows per workgroup of k_cicp_rows
  tf_align_color_iter* log;   // [TF_ALIGN_MAX_EVALUATIONS]
};
struct CicpPoses { float p[12], m[12]; };

// the call's model maps: four planes in the state (or, for L, Gu, Gv of the diagnostic, the caller's)
struct CicpMapArgs {
  const float* vm;
  const float* nm;
  float M[12];
  float ir, max_jump;
  int W, H;
  size_t plane;
  float* L;
  float* Z;
  float* Gu;
  float* Gv;
};

struct CicpSolveArgs {
  AlignSolveCommon c;
  double l2;  // photo_weight squared
  tf_align_color_result* out;
};

__global__ __launch_bounds__(64) void k_cicp_begin(CicpDev d, CicpPoses p, int residuals_only) {
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

// (resources of every kernel here: tests/test_kernel_resources_align_icp_color.py)
__global__ __launch_bounds__(256) void k_cicp_lum(VolumeDev v, CicpMapArgs a) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.plane) return;
  const float nx = a.nm[i], ny = a.nm[a.plane + i], nz = a.nm[2 * a.plane + i];
  const float vx = a.vm[i], vy = a.vm[a.plane + i], vz = a.vm[2 * a.plane + i];
  const bool hit = (nx * nx + ny * ny) + nz * nz > 0.5f;
  const float dx = vx - a.M[3], dy = vy - a.M[7], dz = vz - a.M[11];
  a.Z[i] = (a.M[2] * dx + a.M[6] * dy) + a.M[10] * dz;
  float l = -1.f;
  if (hit) {
    ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
    float sdf = 0.f, lum = 0.f;
    bool okl = false;
    tri_sample_lum(v, cc, vx, vy, vz, a.ir, &sdf, &lum, &okl);
    if (okl) l = lum;
  }
  a.L[i] = l;
}

// one central difference of L: the neighbours at i -+ step, both addresses the pixel's own where they lie outside the image
// (selects around the addresses: the four loads go out together)
__device__ __forceinline__ float cicp_diff(const float* __restrict__ L, const float* __restrict__ Z, size_t i, size_t step,
                                           bool inside, float z, float max_jump) {
  const size_t d = inside ? step : 0;
  const float lm = L[i - d], lp = L[i + d], zm = Z[i - d], zp = Z[i + d];
  const bool ok = inside && lm >= 0.f && lp >= 0.f && fabsf(zm - z) <= max_jump && fabsf(zp - z) <= max_jump;
  return ok ? (lp - lm) * 0.5f : __builtin_nanf("");
}
__global__ __launch_bounds__(256) void k_cicp_grad(CicpMapArgs a) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.plane) return;
  const int u = (int)(i % (size_t)a.W), w = (int)(i / (size_t)a.W);
  const float z = a.Z[i];
  a.Gu[i] = cicp_diff(a.L, a.Z, i, 1, u >= 1 && u + 1 < a.W, z, a.max_jump);
  a.Gv[i] = cicp_diff(a.L, a.Z, i, (size_t)a.W, w >= 1 && w + 1 < a.H, z, a.max_jump);
}

template <bool kGate>
__global__ __launch_bounds__(kAlWaves * 64) void k_cicp_rows(CicpRowsArgs a) {
  const IcpRowsArgs& g = a.icp;
  if (g.state && al_idle(g.state, g.c.level)) return;
  const AlPixel px = al_pixel(g.c);
  uint32_t fl = 0;
  int32_t as = -1;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  float rc = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  AlPoint p{};
  if (px.in) {
    const size_t o = (size_t)px.Y * g.c.W + (size_t)px.X;
    FnTaps t{};
    if (kGate) t = fn_taps(g.c, px, g.depth, o);  // the neighbours' depths with the centre's, as k_gated_rows
    else t.z0 = g.depth[o];
    const uint32_t c8 = a.rgba[o];
    if (al_point(g.c, px, t.z0, g.pose, &p)) {
      IcpPhoto ph;
      ph.L = a.L; ph.Gu = a.Gu; ph.Gv = a.Gv;
      const IcpAssoc m = icp_assoc(g, p, &ph);  // bits 1 to 3 and the nine scattered loads: one batch
      fl = m.fl; as = m.as;
      s = m.s; gx = m.gx; gy = m.gy; gz = m.gz;
      if (kGate) fl |= fn_gate_bits(fl, frame_normal(g.c, px, t, a.max_jump), g.pose, gx, gy, gz, m.m2, a.c2);
      const bool usable = ph.l >= 0.f && ph.gu == ph.gu && ph.gv == ph.gv;
      if (fl == (kGate ? 63u : 15u) && (c8 >> 24) != 0u && usable) {
        fl |= 256u;
        const float lf = al_luma(c8);
        const float du = ph.uc - ph.uf, dv = ph.vc - ph.vf;
        rc = (ph.l + (ph.gu * du + ph.gv * dv)) - lf;
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
  // the geometric row's sums exactly as k_icp_rows / k_gated_rows form them, the photometric row's through the same tree:
  // n_photo takes the place of both counts
  __shared__ double wsum[kAlWaves][kCaRow];
  const bool photo = (fl & 512u) != 0u;
  al_row_sums(wsum, 0, px, gx, gy, gz, p.qx, p.qy, p.qz, s, g.c.huber, (fl & 255u) == (kGate ? 63u : 15u), px.in);
  al_row_sums(wsum, kAlRow, px, cx, cy, cz, p.qx, p.qy, p.qz, rc, a.huber_photo, photo, photo);
  al_store_rows(wsum, g.part + (size_t)blockIdx.x * kCaRow);
}

__global__ __launch_bounds__(256) void k_cicp_solve(CicpDev d, CicpSolveArgs a) {
  al_solve_color(d.ctl, d.log, d.pose_d, d.pose_f, d.part, a.c, a.l2, a.out);
}

// the state block as it lies in AlignIcpColorState::st (base == null: its size)
CicpDev cicp_carve(void* base, size_t cap_tiles, size_t* bytes) {
  CicpDev d{};
  Carver c(base);
  c.take(d.ctl, 1);
  c.take(d.pose_d, 12);
  c.take(d.pose_f, 24);
  c.take(d.pose_r, 24);
  c.take(d.log, TF_ALIGN_MAX_EVALUATIONS);
  c.take(d.part, (size_t)kCaRow * ((cap_tiles + kAlWaves - 1) / kAlWaves));
  if (bytes) *bytes = c.L.size;
  return d;
}
int cicp_dev(tf_volume* v, CicpDev* d) {
  const auto bytes_of = [](size_t tiles) { size_t n = 0; cicp_carve(nullptr, tiles, &n); return n; };
  AlignBlock& s = v->align_icp_color.st;
  const int rc = align_ensure(v, s, bytes_of, sizeof(AlignCtl));
  if (rc) return rc;
  *d = cicp_carve(s.block.p, s.cap_tiles, nullptr);
  return TF_OK;
}

// the ten planes of the state: vertex [3], normal [3] of the form that raycasts itself, then L, Gu, Gv, Z
struct CicpPlanes { float *vm, *nm, *L, *Gu, *Gv, *Z; };
int cicp_planes(tf_volume* v, CicpPlanes* m) {
  const size_t P = align_pixels(v);
  AlignIcpColorState& s = v->align_icp_color;
  if (!s.maps || s.map_pixels < P) {
    if (s.maps) TF_HIP(hipStreamSynchronize(v->stream));
    const int rc = s.maps.alloc(40 * P);
    if (rc) { s.map_pixels = 0; return rc; }
    s.map_pixels = P;
  }
  m->vm = s.maps.as<float>();
  m->nm = s.maps.as<float>(12 * P);
  m->L = s.maps.as<float>(24 * P);
  m->Gu = s.maps.as<float>(28 * P);
  m->Gv = s.maps.as<float>(32 * P);
  m->Z = s.maps.as<float>(36 * P);
  return TF_OK;
}

bool photo_ok(const tf_align_icp_color_params* p) {
  const float f[3] = {p->photo_weight, p->max_photo_residual, p->huber_photo};
  if (!finite_all(f, 3) || p->photo_weight < 0.f || p->max_photo_residual < 0.f || p->huber_photo < 0.f) {
    set_error("align icp color: photo_weight, max_photo_residual, huber_photo must be finite and >= 0");
    return false;
  }
  if (!(p->max_depth_jump > 0.f)) { set_error("align icp color: max_depth_jump must be > 0"); return false; }
  return true;
}

// everything a call is refused for, but the map and result pointers (they differ by form)
int cicp_check(tf_volume* v, const float* depth, const void* rgba, const float* pose, const float* model_pose,
               const tf_align_icp_color_params* p, bool with_iters, bool with_ray) {
  if (!p || !rgba) { set_error("null argument"); return TF_ERR_INVALID; }
  const int rc = align_icp_check(v, depth, pose, model_pose, &p->icp, with_iters, with_ray);
  if (rc) return rc;
  return photo_ok(p) ? TF_OK : TF_ERR_INVALID;
}
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// the two map launches of a call: L and Z, then Gu and Gv (L, Gu, Gv: where they go; Z: the state's plane)
void cicp_maps_enqueue(tf_volume* v, const float* d_vertex, const float* d_normal, const float* model_pose, float max_jump,
                       float* d_L, float* d_Gu, float* d_Gv, float* d_Z) {
  const AlignCam cam = align_cam(v);
  CicpMapArgs a{};
  a.vm = d_vertex; a.nm = d_normal;
  memcpy(a.M, model_pose, sizeof(a.M));
  a.ir = 1.0f / v->res; a.max_jump = max_jump;
  a.W = cam.W; a.H = cam.H;
  a.plane = (size_t)cam.W * cam.H;
  a.L = d_L; a.Z = d_Z; a.Gu = d_Gu; a.Gv = d_Gv;
  const uint32_t blocks = (uint32_t)((a.plane + 255) / 256);
  hipLaunchKernelGGL(k_cicp_lum, dim3(blocks), dim3(256), 0, v->stream, v->dev, a);
  hipLaunchKernelGGL(k_cicp_grad, dim3(blocks), dim3(256), 0, v->stream, a);
}

CicpRowsArgs cicp_rows_args(const tf_volume* v, const AlignRowsCommon& rc, const tf_align_icp_color_params& p,
                            const float* d_depth, const uint8_t* d_rgba, const float* d_vertex, const float* d_normal,
                            const CicpPlanes& m) {
  CicpRowsArgs a{};
  a.icp.c = rc;
  a.icp.depth = d_depth; a.icp.vm = d_vertex; a.icp.nm = d_normal;
  a.icp.max_dist2 = p.icp.max_distance * p.icp.max_distance;
  a.icp.plane = (size_t)rc.W * rc.H;
  a.rgba = reinterpret_cast<const uint32_t*>(d_rgba);
  a.L = m.L; a.Gu = m.Gu; a.Gv = m.Gv;
  a.max_photo_residual = p.max_photo_residual; a.huber_photo = p.huber_photo;
  const tf_align_icp_gate& g = v->align_icp.gate;  // read where icp_gate_on(v)
  a.c2 = g.min_normal_cos * g.min_normal_cos; a.max_jump = g.max_depth_jump;
  return a;
}
void cicp_rows_launch(tf_volume* v, const CicpRowsArgs& a, uint32_t n_rows) {
  if (icp_gate_on(v)) hipLaunchKernelGGL(k_cicp_rows<true>, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, a);
  else hipLaunchKernelGGL(k_cicp_rows<false>, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, a);
}

// every launch of one alignment: begin, the model maps, then (rows, solve) per step and once more to close
int cicp_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose, const float* d_vertex,
                 const float* d_normal, const float* model_pose, const tf_align_icp_color_params& p,
                 tf_align_color_result* d_result) {
  CicpDev d;
  CicpPlanes m;
  int rc = cicp_dev(v, &d);
  if (rc || (rc = cicp_planes(v, &m))) return rc;
  hipStream_t st = v->stream;
  CicpPoses P;
  memcpy(P.p, pose, sizeof(P.p));
  memcpy(P.m, model_pose, sizeof(P.m));
  const double l2 = (double)p.photo_weight * (double)p.photo_weight;
  if (exposure_on(v)) {  // tf_align_set_exposure: begin, rows and solve are tf_align_exposure.hip's, state and log stay this file's
    cicp_maps_enqueue(v, d_vertex, d_normal, model_pose, p.max_depth_jump, m.L, m.Gu, m.Gv, m.Z);
    return exposure_proj_enqueue(v, ExposureOwn{d.ctl, d.pose_d, d.pose_f, d.pose_r, d.log}, P.p, P.m,
                                 cicp_rows_args(v, AlignRowsCommon{}, p, d_depth, d_rgba, d_vertex, d_normal, m), p.icp.geo, l2,
                                 d_result);
  }
  exposure_not_run(v, 1);
  hipLaunchKernelGGL(k_cicp_begin, dim3(1), dim3(64), 0, st, d, P, 0);
  cicp_maps_enqueue(v, d_vertex, d_normal, model_pose, p.max_depth_jump, m.L, m.Gu, m.Gv, m.Z);
  align_walk(v, p.icp.geo, [&](const AlignRowsCommon& c, const AlignSolveCommon& sc) {
    CicpRowsArgs ra = cicp_rows_args(v, c, p, d_depth, d_rgba, d_vertex, d_normal, m);
    ra.icp.pose = d.pose_f; ra.icp.state = &d.ctl->state; ra.icp.part = d.part;
    cicp_rows_launch(v, ra, sc.n_rows);
    hipLaunchKernelGGL(k_cicp_solve, dim3(1), dim3(256), 0, st, d, CicpSolveArgs{sc, l2, d_result});
  });
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int cicp_residuals_enqueue(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float* pose, const float* d_vertex,
                           const float* d_normal, const float* model_pose, const tf_align_icp_color_params& p, float* d_r,
                           float* d_rc, uint32_t* d_flags, int32_t* d_assoc, float* d_gradc3) {
  CicpDev d;
  CicpPlanes m;
  int rc = cicp_dev(v, &d);
  if (rc || (rc = cicp_planes(v, &m))) return rc;
  hipStream_t st = v->stream;
  AlignRowsCommon c;
  AlignSolveCommon sc;
  align_level(v, p.icp.geo, 0, &c, &sc);
  CicpRowsArgs ra = cicp_rows_args(v, c, p, d_depth, d_rgba, d_vertex, d_normal, m);
  ra.icp.pose = d.pose_r; ra.icp.r = d_r; ra.icp.flags = d_flags; ra.icp.assoc = d_assoc; ra.rc = d_rc; ra.gradc = d_gradc3;
  if (c.stride > 1) {  // pixels that are not sampled
    if (d_r) TF_HIP(hipMemsetAsync(d_r, 0, 4 * ra.icp.plane, st));
    if (d_rc) TF_HIP(hipMemsetAsync(d_rc, 0, 4 * ra.icp.plane, st));
    if (d_flags) TF_HIP(hipMemsetAsync(d_flags, 0, 4 * ra.icp.plane, st));
    if (d_assoc) TF_HIP(hipMemsetAsync(d_assoc, 0xFF, 4 * ra.icp.plane, st));  // -1
    if (d_gradc3) TF_HIP(hipMemsetAsync(d_gradc3, 0, 12 * ra.icp.plane, st));
  }
  CicpPoses P;
  memcpy(P.p, pose, sizeof(P.p));
  memcpy(P.m, model_pose, sizeof(P.m));
  if (exposure_on(v)) {
    cicp_maps_enqueue(v, d_vertex, d_normal, model_pose, p.max_depth_jump, m.L, m.Gu, m.Gv, m.Z);
    return exposure_proj_residuals(v, ExposureOwn{d.ctl, d.pose_d, d.pose_f, d.pose_r, d.log}, P.p, P.m, ra, sc.n_rows);
  }
  hipLaunchKernelGGL(k_cicp_begin, dim3(1), dim3(64), 0, st, d, P, 1);
  cicp_maps_enqueue(v, d_vertex, d_normal, model_pose, p.max_depth_jump, m.L, m.Gu, m.Gv, m.Z);
  cicp_rows_launch(v, ra, sc.n_rows);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// the model raycast at model_pose into the state's own maps: tf_raycast_device's launch
int cicp_raycast(tf_volume* v, const float* model_pose, const tf_align_icp_params& p, CicpPlanes* m) {
  const int rc = cicp_planes(v, m);
  if (rc) return rc;
  return tf_raycast_device(v, model_pose, p.ray_near, p.ray_far, p.ray_max_steps, nullptr, m->nm, nullptr, m->vm);
}

// what tf_align_icp_color_model_maps(_device) refuses a call for (there is no frame: the maps are the model's)
int model_maps_check(tf_volume* v, const float* vertex, const float* normal, const float* model_pose,
                     const tf_align_icp_color_params* p) {
  if (!p || !vertex || !normal || !model_pose) { set_error("null argument"); return TF_ERR_INVALID; }
  const int rc = align_icp_check(v, vertex, model_pose, model_pose, &p->icp, false, false);
  if (rc) return rc;
  return photo_ok(p) ? TF_OK : TF_ERR_INVALID;
}

}  // namespace

void align_icp_color_release(tf_volume* v) { v->align_icp_color = AlignIcpColorState{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_icp_color_default_params(tf_align_icp_color_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_align_icp_color_params p{};
  const int rc = tf_align_icp_default_params(&p.icp);
  if (rc) return rc;
  p.photo_weight = 0.1f; p.max_photo_residual = 0.25f; p.huber_photo = 0.05f;  // tf_align_frame_color's
  p.max_depth_jump = 0.1f;                                                      // the gate's jump
  *out = p;
  return TF_OK;
}

int tf_align_frame_icp_color_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                    const float* d_model_vertex, const float* d_model_normal, const float model_pose[12],
                                    const tf_align_icp_color_params* params, tf_align_color_result* d_result) {
  int rc = cicp_check(v, d_depth, d_rgba, pose, model_pose, params, true, false);
  if (rc) return rc;
  if (!d_model_vertex || !d_model_normal || !model_pose || !d_result) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!aligned4(d_rgba)) { set_error("device rgba image must be 4-byte aligned"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  return cicp_enqueue(v, d_depth, d_rgba, pose, d_model_vertex, d_model_normal, model_pose, *params, d_result);
}

int tf_align_frame_icp_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                             const float* model_pose, const tf_align_icp_color_params* params, tf_align_color_result* result) {
  int rc = cicp_check(v, depth, rgba, pose, model_pose, params, true, true);
  if (rc) return rc;
  if (!result) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const float* mp = model_pose ? model_pose : pose;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take(4 * P), o_r = L.take(sizeof(tf_align_color_result));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgba, 4 * P)))
    return rc;
  CicpPlanes m;
  if ((rc = cicp_raycast(v, mp, params->icp, &m))) return rc;
  if ((rc = cicp_enqueue(v, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), pose, m.vm, m.nm, mp, *params,
                         sg.dp<tf_align_color_result>(o_r))))
    return rc;
  return stage_out(v, sg, o_r, sizeof(tf_align_color_result), result);
}

int tf_align_icp_color_log(tf_volume* v, tf_align_color_iter* out, int64_t cap, int64_t* n) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  const AlignBlock& s = v->align_icp_color.st;
  const CicpDev d = s.block ? cicp_carve(s.block.p, s.cap_tiles, nullptr) : CicpDev{};
  return align_log(v, d.ctl, d.log, sizeof(tf_align_color_iter), out, cap, n);
}

int tf_align_icp_color_residuals_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgba, const float pose[12],
                                        const float* d_model_vertex, const float* d_model_normal, const float model_pose[12],
                                        const tf_align_icp_color_params* params, float* d_r, float* d_rc, uint32_t* d_flags,
                                        int32_t* d_assoc, float* d_gradc3) {
  int rc = cicp_check(v, d_depth, d_rgba, pose, model_pose, params, false, false);
  if (rc) return rc;
  if (!d_model_vertex || !d_model_normal || !model_pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!aligned4(d_rgba)) { set_error("device rgba image must be 4-byte aligned"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!d_r && !d_rc && !d_flags && !d_assoc && !d_gradc3) return TF_OK;
  return cicp_residuals_enqueue(v, d_depth, d_rgba, pose, d_model_vertex, d_model_normal, model_pose, *params, d_r, d_rc,
                                d_flags, d_assoc, d_gradc3);
}

int tf_align_icp_color_residuals(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                                 const float* model_vertex, const float* model_normal, const float* model_pose,
                                 const tf_align_icp_color_params* params, float* r, float* rc_map, uint32_t* flags,
                                 int32_t* assoc, float* gradc3) {
  const bool own = !model_vertex && !model_normal;  // no maps given: raycast them
  int rc = cicp_check(v, depth, rgba, pose, model_pose, params, false, own);
  if (rc) return rc;
  if (!own && (!model_vertex || !model_normal)) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!r && !rc_map && !flags && !assoc && !gradc3) return TF_OK;
  const float* mp = model_pose ? model_pose : pose;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take(4 * P), o_v = L.take(own ? 0 : 12 * P), o_n = L.take(own ? 0 : 12 * P);
  const size_t o_r = L.take(r ? 4 * P : 0), o_rc = L.take(rc_map ? 4 * P : 0), o_f = L.take(flags ? 4 * P : 0),
               o_a = L.take(assoc ? 4 * P : 0), o_g = L.take(gradc3 ? 12 * P : 0);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgba, 4 * P)))
    return rc;
  const float *d_v = nullptr, *d_n = nullptr;
  if (own) {
    CicpPlanes m;
    if ((rc = cicp_raycast(v, mp, params->icp, &m))) return rc;
    d_v = m.vm; d_n = m.nm;
  } else {
    if ((rc = stage_in(v, sg, o_v, model_vertex, 12 * P)) || (rc = stage_in(v, sg, o_n, model_normal, 12 * P))) return rc;
    d_v = sg.dp<float>(o_v); d_n = sg.dp<float>(o_n);
  }
  rc = cicp_residuals_enqueue(v, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), pose, d_v, d_n, mp, *params,
                              r ? sg.dp<float>(o_r) : nullptr, rc_map ? sg.dp<float>(o_rc) : nullptr,
                              flags ? sg.dp<uint32_t>(o_f) : nullptr, assoc ? sg.dp<int32_t>(o_a) : nullptr,
                              gradc3 ? sg.dp<float>(o_g) : nullptr);
  if (rc) return rc;
  if ((rc = stage_out(v, sg, o_r, L.size - o_r, nullptr))) return rc;
  if (r) memcpy(r, sg.h + o_r, 4 * P);
  if (rc_map) memcpy(rc_map, sg.h + o_rc, 4 * P);
  if (flags) memcpy(flags, sg.h + o_f, 4 * P);
  if (assoc) memcpy(assoc, sg.h + o_a, 4 * P);
  if (gradc3) memcpy(gradc3, sg.h + o_g, 12 * P);
  return TF_OK;
}

int tf_align_icp_color_model_maps_device(tf_volume* v, const float* d_model_vertex, const float* d_model_normal,
                                         const float model_pose[12], const tf_align_icp_color_params* params, float* d_L,
                                         float* d_Gu, float* d_Gv) {
  int rc = model_maps_check(v, d_model_vertex, d_model_normal, model_pose, params);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (!d_L && !d_Gu && !d_Gv) return TF_OK;
  CicpPlanes m;
  if ((rc = cicp_planes(v, &m))) return rc;
  // into the state's planes, then out: an output that is not wanted needs no buffer of the caller's
  cicp_maps_enqueue(v, d_model_vertex, d_model_normal, model_pose, params->max_depth_jump, m.L, m.Gu, m.Gv, m.Z);
  TF_HIP(hipGetLastError());
  const size_t bytes = 4 * align_pixels(v);
  if (d_L) TF_HIP(hipMemcpyAsync(d_L, m.L, bytes, hipMemcpyDeviceToDevice, v->stream));
  if (d_Gu) TF_HIP(hipMemcpyAsync(d_Gu, m.Gu, bytes, hipMemcpyDeviceToDevice, v->stream));
  if (d_Gv) TF_HIP(hipMemcpyAsync(d_Gv, m.Gv, bytes, hipMemcpyDeviceToDevice, v->stream));
  return TF_OK;
}

int tf_align_icp_color_model_maps(tf_volume* v, const float* model_vertex, const float* model_normal, const float model_pose[12],
                                  const tf_align_icp_color_params* params, float* L_map, float* Gu_map, float* Gv_map) {
  int rc = model_maps_check(v, model_vertex, model_normal, model_pose, params);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (!L_map && !Gu_map && !Gv_map) return TF_OK;
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_v = L.take(12 * P), o_n = L.take(12 * P), o_l = L.take(12 * P);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_v, model_vertex, 12 * P)) ||
      (rc = stage_in(v, sg, o_n, model_normal, 12 * P)))
    return rc;
  CicpPlanes m;
  if ((rc = cicp_planes(v, &m))) return rc;
  float* d_l = sg.dp<float>(o_l);
  cicp_maps_enqueue(v, sg.dp<float>(o_v), sg.dp<float>(o_n), model_pose, params->max_depth_jump, d_l, d_l + P, d_l + 2 * P, m.Z);
  TF_HIP(hipGetLastError());
  if ((rc = stage_out(v, sg, o_l, 12 * P, nullptr))) return rc;
  if (L_map) memcpy(L_map, sg.h + o_l, 4 * P);
  if (Gu_map) memcpy(Gu_map, sg.h + o_l + 4 * P, 4 * P);
  if (Gv_map) memcpy(Gv_map, sg.h + o_l + 8 * P, 4 * P);
  return TF_OK;
}

int tf_track_frame_color(tf_volume* v, const float* depth, const uint8_t* rgba, const float pose[12],
                         const tf_align_icp_color_params* icp_params, const tf_align_color_params* sdf_params,
                         tf_track_color_result* out) {
  int rc = cicp_check(v, depth, rgba, pose, nullptr, icp_params, true, true);
  if (rc) return rc;
  if (!sdf_params || !out) { set_error("null argument"); return TF_ERR_INVALID; }
  if ((rc = align_check(v, depth, pose, &sdf_params->geo, true))) return rc;
  const float f[3] = {sdf_params->photo_weight, sdf_params->max_photo_residual, sdf_params->huber_photo};
  if (!finite_all(f, 3) || f[0] < 0.f || f[1] < 0.f || f[2] < 0.f) {
    set_error("align: photo_weight, max_photo_residual, huber_photo must be finite and >= 0");
    return TF_ERR_INVALID;
  }
  tf_track_color_result t{};
  t.sdf.geo.status = -1;  // not run
  memcpy(t.pose, pose, sizeof(t.pose));
  // (tf_align_set_exposure: the second stage starts at the first stage's estimate, whatever carry says)
  exposure_track_stage(v, 1);
  rc = tf_align_frame_icp_color(v, depth, rgba, pose, nullptr, icp_params, &t.icp);
  exposure_track_stage(v, 0);
  if (rc) return rc;
  if (t.icp.geo.status <= TF_ALIGN_MAX_ITERS) {
    t.stage = 1;
    memcpy(t.pose, t.icp.geo.pose, sizeof(t.pose));
    rc = tf_align_frame_color(v, depth, rgba, t.icp.geo.pose, sdf_params, &t.sdf);
    const int rx = exposure_track_stage(v, 2);
    if (rc || (rc = rx)) return rc;
    if (t.sdf.geo.status <= TF_ALIGN_MAX_ITERS) {
      t.stage = 2;
      memcpy(t.pose, t.sdf.geo.pose, sizeof(t.pose));
    }
  }
  *out = t;
  return TF_OK;
}

}  // extern "C"
