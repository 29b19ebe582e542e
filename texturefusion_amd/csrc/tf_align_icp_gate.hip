// tf_align_icp_gate.hip -- the third rejection test of KinectFusion's projective association: a pair is kept only where the
// frame's own normal at the pixel and the model's normal at the associated pixel agree.  A setting of the handle
// (tf_align_icp_set_gate), off by default; with it on, every call that runs the projective ICP launches k_gated_rows
// below in place of k_icp_rows (tf_align_icp.hip: icp_enqueue, icp_residuals_enqueue).  tests/align_icp_gate_ref.py
// restates this file.
//
//   k_gated_rows     k_icp_rows' launch (one wave per 8 x 8 tile of sampled pixels, eight waves per workgroup, the same sums
//                    by the same functions) with flag bits 4 and 5; the frame normal is formed here, every evaluation, from
//                    four more depth loads that go out with the centre's -- no normal map, no pass per level
//   k_frame_normals  the frame normals alone as a map (tf_align_icp_frame_normals): the same function of the same taps
//
// A sampled pixel (x, y) at stride s with depth z0 in range (bit 0) has the neighbours L = (x - s, y), R = (x + s, y),
// U = (x, y - s), D = (x, y + s).  All f32, every operation rounded on its own (-ffp-contract=off), in this order:
//   the frame normal exists iff all four neighbours lie inside the image, each depth z_n passes bit 0's test (finite,
//   min_depth <= z_n <= max_depth) and fabsf(z_n - z0) <= max_depth_jump, and with
//     dcx_n = ((float)x_n - cxs) / fx, dcy_n = ((float)y_n - cys) / fy          (al_point's text)
//     pc(n) = (dcx_n * z_n, dcy_n * z_n, z_n);  a = pc(R) - pc(L);  b = pc(D) - pc(U)
//     n = b x a = (b.y a.z - b.z a.y, b.z a.x - b.x a.z, b.x a.y - b.y a.x)     (towards the camera: (0, 0, -) on a
//     fronto-parallel plane, as the raycaster's gradient of the SDF on a surface seen from its front)
//     l2 = (n.x^2 + n.y^2) + n.z^2 is finite and > 0                                                            (bit 4)
//   nw_r = (P[r][0] * n.x + P[r][1] * n.y) + P[r][2] * n.z;  d = (nw.x * nm.x + nw.y * nm.y) + nw.z * nm.z
//   m2 = (nm.x^2 + nm.y^2) + nm.z^2, the hit test's value;  c2 = min_normal_cos * min_normal_cos, formed on the host
//   d > 0 and d * d >= (c2 * l2) * m2: no square root, no division                                              (bit 5)
//   bit 4 only where bits 0 to 3 are set, bit 5 only where bit 4 is; the pixel is valid iff flags == 63.
// r, assoc, J (with the model normal), the Huber weight, the sums and the solve are k_icp_rows'.  The frame normal and the
// two bits are functions of tf_align_icp_normal.h (FnTaps, fn_taps, fn_in_range, frame_normal, fn_gate_bits), which the
// colour ICP's gated rows kernel includes too.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_icp_normal.h"
#include "tf_align_icp_rows.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

// (resources: tests/test_kernel_resources_align_icp_gate.py -- k_icp_rows' budget)
__global__ __launch_bounds__(kAlWaves * 64) void k_gated_rows(IcpRowsArgs a, float c2, float max_jump) {
  if (a.state && al_idle(a.state, a.c.level)) return;
  const AlPixel px = al_pixel(a.c);
  uint32_t fl = 0;
  int32_t as = -1;
  float s = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  AlPoint p{};
  if (px.in) {
    const size_t o = (size_t)px.Y * a.c.W + (size_t)px.X;
    const FnTaps t = fn_taps(a.c, px, a.depth, o);  // the neighbours' depths with the centre's, ahead of the first use
    if (al_point(a.c, px, t.z0, a.pose, &p)) {
      const IcpAssoc m = icp_assoc(a, p);  // bits 1 to 3: k_icp_rows' text
      fl = m.fl; as = m.as;
      s = m.s; gx = m.gx; gy = m.gy; gz = m.gz;
      const FrameNormal n = frame_normal(a.c, px, t, max_jump);
      fl |= fn_gate_bits(fl, n, a.pose, gx, gy, gz, m.m2, c2);  // (g is the model normal wherever bit 2 is set)
    }
    if (a.r) a.r[o] = s;
    if (a.flags) a.flags[o] = fl;
    if (a.assoc) a.assoc[o] = as;
  }
  if (!a.part) return;
  __shared__ double wsum[kAlWaves][kAlRow];
  al_row_sums(wsum, 0, px, gx, gy, gz, p.qx, p.qy, p.qz, s, a.c.huber, fl == 63u, px.in);
  al_store_rows(wsum, a.part + (size_t)blockIdx.x * kAlRow);
}

// the rows launch's geometry without its sums: a lane per sampled pixel
__global__ __launch_bounds__(kAlWaves * 64) void k_frame_normals(AlignRowsCommon c, const float* __restrict__ depth, float max_jump,
                                                                 size_t plane, float* __restrict__ out) {
  const AlPixel px = al_pixel(c);
  if (!px.in) return;
  const size_t o = (size_t)px.Y * c.W + (size_t)px.X;
  const FnTaps t = fn_taps(c, px, depth, o);
  const FrameNormal n = frame_normal(c, px, t, max_jump);
  const bool ok = fn_in_range(c, t.z0) && n.ok;
  out[o] = ok ? n.x : 0.f;
  out[plane + o] = ok ? n.y : 0.f;
  out[2 * plane + o] = ok ? n.z : 0.f;
}

bool gate_ok(const tf_align_icp_gate* g) {
  if (!(g->min_normal_cos >= 0.f && g->min_normal_cos <= 1.f)) {
    set_error("align icp gate: min_normal_cos must be in [0, 1]");
    return false;
  }
  if (!(g->max_depth_jump > 0.f)) { set_error("align icp gate: max_depth_jump must be > 0"); return false; }
  return true;
}

// what tf_align_icp_frame_normals(_device) refuses a call for (there is no pose to check: the map is in the camera frame)
int normals_check(tf_volume* v, const float* depth, const tf_align_icp_params* p, const tf_align_icp_gate* g, const float* normal3) {
  if (!p || !g || !normal3) { set_error("null argument"); return TF_ERR_INVALID; }
  const float eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const int rc = align_check(v, depth, eye, &p->geo, false);
  if (rc) return rc;
  return gate_ok(g) ? TF_OK : TF_ERR_INVALID;
}

int normals_enqueue(tf_volume* v, const float* d_depth, const tf_align_icp_params& p, const tf_align_icp_gate& g, float* d_normal3) {
  AlignRowsCommon c;
  AlignSolveCommon sc;
  align_level(v, p.geo, 0, &c, &sc);
  const size_t plane = (size_t)c.W * c.H;
  if (c.stride > 1) TF_HIP(hipMemsetAsync(d_normal3, 0, 12 * plane, v->stream));  // pixels that are not sampled
  hipLaunchKernelGGL(k_frame_normals, dim3(sc.n_rows), dim3(kAlWaves * 64), 0, v->stream, c, d_depth, g.max_depth_jump, plane,
                     d_normal3);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

bool icp_gate_on(const tf_volume* v) { return v->align_icp.gate_on; }

void gated_rows_launch(tf_volume* v, const IcpRowsArgs& a, uint32_t n_rows) {
  const tf_align_icp_gate& g = v->align_icp.gate;
  const float c2 = g.min_normal_cos * g.min_normal_cos;
  hipLaunchKernelGGL(k_gated_rows, dim3(n_rows), dim3(kAlWaves * 64), 0, v->stream, a, c2, g.max_depth_jump);
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_icp_gate_default(tf_align_icp_gate* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  out->min_normal_cos = 0.9396926f;  // cosf(20 degrees): KinectFusion's
  out->max_depth_jump = 0.1f;
  return TF_OK;
}

int tf_align_icp_set_gate(tf_volume* v, const tf_align_icp_gate* gate) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  if (gate && !gate_ok(gate)) return TF_ERR_INVALID;
  v->align_icp.gate_on = gate != nullptr;
  v->align_icp.gate = gate ? *gate : tf_align_icp_gate{};
  return TF_OK;
}

int tf_align_icp_get_gate(tf_volume* v, tf_align_icp_gate* out, int32_t* on) {
  if (!v || !out || !on) { set_error("null argument"); return TF_ERR_INVALID; }
  *on = v->align_icp.gate_on ? 1 : 0;
  if (v->align_icp.gate_on) *out = v->align_icp.gate;
  else tf_align_icp_gate_default(out);
  return TF_OK;
}

int tf_align_icp_frame_normals_device(tf_volume* v, const float* d_depth, const tf_align_icp_params* params,
                                      const tf_align_icp_gate* gate, float* d_normal3) {
  const int rc = normals_check(v, d_depth, params, gate, d_normal3);
  if (rc) return rc;
  TF_DEV_READER(v);
  return normals_enqueue(v, d_depth, *params, *gate, d_normal3);
}

int tf_align_icp_frame_normals(tf_volume* v, const float* depth, const tf_align_icp_params* params, const tf_align_icp_gate* gate,
                               float* normal3) {
  int rc = normals_check(v, depth, params, gate, normal3);
  if (rc) return rc;
  TF_DEV_READER(v);
  const size_t P = align_pixels(v);
  Layout L;
  const size_t o_d = L.take(4 * P), o_n = L.take(12 * P);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  if ((rc = normals_enqueue(v, sg.dp<const float>(o_d), *params, *gate, sg.dp<float>(o_n)))) return rc;
  return stage_out(v, sg, o_n, 12 * P, normal3);
}

}  // extern "C"
