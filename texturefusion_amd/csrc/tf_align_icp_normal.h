// tf_align_icp_normal.h -- the frame's own normal at a sampled pixel, for the rows kernels that gate the projective ICP by
// it: k_gated_rows and k_frame_normals (tf_align_icp_gate.hip, whose header states the arithmetic) and the gated form of
// k_cicp_rows (tf_align_icp_color.hip).  One text; device functions are forced inline and every operation is rounded on its
// own.  tests/align_icp_gate_ref.py restates it.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "tf_align_rows.h"

#pragma clang fp contract(off)

namespace tf {

// The five depths of a sampled pixel inside the image, loaded as one batch.  Where a neighbour lies outside the image all
// four addresses are the pixel's own (in4 == false: the values are not looked at): selects, not branches, around the loads,
// so that none of them waits for a comparison.
struct FnTaps {
  float z0, zl, zr, zu, zd;
  bool in4;
};
__device__ __forceinline__ FnTaps fn_taps(const AlignRowsCommon& c, const AlPixel& px, const float* __restrict__ depth, size_t o) {
  const long long s = c.stride;
  FnTaps t;
  t.in4 = px.X >= s && px.X + s < c.W && px.Y >= s && px.Y + s < c.H;
  const size_t dx = t.in4 ? (size_t)s : 0, dy = t.in4 ? (size_t)s * (size_t)c.W : 0;  // o -+ dx, o -+ dy: inside [0, W * H)
  t.z0 = depth[o];
  t.zl = depth[o - dx]; t.zr = depth[o + dx];
  t.zu = depth[o - dy]; t.zd = depth[o + dy];
  return t;
}
__device__ __forceinline__ bool fn_in_range(const AlignRowsCommon& c, float z) {  // bit 0's test (al_point)
  return isfinite(z) && z >= c.min_depth && z <= c.max_depth;
}
// the frame normal of a pixel whose own depth is in range (tf_align_icp_gate.hip's header)
struct FrameNormal {
  float x, y, z, l2;
  bool ok;
};
__device__ __forceinline__ FrameNormal frame_normal(const AlignRowsCommon& c, const AlPixel& px, const FnTaps& t, float max_jump) {
  const int X = (int)px.X, Y = (int)px.Y, s = c.stride;
  bool ok = t.in4 && fn_in_range(c, t.zl) && fn_in_range(c, t.zr) && fn_in_range(c, t.zu) && fn_in_range(c, t.zd);
  ok = ok && fabsf(t.zl - t.z0) <= max_jump && fabsf(t.zr - t.z0) <= max_jump && fabsf(t.zu - t.z0) <= max_jump &&
       fabsf(t.zd - t.z0) <= max_jump;
  // (X - s, Y - s: not formed as ints where they could overflow -- in4 is false there and the value is not used)
  const float xl = t.in4 ? (float)(X - s) : 0.f, xr = t.in4 ? (float)(X + s) : 0.f;
  const float yu = t.in4 ? (float)(Y - s) : 0.f, yd = t.in4 ? (float)(Y + s) : 0.f;
  const float dcx = ((float)X - c.cxs) / c.fx, dcy = ((float)Y - c.cys) / c.fy;
  const float dcxl = (xl - c.cxs) / c.fx, dcxr = (xr - c.cxs) / c.fx;
  const float dcyu = (yu - c.cys) / c.fy, dcyd = (yd - c.cys) / c.fy;
  const float ax = dcxr * t.zr - dcxl * t.zl, ay = dcy * t.zr - dcy * t.zl, az = t.zr - t.zl;
  const float bx = dcx * t.zd - dcx * t.zu, by = dcyd * t.zd - dcyu * t.zu, bz = t.zd - t.zu;
  FrameNormal n;
  n.x = by * az - bz * ay; n.y = bz * ax - bx * az; n.z = bx * ay - by * ax;
  n.l2 = (n.x * n.x + n.y * n.y) + n.z * n.z;
  n.ok = ok && isfinite(n.l2) && n.l2 > 0.f;
  return n;
}

// Flag bits 4 and 5 of a pixel whose bits 0 to 3 are fl (tf_align_icp_gate.hip's header): the frame normal n turned into the
// world by the pose P, against the model normal g (the model normal wherever bit 2 is set) with m2 = |g|^2 as the hit test
// formed it, c2 = min_normal_cos squared.
__device__ __forceinline__ uint32_t fn_gate_bits(uint32_t fl, const FrameNormal& n, const float* P, float gx, float gy, float gz,
                                                 float m2, float c2) {
  const float wx = (P[0] * n.x + P[1] * n.y) + P[2] * n.z;
  const float wy = (P[4] * n.x + P[5] * n.y) + P[6] * n.z;
  const float wz = (P[8] * n.x + P[9] * n.y) + P[10] * n.z;
  const float d = (wx * gx + wy * gy) + wz * gz;
  const bool has = fl == 15u && n.ok;
  const bool agree = d > 0.f && d * d >= (c2 * n.l2) * m2;
  return has ? (agree ? 48u : 16u) : 0u;
}

}  // namespace tf
