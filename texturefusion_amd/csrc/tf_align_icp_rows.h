// tf_align_icp_rows.h -- what the rows kernels of the projective ICP share: k_icp_rows (tf_align_icp.hip), the gated
// kernel k_gated_rows (tf_align_icp_gate.hip) and the colour ICP's k_cicp_rows (tf_align_icp_color.hip).  The argument block of a rows launch, the association of a pixel's point
// with the model maps (flag bits 1 to 3: one text for both kernels), and the host functions by which tf_align_icp.hip hands
// a launch to the gated file.  Device functions are forced inline and every operation is rounded on its own.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

#include "tf_align_rows.h"

#pragma clang fp contract(off)

struct tf_volume;

namespace tf {

struct IcpRowsArgs {
  AlignRowsCommon c;
  const float* depth;
  const float* vm;        // model vertex map, planar
  const float* nm;        // model normal map, planar
  const float* pose;      // 24 floats in the state block: the frame's pose, the model's
  const uint32_t* state;  // null: always run (tf_align_icp_residuals)
  float max_dist2;
  size_t plane;
  float* r;
  uint32_t* flags;
  int32_t* assoc;
  double* part;  // null: no sums
};

// The argument block of the colour ICP's rows launch (k_cicp_rows, and k_ealign_proj_rows of tf_align_exposure.hip)
struct CicpRowsArgs {
  IcpRowsArgs icp;
  const uint32_t* rgba;  // RGBA8, one word per pixel (r in the low byte)
  const float* L;
  const float* Gu;
  const float* Gv;
  float max_photo_residual, huber_photo;
  float c2, max_jump;    // the gate's (read by the gated variant only)
  float* rc;
  float* gradc;
};

// Bits 1 to 3 of a pixel whose depth is in range (bit 0; p is its point, tf_align_icp.hip's header has the arithmetic):
// fl with bit 0 and whichever of bits 1 to 3 hold, the associated model pixel (-1 without bit 1), the residual s and the
// model normal g (0 without bit 2), m2 = |nm|^2 as the hit test formed it (0 without bit 1).
struct IcpAssoc {
  uint32_t fl;
  int32_t as;
  float s, gx, gy, gz, m2;
};
// What the colour ICP's photometric row takes from the association (tf_align_icp_color.hip's header): in, the three planes
// of the call's model maps; out, where bit 1 is set, the point in the model camera, its projection (uc, vc), the nearest
// pixel (uf, vf) and that pixel's three map values, loaded with the six of the geometric row.  Without bit 1: zeros, l = -1.
struct IcpPhoto {
  const float* L;
  const float* Gu;
  const float* Gv;
  float mx, my, mz, uc, vc, uf, vf, l, gu, gv;
};
__device__ __forceinline__ IcpAssoc icp_assoc(const IcpRowsArgs& a, const AlPoint& p, IcpPhoto* ph = nullptr) {
  IcpAssoc r{1u, -1, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (ph) { ph->mx = ph->my = ph->mz = ph->uc = ph->vc = ph->uf = ph->vf = ph->gu = ph->gv = 0.f; ph->l = -1.f; }
  const float* M = a.pose + 12;
  const float dx = p.wx - M[3], dy = p.wy - M[7], dz = p.wz - M[11];
  const float mx = (M[0] * dx + M[4] * dy) + M[8] * dz;
  const float my = (M[1] * dx + M[5] * dy) + M[9] * dz;
  const float mz = (M[2] * dx + M[6] * dy) + M[10] * dz;
  if (mz > a.c.min_depth) {
    const float uc = (a.c.fx * mx) / mz + a.c.cxs, vc = (a.c.fy * my) / mz + a.c.cys;
    const float uf = floorf(uc + 0.5f), vf = floorf(vc + 0.5f);
    // (compared as floats: a NaN or an infinity of a point near the model camera's plane fails here, ahead of the cast)
    if (uf >= 0.f && uf < (float)a.c.W && vf >= 0.f && vf < (float)a.c.H) {
      r.fl |= 2u;
      const size_t i = (size_t)(int)vf * (size_t)a.c.W + (size_t)(int)uf;  // < W * H
      r.as = (int32_t)i;
      // the six scattered loads of the pixel, all issued ahead of the first use: one batch in flight
      const float nx = a.nm[i], ny = a.nm[a.plane + i], nz = a.nm[2 * a.plane + i];
      const float vx = a.vm[i], vy = a.vm[a.plane + i], vz = a.vm[2 * a.plane + i];
      if (ph) {  // (a constant after inlining) the photometric row's three, in the same batch
        ph->l = ph->L[i]; ph->gu = ph->Gu[i]; ph->gv = ph->Gv[i];
        ph->mx = mx; ph->my = my; ph->mz = mz; ph->uc = uc; ph->vc = vc; ph->uf = uf; ph->vf = vf;
      }
      // (selects, not a branch on the normal: a branch would let the compiler hold the vertex loads back behind it)
      r.m2 = (nx * nx + ny * ny) + nz * nz;
      const bool hit = r.m2 > 0.5f;
      const float ex = p.wx - vx, ey = p.wy - vy, ez = p.wz - vz;
      const float rr = (nx * ex + ny * ey) + nz * ez;
      const bool near = (ex * ex + ey * ey) + ez * ez <= a.max_dist2 && fabsf(rr) <= a.c.max_residual;
      r.s = hit ? rr : 0.f;
      r.gx = hit ? nx : 0.f; r.gy = hit ? ny : 0.f; r.gz = hit ? nz : 0.f;
      r.fl |= hit ? (near ? 12u : 4u) : 0u;
    }
  }
  return r;
}

// tf_align_icp_gate.hip.  gated_rows_launch: k_icp_rows' launch with the handle's gate (which is on), on the handle's
// stream.  icp_gate_on: the handle's setting.
bool icp_gate_on(const tf_volume* v);
void gated_rows_launch(tf_volume* v, const IcpRowsArgs& a, uint32_t n_rows);

}  // namespace tf
