// tf_draw_body.h -- Chisel::DrawMeshes (Structure/Chisel.cpp:288-355) for one complete() patch: interleaved vertex stream +
// rebased indices.  One text for k_draw (tf_atlas.hip: the table comes from the host) and k_model_write (tf_model.hip: the
// table is built on the device), so both write the same bits.  Every output element is written once, 48 B per vertex.
#pragma once

#include "tf_device.h"

#pragma clang fp contract(off)

namespace tf {

struct DrawPatch {
  uint32_t slot, nv, nt, flags;  // flags: bit1 wrong_mapping, bit2 labs valid
  unsigned long long vout, iout;  // output positions (running counts over the patches before this one)
};
// DrawPatch::flags of a patch with these Patch flags: labs valid = has_adjusted && !labs.empty()
__host__ __device__ __forceinline__ uint32_t draw_flags(const uint32_t pflags) {
  const bool labs_valid = (pflags & kPfAdjusted) && !(pflags & kPfWrong);
  return 1u | ((pflags & kPfWrong) ? 2u : 0u) | (labs_valid ? 4u : 0u);
}
// Patch::complete (Patch.cpp:191-196) of a mesh that has a patch
__host__ __device__ __forceinline__ bool draw_complete(uint32_t nv, uint32_t state, uint32_t pflags, int32_t frameid) {
  return nv > 0 && (state & kMsSimplified) && (pflags & kPfHasImage) && frameid >= 0;
}
// one 9-bit field of the colour delta.  A delta that is not a number (labs of a one-vertex cluster: 0 / (N - 1) = 0 / 0)
// packs as a zero delta, 255: stated here, as in the oracle, not left to what the hardware conversion makes of a NaN
__device__ __forceinline__ int pack_delta(const float a) { return a != a ? 255 : (int)(a * 255.0f) + 255; }

// the workgroup's 256 lanes stride over the patch's triangles, then over its vertices
__device__ __forceinline__ void draw_patch_body(const VolumeDev& v, const DrawPatch& P, float* __restrict__ out_v,
                                                uint32_t* __restrict__ out_i) {
  const MeshRec rec = v.mesh_rec[P.slot];
  const float ox = (float)(rec.texloc % (unsigned long long)v.atlas_w);  // Atlas::GetTexLoc (Atlas.cpp:66-69)
  const float oy = (float)(rec.texloc / (unsigned long long)v.atlas_w);
  const float rx = rec.ratio[0], ry = rec.ratio[1];
  const float aw = (float)v.atlas_w, ah = (float)v.atlas_h;
  for (uint32_t j = threadIdx.x; j < P.nt; j += 256)
#pragma unroll
    for (int a = 0; a < 3; ++a) out_i[P.iout + 3 * (size_t)j + a] = (uint32_t)tri_plane(v, rec.block, a)[j] + (uint32_t)P.vout;
  for (uint32_t k = threadIdx.x; k < P.nv; k += 256) {
    float* o = out_v + 12 * (P.vout + k);
    float tx = mesh_plane(v, rec.block, kMpTc)[k], ty = mesh_plane(v, rec.block, kMpTc + 1)[k];
    if (rx < 1.0f) tx = tx * rx;
    if (ry < 1.0f) ty = ty * ry;
    tx = tx + ox;
    ty = ty + oy;
    const float c0 = mesh_plane(v, rec.block, kMpCol)[k], c1 = mesh_plane(v, rec.block, kMpCol + 1)[k],
                c2 = mesh_plane(v, rec.block, kMpCol + 2)[k];
    int rgb = (int)(c0 * 255.0f);
    rgb = (rgb << 8) + (int)(c1 * 255.0f);
    rgb = (rgb << 8) + (int)(c2 * 255.0f);
    float adj = 0.0f;
    if (P.flags & 4u) {
      const float a0 = mesh_plane(v, rec.block, kMpLabs)[k] - mesh_plane(v, rec.block, kMpTcol)[k],
                  a1 = mesh_plane(v, rec.block, kMpLabs + 1)[k] - mesh_plane(v, rec.block, kMpTcol + 1)[k],
                  a2 = mesh_plane(v, rec.block, kMpLabs + 2)[k] - mesh_plane(v, rec.block, kMpTcol + 2)[k];
      int ad = pack_delta(a0);
      ad = (ad << 9) + pack_delta(a1);
      ad = (ad << 9) + pack_delta(a2);
      adj = (float)ad;
    }
    const float4 q0 = make_float4(mesh_plane(v, rec.block, kMpPos)[k], mesh_plane(v, rec.block, kMpPos + 1)[k],
                                  mesh_plane(v, rec.block, kMpPos + 2)[k], 50.0f);
    const float4 q1 = make_float4((float)rgb, adj, tx / aw, ty / ah);
    const float4 q2 = make_float4(mesh_plane(v, rec.block, kMpNrm)[k], mesh_plane(v, rec.block, kMpNrm + 1)[k],
                                  mesh_plane(v, rec.block, kMpNrm + 2)[k], (P.flags & 2u) ? 1.0f : 0.0f);
    reinterpret_cast<float4*>(o)[0] = q0;
    reinterpret_cast<float4*>(o)[1] = q1;
    reinterpret_cast<float4*>(o)[2] = q2;
  }
}

}  // namespace tf
