// tf_ray_devfn.h -- the device functions that every reader of the fused volume shares (tf_ray.hip, tf_align.hip): the
// per-lane chunk cache and the trilinear sampler.  The sampler's arithmetic is defined in tf_ray.hip's header comment and
// restated bit for bit by tests/raycast_ref.py; including files are built with -ffp-contract=off.  Device only.
#pragma once

#include <limits.h>
#include <math.h>

#include "tf_devfn.h"

#pragma clang fp contract(off)

namespace tf {

constexpr float kVoxLimit = 8388607.0f;  // |voxel coordinate| bound: chunk ids stay inside pack_id's 21-bit range
constexpr float kChunkLimit = 1048576.0f;

// per-lane cache of the last chunk lookup
struct ChunkCache {
  int x, y, z;
  uint32_t slot;
};

__device__ __forceinline__ uint32_t lookup_cached(const VolumeDev& v, ChunkCache& cc, int x, int y, int z) {
  if (x != cc.x || y != cc.y || z != cc.z) {
    cc.x = x; cc.y = y; cc.z = z;
    cc.slot = hash_slot_alive(v, pack_id(x, y, z));
  }
  return cc.slot;
}

// floor of a float as an int, false when it is not finite or outside (-lim, lim)
__device__ __forceinline__ bool floor_in(float a, float lim, int* out) {
  const float f = floorf(a);
  if (!(f > -lim && f < lim)) return false;
  *out = (int)f;
  return true;
}

__device__ __forceinline__ float lerpf(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ float tri8(const float c[8], float fx, float fy, float fz) {
  const float e0 = lerpf(c[0], c[1], fx), e1 = lerpf(c[2], c[3], fx), e2 = lerpf(c[4], c[5], fx), e3 = lerpf(c[6], c[7], fx);
  const float g0 = lerpf(e0, e1, fy), g1 = lerpf(e2, e3, fy);
  return lerpf(g0, g1, fz);
}

// Trilinear SDF (and, with rgb != nullptr, colour) at world point p.  Returns the SDF validity; *okc the colour's.
// The corners' chunks: the base corner's through the cache / hash, the others through the base chunk's row of the neighbour
// table (a non-zero word is the neighbour's pool slot for the life of the volume) and the hash where a word
// is 0.  A parked chunk that the table still names holds fresh voxels (weight 0, count 0): invalid, as if absent.
template <bool kRgb>
__device__ __forceinline__ bool tri_sample(const VolumeDev& v, ChunkCache& cc, float px, float py, float pz, float ir,
                                           float* sdf, float* rgb = nullptr, bool* okc = nullptr) {
  if (kRgb) *okc = false;
  const float gx = px * ir - 0.5f, gy = py * ir - 0.5f, gz = pz * ir - 0.5f;
  int ix, iy, iz;
  if (!floor_in(gx, kVoxLimit, &ix) || !floor_in(gy, kVoxLimit, &iy) || !floor_in(gz, kVoxLimit, &iz)) return false;
  const float fx = gx - floorf(gx), fy = gy - floorf(gy), fz = gz - floorf(gz);
  const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3;  // arithmetic shift = floor division
  const int lx = ix & 7, ly = iy & 7, lz = iz & 7;
  const uint32_t base = lookup_cached(v, cc, bx, by, bz);
  if (base == kInvalidSlot) return false;
  const int ox = lx == 7, oy = ly == 7, oz = lz == 7;
  uint32_t slots[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = (k & 1) & ox, dy = ((k >> 1) & 1) & oy, dz = ((k >> 2) & 1) & oz;
    if ((dx | dy | dz) == 0) { slots[k] = base; continue; }
    const uint32_t w = v.nbr[(size_t)base * kNbrWords + (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)];
    slots[k] = w ? w - 1u : hash_slot_alive(v, pack_id(bx + dx, by + dy, bz + dz));
  }
  float c[8];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c[k] = 0.f;
    if (slots[k] == kInvalidSlot) { ok = false; continue; }
    const int vx = (lx + (k & 1)) & 7, vy = (ly + ((k >> 1) & 1)) & 7, vz = (lz + ((k >> 2) & 1)) & 7;
    const float2 sw = v.tsdf[(size_t)slots[k] * kChunkVoxels + (vz * 8 + vy) * 8 + vx];
    if (!(sw.y > 0.f)) ok = false;
    c[k] = sw.x;
  }
  if (ok) *sdf = tri8(c, fx, fy, fz);
  if (!kRgb) return ok;
  ushort4 q[8];  // the corners' colour words (two VGPRs each); the means are formed channel by channel
  bool okk = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    q[k] = make_ushort4(0, 0, 0, 0);
    if (slots[k] == kInvalidSlot) { okk = false; continue; }
    const int vx = (lx + (k & 1)) & 7, vy = (ly + ((k >> 1) & 1)) & 7, vz = (lz + ((k >> 2) & 1)) & 7;
    q[k] = v.color[(size_t)slots[k] * kChunkVoxels + (vz * 8 + vy) * 8 + vx];
    if (q[k].w == 0) okk = false;
  }
  if (okk) {
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = (float)q[k].x / (float)q[k].w;
    rgb[0] = fminf(255.f, floorf(tri8(c, fx, fy, fz) + 0.5f));
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = (float)q[k].y / (float)q[k].w;
    rgb[1] = fminf(255.f, floorf(tri8(c, fx, fy, fz) + 0.5f));
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = (float)q[k].z / (float)q[k].w;
    rgb[2] = fminf(255.f, floorf(tri8(c, fx, fy, fz) + 0.5f));
  }
  *okc = okk;
  return ok;
}

// Trilinear SDF and model intensity at world point p, for the colour-aided aligner (tf_align_color.hip; restated by
// tests/align_color_ref.py).  The eight slots are resolved once, as above; a corner's colour word is loaded beside its SDF
// word (the two addresses differ by the arrays' bases only).  Returns the SDF validity and value exactly as
// tri_sample<false>.  Intensity: per corner l_k = (0.299f * (R / n) + 0.587f * (G / n)) + 0.114f * (B / n) of the u16 word
// (R, G, B, n), *lum = tri8(l, fx, fy, fz) * (1.0f / 255.0f) -- not rounded to a grey level: its differences are gradients.
// *okl: every corner's chunk is present and its n > 0 (the weights do not matter, as for tri_sample<true>'s colour).
__device__ __forceinline__ bool tri_sample_lum(const VolumeDev& v, ChunkCache& cc, float px, float py, float pz, float ir,
                                               float* sdf, float* lum, bool* okl) {
  *okl = false;
  const float gx = px * ir - 0.5f, gy = py * ir - 0.5f, gz = pz * ir - 0.5f;
  int ix, iy, iz;
  if (!floor_in(gx, kVoxLimit, &ix) || !floor_in(gy, kVoxLimit, &iy) || !floor_in(gz, kVoxLimit, &iz)) return false;
  const float fx = gx - floorf(gx), fy = gy - floorf(gy), fz = gz - floorf(gz);
  const int bx = ix >> 3, by = iy >> 3, bz = iz >> 3;
  const int lx = ix & 7, ly = iy & 7, lz = iz & 7;
  const uint32_t base = lookup_cached(v, cc, bx, by, bz);
  if (base == kInvalidSlot) return false;
  const int ox = lx == 7, oy = ly == 7, oz = lz == 7;
  uint32_t slots[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int dx = (k & 1) & ox, dy = ((k >> 1) & 1) & oy, dz = ((k >> 2) & 1) & oz;
    if ((dx | dy | dz) == 0) { slots[k] = base; continue; }
    const uint32_t w = v.nbr[(size_t)base * kNbrWords + (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)];
    slots[k] = w ? w - 1u : hash_slot_alive(v, pack_id(bx + dx, by + dy, bz + dz));
  }
  float2 sw[8];
  ushort4 q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {  // all sixteen loads issued before the first use
    sw[k] = make_float2(0.f, 0.f);
    q[k] = make_ushort4(0, 0, 0, 0);
    if (slots[k] == kInvalidSlot) continue;
    const int vx = (lx + (k & 1)) & 7, vy = (ly + ((k >> 1) & 1)) & 7, vz = (lz + ((k >> 2) & 1)) & 7;
    const size_t at = (size_t)slots[k] * kChunkVoxels + (vz * 8 + vy) * 8 + vx;
    sw[k] = v.tsdf[at];
    q[k] = v.color[at];
  }
  float c[8], l[8];
  bool ok = true, okk = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    c[k] = sw[k].x;
    l[k] = 0.f;
    if (!(sw[k].y > 0.f)) ok = false;  // (an absent corner reads as weight 0, count 0)
    if (q[k].w == 0) { okk = false; continue; }
    const float n = (float)q[k].w;
    l[k] = (0.299f * ((float)q[k].x / n) + 0.587f * ((float)q[k].y / n)) + 0.114f * ((float)q[k].z / n);
  }
  if (ok) *sdf = tri8(c, fx, fy, fz);
  if (okk) *lum = tri8(l, fx, fy, fz) * (1.0f / 255.0f);
  *okl = okk;
  return ok;
}

}  // namespace tf
