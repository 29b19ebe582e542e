// tf_ray.hip -- reading the fused volume back: batched point queries and a device raycaster.
//
//   k_query    one lane per world point: ChunkManager::GetSDF / GetWeight (Structure/ChunkManager.cpp:1151-1185),
//              GetSDFAndGradient (:1043-1141, the live #else branch), and a trilinear SDF / colour sampler
//   k_raycast  one lane per pixel, an 8 x 8 pixel tile per wave64: depth / normal / colour / vertex maps of the model
//              from a pose (chunk DDA over absent chunks, voxel steps where the sampler is invalid, sdf-sized steps where
//              it is valid, linear refinement at the first + -> - crossing)
//
//   k_surface_dist  one lane per world point: Chisel::GetDistanceFromSurface (Structure/Chisel.h:251-342)
//   k_refine_frame  one lane per pixel, an 8 x 8 pixel tile per wave64: Chisel::RefineFrameInVoxel (:377-451)
//
// All four kernels only READ the volume (tsdf, color, hent, nbr): no voxel, hash entry, dirty mark, summary, neighbour
// word or statistic is written.  A chunk that is not alive counts as absent, as in tf_has_chunk.
//
// Trilinear sampler (bits 3 / 4 of k_query, every sample of k_raycast) -- the reference's own form is under #if 0, so its
// arithmetic is defined here, once:
//   g = p * (1 / res) - 0.5 per axis (voxel-centre coordinates), i = floor(g), f = g - i (all f32);
//   corner k = dx + 2 dy + 4 dz is voxel (i.x + dx, i.y + dy, i.z + dz);
//   lerp(a, b, t) = a + t * (b - a) (three roundings);
//   e0 = lerp(c0, c1, fx), e1 = lerp(c2, c3, fx), e2 = lerp(c4, c5, fx), e3 = lerp(c6, c7, fx);
//   g0 = lerp(e0, e1, fy), g1 = lerp(e2, e3, fy);  result = lerp(g0, g1, fz).
//   SDF: valid iff all 8 corners exist with weight > 0.  Colour: per corner the mean R / count, G / count, B / count (f32
//   divisions, ColorVoxel.h:44-55), the same lerps, then u8 = min(255, floor(x + 0.5)); valid iff all 8 counts > 0.
// The library is built with -ffp-contract=off, so tests/raycast_ref.py restates all of this bit for bit in numpy: k_query in
// RefVolume.query, and raycast_body's four maps -- the march, vertex = o + thit * d, the normal's six taps with sp - sm /
// 2 sp / -2 sm per axis, the colour at the hit -- in RefVolume.raycast_maps (tests/test_gpu_ray_edges.py holds the kernel to
// it on hand-built volumes, tests/test_gpu_raycast.py on integrated scenes).
//
// GetDistanceFromSurface, in this order, all f32 (tests/refine_ref.py restates it):
//   r = (p - res / 2) * (1 / res) per axis (the reciprocal rounded first); d = r - floor(r);
//   corner k = 0..7 takes ceil(r) on x where bit 2 is set, on y where bit 1 is, on z where bit 0 is, else floor(r)
//   (an integral r repeats the corner: ceil == floor); its weight sw = (a_x * a_y) * a_z with a = d (ceil) or 1 - d;
//   a corner coordinate that is not finite or beyond +-(2^23 - 1) is absent (the reference's float -> int is undefined
//   there); chunk = V >> 3 (= floor((float)V / 8), exact), voxel = (V & 7) as x + 8 y + 64 z;
//   over k in order, corners whose chunk is alive only: weight += sw * w; distance += (sdf * sw) * w; tw += w * sw;
//   if weight > 0: distance /= weight, tw /= weight (else both stay as accumulated).
// RefineFrameInVoxel per pixel (i, j): skipped, depth and weight untouched, if (double)depth < 0.05 or > 3;
//   dir = ((j - cx) / fx, (i - cy) / fy, 1) with the int-truncated intrinsics as float; R * dir per row as
//   a0 b0 + (a1 b1 + a2 b2) -- the reading of Eigen's fixed-size product the integrator kernels use;
//   six times: vertex = (R dir) * depth + t, d = GetDistanceFromSurface(vertex), depth += d; weight = the sixth tw;
//   then depth = weight = 0 where |d| > 5e-3 (double), where depth > far or < near (f32), where |depth - depth_init|
//   > 0.1 (f32 difference, double compare), in that order on the value written so far.
#include <math.h>
#include <limits.h>
#include <string.h>

#include "tf_devfn.h"
#include "tf_devpose.h"
#include "tf_ray_devfn.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {

constexpr float kRayStepK = 0.75f;       // k of the step rule max(voxel, k * sdf)
constexpr float kRayGap = 4.0f;          // voxels an invalid stretch may span between the two samples of a crossing
constexpr int kRayMaxSide = 32768;       // tf_raycast_camera: largest width / height (the tile grid stays in 32 bits)
// (the chunk cache and the trilinear sampler: tf_ray_devfn.h, shared with tf_align.hip)

struct QueryArgs {
  const float* xyz;
  uint32_t n;
  uint32_t want;
  float res;
  float* sdf;
  float* weight;
  float* grad;
  float* sdf_tri;
  uint8_t* rgb;
  uint32_t* flags;
};

// ChunkManager::GetSDF / GetWeight: the chunk GetIDAt names, the voxel Chunk::GetVoxelCoords names (relative to the chunk's
// origin), accepted iff its linear id is in [0, 512) -- as the reference checks it
__device__ __forceinline__ bool point_voxel(const VolumeDev& v, ChunkCache& cc, float px, float py, float pz, float res,
                                            uint32_t* slot, int* id) {
  const float rc = 1.0f / (8.0f * res), ir = 1.0f / res;
  int cx, cy, cz;
  if (!floor_in(px * rc, kChunkLimit, &cx) || !floor_in(py * rc, kChunkLimit, &cy) || !floor_in(pz * rc, kChunkLimit, &cz))
    return false;
  *slot = lookup_cached(v, cc, cx, cy, cz);
  if (*slot == kInvalidSlot) return false;
  int vx, vy, vz;
  if (!floor_in((px - (float)(8 * cx) * res) * ir, kChunkLimit, &vx) ||
      !floor_in((py - (float)(8 * cy) * res) * ir, kChunkLimit, &vy) ||
      !floor_in((pz - (float)(8 * cz) * res) * ir, kChunkLimit, &vz))
    return false;
  const long long i = ((long long)vz * 8 + vy) * 8 + vx;
  if (i < 0 || i >= kChunkVoxels) return false;
  *id = (int)i;
  return true;
}

// one face neighbour: the voxel at (wrapped) local index (nx, ny, nz), in the adjacent chunk (cid + e) when the centre
// voxel lies on that face (cross), else in the centre chunk
__device__ __forceinline__ bool face_sdf(const VolumeDev& v, uint32_t centre, bool cross, int cx, int cy, int cz, int nx,
                                         int ny, int nz, float* d) {
  uint32_t slot = centre;
  if (cross) {
    slot = hash_slot_alive(v, pack_id(cx, cy, cz));
    if (slot == kInvalidSlot) return false;
  }
  *d = v.tsdf[(size_t)slot * kChunkVoxels + (nz * 8 + ny) * 8 + nx].x;
  return *d < 1.f;
}

// ChunkManager::GetSDFAndGradient (live branch): snap to the voxel centre, ids by the reference's f32 arithmetic, the six
// face neighbours (across a chunk face: the adjacent chunk at the wrapped index, voxelNeighborIndex), each must be < 1
// (GetNeighborSDF, ChunkManager.h:755-788)
__device__ __forceinline__ bool point_gradient(const VolumeDev& v, ChunkCache& cc, float px, float py, float pz, float res,
                                               float* gx, float* gy, float* gz) {
  const float half = res / 2.0f, ir = 1.0f / res, rc = 1.0f / (res * 8.0f);
  const float qx = floorf(px / res) * res + half, qy = floorf(py / res) * res + half, qz = floorf(pz / res) * res + half;
  int vgx, vgy, vgz, cx, cy, cz;
  if (!floor_in(qx * ir, kVoxLimit, &vgx) || !floor_in(qy * ir, kVoxLimit, &vgy) || !floor_in(qz * ir, kVoxLimit, &vgz) ||
      !floor_in(qx * rc, kChunkLimit, &cx) || !floor_in(qy * rc, kChunkLimit, &cy) || !floor_in(qz * rc, kChunkLimit, &cz))
    return false;
  const int x = vgx - cx * 8, y = vgy - cy * 8, z = vgz - cz * 8;
  if ((unsigned)x > 7u || (unsigned)y > 7u || (unsigned)z > 7u) return false;  // (f32 rounding far from the origin)
  const uint32_t centre = lookup_cached(v, cc, cx, cy, cz);
  if (centre == kInvalidSlot) return false;
  float xm, xp, ym, yp, zm, zp;
  if (!face_sdf(v, centre, x == 0, cx - 1, cy, cz, (x + 7) & 7, y, z, &xm)) return false;
  if (!face_sdf(v, centre, x == 7, cx + 1, cy, cz, (x + 1) & 7, y, z, &xp)) return false;
  if (!face_sdf(v, centre, y == 0, cx, cy - 1, cz, x, (y + 7) & 7, z, &ym)) return false;
  if (!face_sdf(v, centre, y == 7, cx, cy + 1, cz, x, (y + 1) & 7, z, &yp)) return false;
  if (!face_sdf(v, centre, z == 0, cx, cy, cz - 1, x, y, (z + 7) & 7, &zm)) return false;
  if (!face_sdf(v, centre, z == 7, cx, cy, cz + 1, x, y, (z + 1) & 7, &zp)) return false;
  *gx = xp - xm;
  *gy = yp - ym;
  *gz = zp - zm;
  return true;
}

__global__ __launch_bounds__(256) void k_query(VolumeDev v, QueryArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const float px = a.xyz[3 * (size_t)i], py = a.xyz[3 * (size_t)i + 1], pz = a.xyz[3 * (size_t)i + 2];
  ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
  uint32_t fl = 0;
  if (a.want & 3u) {
    uint32_t slot;
    int id;
    if (point_voxel(v, cc, px, py, pz, a.res, &slot, &id)) {
      const float2 sw = v.tsdf[(size_t)slot * kChunkVoxels + id];
      if ((a.want & 1u) && (double)sw.y > 1e-12) { a.sdf[i] = sw.x; fl |= 1u; }
      if (a.want & 2u) { a.weight[i] = sw.y; fl |= 2u; }
    }
    if ((a.want & 1u) && !(fl & 1u)) a.sdf[i] = 0.f;
    if ((a.want & 2u) && !(fl & 2u)) a.weight[i] = 0.f;
  }
  if (a.want & 4u) {
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (point_gradient(v, cc, px, py, pz, a.res, &gx, &gy, &gz)) fl |= 4u;
    else gx = gy = gz = 0.f;
    a.grad[3 * (size_t)i] = gx; a.grad[3 * (size_t)i + 1] = gy; a.grad[3 * (size_t)i + 2] = gz;
  }
  if (a.want & 24u) {
    float s = 0.f, rgb[3] = {0.f, 0.f, 0.f};
    bool okc = false;
    const bool ok = (a.want & 16u) ? tri_sample<true>(v, cc, px, py, pz, 1.0f / a.res, &s, rgb, &okc)
                                   : tri_sample<false>(v, cc, px, py, pz, 1.0f / a.res, &s);
    if (a.want & 8u) { a.sdf_tri[i] = ok ? s : 0.f; if (ok) fl |= 8u; }
    if (a.want & 16u) {
      if (!okc) rgb[0] = rgb[1] = rgb[2] = 0.f;
      else fl |= 16u;
      a.rgb[3 * (size_t)i] = (uint8_t)rgb[0]; a.rgb[3 * (size_t)i + 1] = (uint8_t)rgb[1]; a.rgb[3 * (size_t)i + 2] = (uint8_t)rgb[2];
    }
  }
  a.flags[i] = fl;
}

struct RayArgs {
  float R[9], t[3];
  float fx, fy, cxs, cys;  // int-truncated intrinsics, cx + 0.5 / cy + 0.5 (the integrator's projection)
  int W, H, tiles_x;
  float near_p, far_p;
  int max_steps;
  float res;
  size_t plane;  // W * H
  float* depth;
  float* normal;
  uint8_t* rgba;
  float* vertex;
};

// one wave per 8 x 8 pixel tile (lane = 8 y + x): neighbouring rays march through the same chunks
__device__ __forceinline__ void raycast_body(const VolumeDev& v, const RayArgs& a) {
  const int lane = threadIdx.x;
  const int px = (blockIdx.x % a.tiles_x) * 8 + (lane & 7), py = (blockIdx.x / a.tiles_x) * 8 + (lane >> 3);
  if (px >= a.W || py >= a.H) return;
  const float res = a.res, ir = 1.0f / res, cs = 8.0f * res, rc = 1.0f / (8.0f * res), eps = res * 0.015625f, gap = kRayGap * res;
  // ray through the pixel centre, camera frame z = 1: t is the camera-frame depth
  const float dcx = ((float)px - a.cxs) / a.fx, dcy = ((float)py - a.cys) / a.fy;
  const float dx = (a.R[0] * dcx + a.R[1] * dcy) + a.R[2];
  const float dy = (a.R[3] * dcx + a.R[4] * dcy) + a.R[5];
  const float dz = (a.R[6] * dcx + a.R[7] * dcy) + a.R[8];
  const float ox = a.t[0], oy = a.t[1], oz = a.t[2];
  ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
  float t = a.near_p, pt = 0.f, ps = 0.f, thit = -1.f;
  bool pok = false;
  for (int step = 0; step < a.max_steps && t <= a.far_p; ++step) {  // the step cap bounds the loop whatever the volume holds
    const float x = ox + t * dx, y = oy + t * dy, z = oz + t * dz;
    int cx, cy, cz;
    if (!floor_in(x * rc, kChunkLimit, &cx) || !floor_in(y * rc, kChunkLimit, &cy) || !floor_in(z * rc, kChunkLimit, &cz)) break;
    if (lookup_cached(v, cc, cx, cy, cz) == kInvalidSlot) {
      // absent chunk: every sample inside it is invalid (the voxel holding the point is one of its corners) -- jump to the
      // ray's exit from the chunk's box
      const float tx = dx > 0.f ? ((float)(cx + 1) * cs - ox) / dx : (dx < 0.f ? ((float)cx * cs - ox) / dx : INFINITY);
      const float ty = dy > 0.f ? ((float)(cy + 1) * cs - oy) / dy : (dy < 0.f ? ((float)cy * cs - oy) / dy : INFINITY);
      const float tz = dz > 0.f ? ((float)(cz + 1) * cs - oz) / dz : (dz < 0.f ? ((float)cz * cs - oz) / dz : INFINITY);
      t = fmaxf(fminf(fminf(tx, ty), tz), t) + eps;
      pok = false;
      continue;
    }
    float s;
    if (!tri_sample<false>(v, cc, x, y, z, ir, &s)) {  // (the last valid sample stays: voxels that only hole pixels saw
      t = t + res;                                       // leave one-voxel gaps in the band right behind a surface)
      continue;
    }
    pok = pok && t - pt <= gap;  // a crossing pairs two valid samples at most kRayGap voxels apart
    if (pok && ps > 0.f && s <= 0.f) { thit = pt + (t - pt) * (ps / (ps - s)); break; }
    if (pok && ps <= 0.f && s > 0.f) break;  // - -> +: leaving a surface from behind
    pt = t;
    ps = s;
    pok = true;
    t = t + fmaxf(res, kRayStepK * s);
  }
  const size_t o = (size_t)py * a.W + px;
  const bool hit = thit >= 0.f;
  const float hx = ox + thit * dx, hy = oy + thit * dy, hz = oz + thit * dz;
  if (a.depth) a.depth[o] = hit ? thit : 0.f;
  if (a.vertex) {
    a.vertex[o] = hit ? hx : 0.f; a.vertex[a.plane + o] = hit ? hy : 0.f; a.vertex[2 * a.plane + o] = hit ? hz : 0.f;
  }
  if (a.normal) {
    float n[3] = {0.f, 0.f, 0.f};
    if (hit) {
      // central differences of the trilinear SDF, one voxel each way (tap k: axis k >> 1, sign - / + by k & 1).  An axis
      // with one invalid tap takes the one-sided difference against the hit itself, where the SDF is 0 (the refined
      // crossing), doubled; an axis with none valid leaves the normal 0.
      float sp[3] = {0.f, 0.f, 0.f}, sm[3] = {0.f, 0.f, 0.f};
      uint32_t okm = 0;
#pragma unroll 1
      for (int k = 0; k < 6; ++k) {
        const float h = (k & 1) ? res : -res;
        float s = 0.f;
        if (tri_sample<false>(v, cc, hx + ((k >> 1) == 0 ? h : 0.f), hy + ((k >> 1) == 1 ? h : 0.f),
                              hz + ((k >> 1) == 2 ? h : 0.f), ir, &s)) okm |= 1u << k;
        if ((k >> 1) == 0) { if (k & 1) sp[0] = s; else sm[0] = s; }
        else if ((k >> 1) == 1) { if (k & 1) sp[1] = s; else sm[1] = s; }
        else { if (k & 1) sp[2] = s; else sm[2] = s; }
      }
      float g[3];
      bool ok = true;
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        const uint32_t m = (okm >> (2 * ax)) & 3u;  // bit 0: minus tap, bit 1: plus tap
        g[ax] = m == 3u ? sp[ax] - sm[ax] : (m == 2u ? 2.f * sp[ax] : -2.f * sm[ax]);
        ok = ok && m != 0u;
      }
      if (ok) {
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        if (len > 0.f) { n[0] = g[0] / len; n[1] = g[1] / len; n[2] = g[2] / len; }
      }
    }
    a.normal[o] = n[0]; a.normal[a.plane + o] = n[1]; a.normal[2 * a.plane + o] = n[2];
  }
  if (a.rgba) {
    float rgb[3] = {0.f, 0.f, 0.f}, s;
    bool okc = false;
    if (hit) tri_sample<true>(v, cc, hx, hy, hz, ir, &s, rgb, &okc);
    uchar4 c;
    c.x = okc ? (uint8_t)rgb[0] : 0; c.y = okc ? (uint8_t)rgb[1] : 0; c.z = okc ? (uint8_t)rgb[2] : 0;
    c.w = hit ? 255 : 0;
    reinterpret_cast<uchar4*>(a.rgba)[o] = c;
  }
}
__global__ __launch_bounds__(64) void k_raycast(VolumeDev v, RayArgs a) { raycast_body(v, a); }
// the same march from a pose in device memory (tf_devpose.h): R and t come from the cell through a uniform pointer; a
// cell that holds no pose leaves the maps as they are (whoever reads them is gated by the same cell)
__global__ __launch_bounds__(64) void k_raycast_posed(VolumeDev v, RayArgs a, const tf_device_pose* __restrict__ cell) {
  if (!devpose_ok(cell)) return;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a.R[3 * r + c] = cell->pose[4 * r + c];
    a.t[r] = cell->pose[4 * r + 3];
  }
  raycast_body(v, a);
}

// ---- Chisel::GetDistanceFromSurface / RefineFrameInVoxel (Structure/Chisel.h:251-342, 377-451) ----------------------

// voxel coordinate of a corner: absent unless finite and |c| <= 2^23 - 1 (the reference converts any float to int)
__device__ __forceinline__ bool vox_in(float c, int* out) {
  if (!(fabsf(c) <= kVoxLimit)) return false;
  *out = (int)c;
  return true;
}

// GetDistanceFromSurface at world point p: the weight-averaged trilinear SDF over the 8 voxels around p - res / 2.
// cc caches the base corner's chunk (corner 0: floor on every axis), cn the last other chunk a corner fell in.  Those go
// through the hash, not the base chunk's neighbour-table row: a non-zero word may name a parked chunk, and a pool slot
// carries no alive state of its own (HEntry::alive does) -- HasChunk must be false there, and weight 0 is not the same.
__device__ __forceinline__ float surface_dist(const VolumeDev& v, ChunkCache& cc, ChunkCache& cn, float px, float py,
                                             float pz, float half, float step, float* tsdf_weight) {
  const float rx = (px - half) * step, ry = (py - half) * step, rz = (pz - half) * step;
  const float flx = floorf(rx), fly = floorf(ry), flz = floorf(rz);
  const float dX = rx - flx, dY = ry - fly, dZ = rz - flz;
  int fx, fy, fz, cx, cy, cz;
  const bool okfx = vox_in(flx, &fx), okfy = vox_in(fly, &fy), okfz = vox_in(flz, &fz);
  const bool okcx = vox_in(ceilf(rx), &cx), okcy = vox_in(ceilf(ry), &cy), okcz = vox_in(ceilf(rz), &cz);
  const uint32_t base = (okfx && okfy && okfz) ? lookup_cached(v, cc, fx >> 3, fy >> 3, fz >> 3) : kInvalidSlot;
  float weight = 0.f, distance = 0.f, tw = 0.f;
#pragma unroll 1
  for (int k = 0; k < 8; ++k) {  // the reference's corner order: x from bit 2, y from bit 1, z from bit 0 (ceil where set)
    const bool sx = (k >> 2) & 1, sy = (k >> 1) & 1, sz = k & 1;
    if (!(sx ? okcx : okfx) || !(sy ? okcy : okfy) || !(sz ? okcz : okfz)) continue;
    const int Vx = sx ? cx : fx, Vy = sy ? cy : fy, Vz = sz ? cz : fz;
    const int bx = Vx >> 3, by = Vy >> 3, bz = Vz >> 3;  // = floor((float)V / 8.0f): V is exact in f32, /8 is exact
    const uint32_t slot = (bx == (fx >> 3) && by == (fy >> 3) && bz == (fz >> 3) && okfx && okfy && okfz)
                              ? base : lookup_cached(v, cn, bx, by, bz);
    if (slot == kInvalidSlot) continue;
    const float ax = sx ? dX : 1.f - dX, ay = sy ? dY : 1.f - dY, az = sz ? dZ : 1.f - dZ;
    const float sw = (ax * ay) * az;
    const float2 d = v.tsdf[(size_t)slot * kChunkVoxels + ((Vz & 7) * 8 + (Vy & 7)) * 8 + (Vx & 7)];
    weight = weight + sw * d.y;
    distance = distance + (d.x * sw) * d.y;
    tw = tw + d.y * sw;
  }
  if (weight > 0.f) {
    distance = distance / weight;
    tw = tw / weight;
  }
  *tsdf_weight = tw;
  return distance;
}

struct SurfArgs {
  const float* xyz;
  uint32_t n;
  float half, step;
  float* dist;
  float* tw;
};

__global__ __launch_bounds__(256) void k_surface_dist(VolumeDev v, SurfArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot}, cn{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
  float tw;
  a.dist[i] = surface_dist(v, cc, cn, a.xyz[3 * (size_t)i], a.xyz[3 * (size_t)i + 1], a.xyz[3 * (size_t)i + 2], a.half,
                           a.step, &tw);
  a.tw[i] = tw;
}

struct RefineArgs {
  float R[9], t[3];
  float fx, fy, cx, cy;  // int-truncated intrinsics (PinholeCamera::GetFx ... return int), used as float
  int W, H, tiles_x;
  float near_p, far_p;
  float half, step;
  float* depth;
  float* weight;
};

// one wave per 8 x 8 pixel tile (lane = 8 y + x), as k_raycast: neighbouring pixels read the same chunks
__global__ __launch_bounds__(64) void k_refine_frame(VolumeDev v, RefineArgs a) {
  const int lane = threadIdx.x;
  const int j = (blockIdx.x % a.tiles_x) * 8 + (lane & 7), i = (blockIdx.x / a.tiles_x) * 8 + (lane >> 3);
  if (j >= a.W || i >= a.H) return;
  const size_t o = (size_t)i * a.W + j;
  float depth = a.depth[o];
  if ((double)depth < 0.05 || (double)depth > 3.0) return;  // skipped: depth and weight untouched
  const float dx = ((float)j - a.cx) / a.fx, dy = ((float)i - a.cy) / a.fy;
  // R * (dx, dy, 1): a0 b0 + (a1 b1 + a2 b2) per row, a2 * 1 exact
  const float rx = a.R[0] * dx + (a.R[1] * dy + a.R[2]);
  const float ry = a.R[3] * dx + (a.R[4] * dy + a.R[5]);
  const float rz = a.R[6] * dx + (a.R[7] * dy + a.R[8]);
  const float depth_init = depth;
  ChunkCache cc{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot}, cn{INT_MIN, INT_MIN, INT_MIN, kInvalidSlot};
  float d = 0.f, tw = 0.f;
#pragma unroll 1
  for (int r = 0; r < 6; ++r) {
    d = surface_dist(v, cc, cn, rx * depth + a.t[0], ry * depth + a.t[1], rz * depth + a.t[2], a.half, a.step, &tw);
    depth = depth + d;
  }
  // the three rejections in the reference's order, each on the value written so far (double constants compared in double)
  if (fabs((double)d) > 5e-3) { depth = 0.f; tw = 0.f; }
  if (depth > a.far_p || depth < a.near_p) { depth = 0.f; tw = 0.f; }
  if (fabs((double)(depth - depth_init)) > 0.1) { depth = 0.f; tw = 0.f; }
  a.depth[o] = depth;
  a.weight[o] = tw;
}

}  // namespace tf

using namespace tf;

namespace {

int query_launch(tf_volume* v, const float* d_xyz, uint32_t n, uint32_t want, float* sdf, float* weight, float* grad3,
                 float* sdf_tri, uint8_t* rgb3, uint32_t* flags) {
  QueryArgs a{d_xyz, n, want, v->res, sdf, weight, grad3, sdf_tri, rgb3, flags};
  hipLaunchKernelGGL(k_query, dim3((n + 255) / 256), dim3(256), 0, v->stream, v->dev, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int query_check(tf_volume* v, const float* xyz, int64_t n, uint32_t want, const float* sdf, const float* weight,
                const float* grad3, const float* sdf_tri, const uint8_t* rgb3, const uint32_t* flags) {
  if (!v || (n > 0 && (!xyz || !flags))) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n < 0 || n > 0x7FFFFFFFll) { set_error("point count out of range"); return TF_ERR_INVALID; }
  if (want & ~31u) { set_error("want_mask: unknown bits (0 sdf, 1 weight, 2 grad, 3 sdf_tri, 4 rgb_tri)"); return TF_ERR_INVALID; }
  if (((want & 1u) && !sdf) || ((want & 2u) && !weight) || ((want & 4u) && !grad3) || ((want & 8u) && !sdf_tri) ||
      ((want & 16u) && !rgb3)) {
    set_error("a requested output is null");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

struct RayCam { float fx, fy, cx, cy; int W, H; };

bool pose_finite(const float* pose) {
  for (int i = 0; i < 12; ++i)
    if (!isfinite(pose[i])) return false;
  return true;
}

// camera-to-world 3x4 pose -> rotation (row-major) and translation
void split_pose(const float* pose, float R[9], float t[3]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[3 * r + c] = pose[4 * r + c];
    t[r] = pose[4 * r + 3];
  }
}

int ray_check(tf_volume* v, const float* pose, float near_plane, float far_plane, int32_t max_steps, RayCam* cam) {
  if (!v || !pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!(near_plane >= 0.f) || !(far_plane > near_plane) || !isfinite(far_plane)) {
    set_error("need 0 <= near < far < inf");
    return TF_ERR_INVALID;
  }
  if (max_steps <= 0) { set_error("max_steps must be positive"); return TF_ERR_INVALID; }
  if (!pose_finite(pose)) { set_error("pose is not finite"); return TF_ERR_INVALID; }
  if (v->ray_w > 0) *cam = {v->ray_fx, v->ray_fy, v->ray_cx, v->ray_cy, v->ray_w, v->ray_h};
  else *cam = {v->cam.fxi, v->cam.fyi, v->cam.cxi, v->cam.cyi, v->cam.W, v->cam.H};
  if (cam->W <= 0 || cam->H <= 0 || !(cam->fx > 0.f) || !(cam->fy > 0.f)) {
    set_error("no camera (tf_set_camera / tf_raycast_camera)");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

// d_cell != null: the pose is read from that cell on the device (k_raycast_posed; `pose` is not read)
int ray_launch(tf_volume* v, const float* pose, float near_plane, float far_plane, int32_t max_steps, const RayCam& cam,
               float* depth, float* normal, uint8_t* rgba, float* vertex, const tf_device_pose* d_cell = nullptr) {
  RayArgs a{};
  if (!d_cell) split_pose(pose, a.R, a.t);
  a.fx = cam.fx; a.fy = cam.fy; a.cxs = cam.cx + 0.5f; a.cys = cam.cy + 0.5f;
  a.W = cam.W; a.H = cam.H; a.tiles_x = (cam.W + 7) / 8;
  a.near_p = near_plane; a.far_p = far_plane; a.max_steps = max_steps; a.res = v->res;
  a.plane = (size_t)cam.W * cam.H;
  a.depth = depth; a.normal = normal; a.rgba = rgba; a.vertex = vertex;
  const unsigned tiles = (unsigned)(a.tiles_x * ((cam.H + 7) / 8));
  if (d_cell) hipLaunchKernelGGL(k_raycast_posed, dim3(tiles), dim3(64), 0, v->stream, v->dev, a, d_cell);
  else hipLaunchKernelGGL(k_raycast, dim3(tiles), dim3(64), 0, v->stream, v->dev, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int surf_launch(tf_volume* v, const float* d_xyz, uint32_t n, float* d_dist, float* d_tw) {
  SurfArgs a{d_xyz, n, v->res / 2.0f, 1.0f / v->res, d_dist, d_tw};
  hipLaunchKernelGGL(k_surface_dist, dim3((n + 255) / 256), dim3(256), 0, v->stream, v->dev, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int surf_check(tf_volume* v, const float* xyz, int64_t n, const float* dist, const float* tw) {
  if (!v || (n > 0 && (!xyz || !dist || !tw))) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n < 0 || n > 0x7FFFFFFFll) { set_error("point count out of range"); return TF_ERR_INVALID; }
  return TF_OK;
}

int refine_check(tf_volume* v, const float* depth, const float* weight, const float* pose) {
  if (!v || !depth || !weight || !pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!pose_finite(pose)) { set_error("pose is not finite"); return TF_ERR_INVALID; }
  if (v->cam.W <= 0 || v->cam.H <= 0) { set_error("no camera (tf_set_camera)"); return TF_ERR_INVALID; }
  return TF_OK;
}

int refine_launch(tf_volume* v, const float* pose, float* d_depth, float* d_weight) {
  RefineArgs a;
  split_pose(pose, a.R, a.t);
  a.fx = v->cam.fxi; a.fy = v->cam.fyi; a.cx = v->cam.cxi; a.cy = v->cam.cyi;
  a.W = v->cam.W; a.H = v->cam.H; a.tiles_x = (v->cam.W + 7) / 8;
  a.near_p = v->cam.nearP; a.far_p = v->cam.farP;
  a.half = v->res / 2.0f; a.step = 1.0f / v->res;
  a.depth = d_depth; a.weight = d_weight;
  const unsigned tiles = (unsigned)(a.tiles_x * ((v->cam.H + 7) / 8));
  hipLaunchKernelGGL(k_refine_frame, dim3(tiles), dim3(64), 0, v->stream, v->dev, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace

// tf_raycast_device's launch at the pose in *d_cell (tf_devpose.hip: the device tracker's model maps)
int tf::raycast_posed(tf_volume* v, const tf_device_pose* d_cell, float near_plane, float far_plane, int32_t max_steps,
                      float* d_normal, float* d_vertex) {
  const float eye[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  RayCam cam;
  const int rc = ray_check(v, eye, near_plane, far_plane, max_steps, &cam);
  return rc ? rc : ray_launch(v, eye, near_plane, far_plane, max_steps, cam, nullptr, d_normal, nullptr, d_vertex, d_cell);
}

// the vertex and normal maps of a camera that is neither the handle's nor tf_raycast_camera's -- a level of the projective
// ICP's depth pyramid -- at `pose`, or at the pose in *d_cell where that is given; the caller has checked the parameters
int tf::raycast_level(tf_volume* v, const float* pose, const tf_device_pose* d_cell, float near_plane, float far_plane,
                      int32_t max_steps, const AlignCam& cam, float* d_normal, float* d_vertex) {
  const float eye[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  const RayCam rc{cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H};
  return ray_launch(v, d_cell ? eye : pose, near_plane, far_plane, max_steps, rc, nullptr, d_normal, nullptr, d_vertex, d_cell);
}

extern "C" {

int tf_query_points_device(tf_volume* v, const float* d_xyz, int64_t n, uint32_t want_mask, float* d_sdf, float* d_weight,
                           float* d_grad3, float* d_sdf_tri, uint8_t* d_rgb3, uint32_t* d_flags) {
  int rc = query_check(v, d_xyz, n, want_mask, d_sdf, d_weight, d_grad3, d_sdf_tri, d_rgb3, d_flags);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (n == 0) return TF_OK;
  return query_launch(v, d_xyz, (uint32_t)n, want_mask, d_sdf, d_weight, d_grad3, d_sdf_tri, d_rgb3, d_flags);
}

int tf_query_points(tf_volume* v, const float* xyz, int64_t n, uint32_t want_mask, float* sdf, float* weight, float* grad3,
                    float* sdf_tri, uint8_t* rgb3, uint32_t* flags) {
  int rc = query_check(v, xyz, n, want_mask, sdf, weight, grad3, sdf_tri, rgb3, flags);
  if (rc) return rc;
  TF_DEV_READER(v);
  if (n == 0) return TF_OK;
  // staging: xyz | sdf | weight | grad | sdf_tri | flags | rgb
  Layout L;
  const size_t N = (size_t)n;
  const size_t o_xyz = L.take(12 * N), o_s = L.take(4 * N), o_w = L.take(4 * N), o_g = L.take(12 * N), o_t = L.take(4 * N),
               o_f = L.take(4 * N), o_c = L.take(3 * N);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_xyz, xyz, 12 * N))) return rc;
  rc = query_launch(v, sg.dp<const float>(o_xyz), (uint32_t)n, want_mask, sg.dp<float>(o_s), sg.dp<float>(o_w),
                    sg.dp<float>(o_g), sg.dp<float>(o_t), sg.d + o_c, sg.dp<uint32_t>(o_f));
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_s, sg.d + o_s, L.size - o_s, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (want_mask & 1u) memcpy(sdf, sg.h + o_s, 4 * N);
  if (want_mask & 2u) memcpy(weight, sg.h + o_w, 4 * N);
  if (want_mask & 4u) memcpy(grad3, sg.h + o_g, 12 * N);
  if (want_mask & 8u) memcpy(sdf_tri, sg.h + o_t, 4 * N);
  if (want_mask & 16u) memcpy(rgb3, sg.h + o_c, 3 * N);
  memcpy(flags, sg.h + o_f, 4 * N);
  return TF_OK;
}

int tf_raycast_camera(tf_volume* v, float fx, float fy, float cx, float cy, int width, int height) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  if (width < 0 || height < 0 || (width > 0) != (height > 0) || width > kRayMaxSide || height > kRayMaxSide) {
    set_error("raycast camera: width and height both in 1..32768, or both 0 (= the handle's camera)");
    return TF_ERR_INVALID;
  }
  const float lim = 2147483648.0f;  // 2^31: the int truncation below is defined only inside (-2^31, 2^31)
  if (!(fabsf(fx) < lim) || !(fabsf(fy) < lim) || !(fabsf(cx) < lim) || !(fabsf(cy) < lim)) {
    set_error("raycast camera: fx, fy, cx, cy must be finite and of magnitude below 2^31");
    return TF_ERR_INVALID;
  }
  if (width > 0 && (!(fx >= 1.f) || !(fy >= 1.f))) { set_error("raycast camera: fx, fy must be >= 1"); return TF_ERR_INVALID; }
  v->ray_fx = (float)(int)fx;  // truncated like PinholeCamera::GetFx (the integrator's convention)
  v->ray_fy = (float)(int)fy;
  v->ray_cx = (float)(int)cx;
  v->ray_cy = (float)(int)cy;
  v->ray_w = width;
  v->ray_h = height;
  return TF_OK;
}

int tf_raycast_device(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t max_steps,
                      float* d_depth, float* d_normal, uint8_t* d_rgba, float* d_vertex) {
  RayCam cam;
  int rc = ray_check(v, pose, near_plane, far_plane, max_steps, &cam);
  if (rc) return rc;
  TF_DEV_READER(v);
  return ray_launch(v, pose, near_plane, far_plane, max_steps, cam, d_depth, d_normal, d_rgba, d_vertex);
}

int tf_raycast(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t max_steps, float* depth,
               float* normal, uint8_t* rgba, float* vertex) {
  RayCam cam;
  int rc = ray_check(v, pose, near_plane, far_plane, max_steps, &cam);
  if (rc) return rc;
  TF_DEV_READER(v);
  const size_t P = (size_t)cam.W * cam.H;
  Layout L;
  const size_t o_d = L.take(depth ? 4 * P : 0), o_n = L.take(normal ? 12 * P : 0), o_c = L.take(rgba ? 4 * P : 0),
               o_v = L.take(vertex ? 12 * P : 0);
  if (L.size == 0) return TF_OK;
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg))) return rc;
  rc = ray_launch(v, pose, near_plane, far_plane, max_steps, cam, depth ? sg.dp<float>(o_d) : nullptr,
                  normal ? sg.dp<float>(o_n) : nullptr, rgba ? sg.d + o_c : nullptr, vertex ? sg.dp<float>(o_v) : nullptr);
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h, sg.d, L.size, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (depth) memcpy(depth, sg.h + o_d, 4 * P);
  if (normal) memcpy(normal, sg.h + o_n, 12 * P);
  if (rgba) memcpy(rgba, sg.h + o_c, 4 * P);
  if (vertex) memcpy(vertex, sg.h + o_v, 12 * P);
  return TF_OK;
}

int tf_distance_from_surface_device(tf_volume* v, const float* d_xyz, int64_t n, float* d_dist, float* d_tsdf_weight) {
  int rc = surf_check(v, d_xyz, n, d_dist, d_tsdf_weight);
  if (rc) return rc;
  TF_DEV(v);
  if (n == 0) return TF_OK;
  return surf_launch(v, d_xyz, (uint32_t)n, d_dist, d_tsdf_weight);
}

int tf_distance_from_surface(tf_volume* v, const float* xyz, int64_t n, float* dist, float* tsdf_weight) {
  int rc = surf_check(v, xyz, n, dist, tsdf_weight);
  if (rc) return rc;
  TF_DEV(v);
  if (n == 0) return TF_OK;
  const size_t N = (size_t)n;
  Layout L;
  const size_t o_xyz = L.take(12 * N), o_d = L.take(4 * N), o_w = L.take(4 * N);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_xyz, xyz, 12 * N))) return rc;
  rc = surf_launch(v, sg.dp<const float>(o_xyz), (uint32_t)n, sg.dp<float>(o_d), sg.dp<float>(o_w));
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_d, sg.d + o_d, L.size - o_d, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(dist, sg.h + o_d, 4 * N);
  memcpy(tsdf_weight, sg.h + o_w, 4 * N);
  return TF_OK;
}

int tf_refine_frame_in_voxel_device(tf_volume* v, float* d_depth, float* d_weight, const float pose[12]) {
  int rc = refine_check(v, d_depth, d_weight, pose);
  if (rc) return rc;
  TF_DEV(v);
  return refine_launch(v, pose, d_depth, d_weight);
}

int tf_refine_frame_in_voxel(tf_volume* v, float* depth, float* weight, const float pose[12]) {
  int rc = refine_check(v, depth, weight, pose);
  if (rc) return rc;
  TF_DEV(v);
  const size_t P = (size_t)v->cam.W * v->cam.H;
  Layout L;
  const size_t o_d = L.take(4 * P), o_w = L.take(4 * P);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg))) return rc;
  memcpy(sg.h + o_d, depth, 4 * P);
  memcpy(sg.h + o_w, weight, 4 * P);  // (skipped pixels keep the caller's weight)
  TF_HIP(hipMemcpyAsync(sg.d, sg.h, L.size, hipMemcpyHostToDevice, v->stream));
  rc = refine_launch(v, pose, sg.dp<float>(o_d), sg.dp<float>(o_w));
  if (rc) return rc;
  TF_HIP(hipMemcpyAsync(sg.h, sg.d, L.size, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  memcpy(depth, sg.h + o_d, 4 * P);
  memcpy(weight, sg.h + o_w, 4 * P);
  return TF_OK;
}

}  // extern "C"
