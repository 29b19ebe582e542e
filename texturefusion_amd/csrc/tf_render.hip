// tf_render.hip -- the textured model from a pose: a software rasteriser over the DrawMeshes stream and the atlas.
//
// What the reference's GL viewer does with Chisel::DrawMeshes' stream and Atlas::texture_buffer (GCFusion/MobileFusion.h:
// 404-476, Shaders/draw_mesh.vert / .frag, Shaders/color.glsl), done in HIP: colour, camera-frame depth and triangle id
// of the nearest surface per pixel, left in device memory.  Everything here only READS its inputs (stream, texture /
// atlas); the volume, the meshes and the patches are not touched at all.
//
//   k_render_bin      one lane per triangle: setup, then either the triangle's own samples (a viewport-clipped bounding
//                     box of at most kSmallSamples = 64 samples) or an append to the queue of large triangles
//   k_render_large    one workgroup per queued triangle, its 256 lanes striding over the box -- no lane ever loops over
//                     an image-sized box
//   k_render_resolve  one lane per pixel: the winning triangle's setup again (the same code, so the same bits),
//                     attributes, texture, shading
// The depth test between the first two and the third is one 64-bit word per pixel, key = bits(z) << 32 | triangle, taken
// with atomicMin (one global_atomic_umin_x2): z > 0, so floats order like their bits -- the nearest fragment wins, the
// lower triangle index on equal depth, whatever order fragments arrive in.  A plain load goes first and the atomic is
// skipped when the stored key is already smaller (the word only ever decreases).  Two runs give the same bits.
//
// Arithmetic, all f32 with every operation rounded on its own (-ffp-contract=off), integers where stated;
// tests/render_ref.py restates it operation by operation:
//   camera      the camera tf_raycast uses (tf_raycast_camera, else tf_set_camera; int-truncated intrinsics);
//               pose = camera-to-world [R | t]
//   vertex      d = p - t per axis;  camera frame  c_k = R[0][k] d.x + (R[1][k] d.y + R[2][k] d.z)   (= R^T d)
//               sx = fx * (c.x / c.z) + (cx + 0.5),  sy = fy * (c.y / c.z) + (cy + 0.5)  -- pixel (x, y) is sampled at
//               (sx, sy) = (x, y): the ray tf_raycast casts for that pixel, so a surface lands on the same pixel
//               X = (int)floorf(sx * 256 + 0.5),  Y likewise: 1 / 256 pixel
//   dropped     whole, no clipping: an index >= n_vertices (tested, never dereferenced); a camera coordinate that is
//               not finite; a vertex with c.z < near; a snapped coordinate beyond +-2^22 (+-16384 pixels: every edge
//               function stays far inside int64); snapped area 0.  No clipping is needed for what this renders: a
//               triangle of the model is at most a voxel diagonal long, so with near >= 0.05 m it cannot be partly in
//               view and partly beyond the guard band -- it is either wholly behind near / outside the band, or inside.
//   orientation no back-face culling (the reference enables none): area = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) in
//               int64; where it is negative vertices 1 and 2 swap, with everything they carry
//   coverage    E0 = (X2 - X1)(py - Y1) - (Y2 - Y1)(px - X1), E1 over edge 2 -> 0, E2 over edge 0 -> 1, int64, at
//               (px, py) = (256 x, 256 y); a sample is covered iff every E > 0, or E == 0 on an edge (dx, dy) with dy < 0
//               (a left edge, y down) or dy == 0 and dx > 0 (a horizontal top edge): two triangles sharing an edge
//               cover each sample on it exactly once
//   depth       l_i = (float)E_i / (float)(E0 + E1 + E2);  w_i = l_i / c_i.z;  z = 1 / (w0 + (w1 + w2));
//               the fragment is discarded unless near <= z <= far (a z that is not finite fails that)
//   attributes  a = (w0 a0 + (w1 a1 + w2 a2)) * z
//   shading     the reference's colorType: 1 colour = -normal; 2 decodeColor(col 4) per vertex, interpolated; 3 texture
//               + interpolated decodeSignedColor(col 5); 4 texture only.  In 3 and 4 a triangle whose FIRST vertex (in
//               stream order) has wrong_mapping != 0 takes mode 2's colour.  The reference's own quirk is kept: a
//               vertex with adj == 0 (no labs yet) decodes to a delta of -1 per channel, so unadjusted patches are
//               black in mode 3; mode 4 shows them.  (So is the stream's own: the 27-bit delta word travels as an f32,
//               which keeps 24 bits, so blue's field arrives rounded to a multiple of 4 or 8.)  The Phong branch is not
//               built.  The packed floats convert to int by truncation; one that is not inside (-2^31, 2^31) counts
//               as 0.
//   texture     GL_LINEAR, GL_CLAMP_TO_EDGE, one level: tc = u * tex_w - 0.5, f = floorf(tc), t = tc - f, taps
//               clamp((int)f, 0, tex_w - 1) and clamp((int)f + 1, 0, tex_w - 1) (f limited to [-1, tex_w] first), v
//               likewise; texel = u8 / 255; lerp(a, b, t) = a + t * (b - a): top = lerp(t00, t10, tx), bottom =
//               lerp(t01, t11, tx), result = lerp(top, bottom, ty)
//   output      rgba: c = fminf(fmaxf(c, 0), 1), (int)(c * 255 + 0.5), a = 255; an empty pixel is 0 0 0 0, depth 0,
//               triangle -1
// Deliberately not GL: no clipping (the guard band instead), no mip maps, no anti-aliasing, no Phong.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {

constexpr int kSmallSamples = 64;          // a triangle whose clipped box holds more samples goes to the queue
constexpr float kGuard = 4194304.0f;       // 2^22 snapped units = 16384 pixels
constexpr unsigned long long kNoKey = ~0ull;
constexpr unsigned kLargeGrid = 1024;      // workgroups of k_render_large (they stride over the queue)

struct RenderArgs {
  float R[9], t[3];
  float fx, fy, cxs, cys;  // int-truncated intrinsics, cx + 0.5 / cy + 0.5
  int W, H;
  float near_p, far_p;
  int mode;
  const float* vtx;
  uint32_t nv;
  const uint32_t* idx;
  uint32_t ntri;
  const uint8_t* tex;
  int tw, th;
  unsigned long long* keys;  // [H][W]
  uint32_t* queue;           // [ntri]
  uint32_t* qcount;
  const uint32_t* counts;    // null, or the model stream's control block: {n_vertices, n_indices, ...} bound nv / ntri
  uint8_t* rgba;
  float* depth;
  int32_t* tri;
};

struct Tri {
  int X0, Y0, X1, Y1, X2, Y2;
  float z0, z1, z2;
  uint32_t i0, i1, i2;  // vertices of the oriented triangle (i0 is the stream's first: 1 and 2 swap)
};

// the stream's lengths when they are device words (tf_model.hip's control block): nv / ntri as given are then the capacity
// the grids and the queue were sized from, and surplus lanes leave at once.  Wave-uniform loads: the counts stay scalar.
__device__ __forceinline__ void render_counts(RenderArgs& a) {
  if (!a.counts) return;
  a.nv = min(a.nv, a.counts[0]);
  a.ntri = min(a.ntri, a.counts[1] / 3u);
}

__device__ __forceinline__ bool render_vertex(const RenderArgs& a, uint32_t i, float* zc, int* X, int* Y) {
  const float* p = a.vtx + 12 * (size_t)i;
  const float dx = p[0] - a.t[0], dy = p[1] - a.t[1], dz = p[2] - a.t[2];
  const float cx = a.R[0] * dx + (a.R[3] * dy + a.R[6] * dz);
  const float cy = a.R[1] * dx + (a.R[4] * dy + a.R[7] * dz);
  const float cz = a.R[2] * dx + (a.R[5] * dy + a.R[8] * dz);
  if (!isfinite(cx) || !isfinite(cy) || !isfinite(cz)) return false;
  if (cz < a.near_p) return false;
  const float sx = a.fx * (cx / cz) + a.cxs, sy = a.fy * (cy / cz) + a.cys;
  const float qx = floorf(sx * 256.0f + 0.5f), qy = floorf(sy * 256.0f + 0.5f);
  if (!(fabsf(qx) <= kGuard) || !(fabsf(qy) <= kGuard)) return false;
  *zc = cz;
  *X = (int)qx;
  *Y = (int)qy;
  return true;
}

__device__ __forceinline__ long long cross2(int ax, int ay, int bx, int by) {
  return (long long)ax * (long long)by - (long long)ay * (long long)bx;
}

__device__ __forceinline__ bool tri_setup(const RenderArgs& a, uint32_t t, Tri* T) {
  const uint32_t i0 = a.idx[3 * (size_t)t], i1 = a.idx[3 * (size_t)t + 1], i2 = a.idx[3 * (size_t)t + 2];
  if (i0 >= a.nv || i1 >= a.nv || i2 >= a.nv) return false;
  if (!render_vertex(a, i0, &T->z0, &T->X0, &T->Y0) || !render_vertex(a, i1, &T->z1, &T->X1, &T->Y1) ||
      !render_vertex(a, i2, &T->z2, &T->X2, &T->Y2))
    return false;
  T->i0 = i0; T->i1 = i1; T->i2 = i2;
  const long long area = cross2(T->X1 - T->X0, T->Y1 - T->Y0, T->X2 - T->X0, T->Y2 - T->Y0);
  if (area == 0) return false;
  if (area < 0) {
    const int x = T->X1, y = T->Y1; T->X1 = T->X2; T->Y1 = T->Y2; T->X2 = x; T->Y2 = y;
    const float z = T->z1; T->z1 = T->z2; T->z2 = z;
    T->i1 = i2; T->i2 = i1;
  }
  return true;
}

// pixels whose sample may lie inside the triangle, clipped to the viewport; false = none
__device__ __forceinline__ bool tri_box(const RenderArgs& a, const Tri& T, int* x0, int* x1, int* y0, int* y1) {
  const int lx = min(T.X0, min(T.X1, T.X2)), hx = max(T.X0, max(T.X1, T.X2));
  const int ly = min(T.Y0, min(T.Y1, T.Y2)), hy = max(T.Y0, max(T.Y1, T.Y2));
  *x0 = max(0, (lx + 255) >> 8);  // arithmetic shifts: ceil / floor of a 1 / 256 coordinate
  *x1 = min(a.W - 1, hx >> 8);
  *y0 = max(0, (ly + 255) >> 8);
  *y1 = min(a.H - 1, hy >> 8);
  return *x0 <= *x1 && *y0 <= *y1;
}

// edge function over a -> b at sample (px, py), and whether a sample exactly on the edge belongs to the triangle
__device__ __forceinline__ bool edge_in(int ax, int ay, int bx, int by, int px, int py, long long* E) {
  const int dx = bx - ax, dy = by - ay;
  *E = cross2(dx, dy, px - ax, py - ay);
  return *E > 0 || (*E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// coverage and depth of the triangle at pixel (x, y): false = no fragment
__device__ __forceinline__ bool tri_fragment(const RenderArgs& a, const Tri& T, int x, int y, float* w0, float* w1,
                                             float* w2, float* z) {
  const int px = x << 8, py = y << 8;
  long long E0, E1, E2;
  const bool in0 = edge_in(T.X1, T.Y1, T.X2, T.Y2, px, py, &E0);
  const bool in1 = edge_in(T.X2, T.Y2, T.X0, T.Y0, px, py, &E1);
  const bool in2 = edge_in(T.X0, T.Y0, T.X1, T.Y1, px, py, &E2);
  if (!(in0 && in1 && in2)) return false;
  const float area = (float)(E0 + E1 + E2);
  *w0 = ((float)E0 / area) / T.z0;
  *w1 = ((float)E1 / area) / T.z1;
  *w2 = ((float)E2 / area) / T.z2;
  *z = 1.0f / (*w0 + (*w1 + *w2));
  return *z >= a.near_p && *z <= a.far_p;
}

__device__ __forceinline__ void tri_sample(const RenderArgs& a, const Tri& T, uint32_t t, int x, int y) {
  float w0, w1, w2, z;
  if (!tri_fragment(a, T, x, y, &w0, &w1, &w2, &z)) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | t;
  unsigned long long* k = a.keys + (size_t)y * a.W + x;
  if (*k <= key) return;  // the word only ever decreases
  atomicMin(k, key);
}

__global__ __launch_bounds__(256) void k_render_bin(RenderArgs a) {
  render_counts(a);
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.ntri) return;
  Tri T;
  int x0, x1, y0, y1;
  if (!tri_setup(a, t, &T) || !tri_box(a, T, &x0, &x1, &y0, &y1)) return;
  if ((x1 - x0 + 1) * (y1 - y0 + 1) > kSmallSamples) {  // (at most 32768^2 = 2^30)
    a.queue[atomicAdd(a.qcount, 1u)] = t;                // each triangle at most once: the queue holds ntri entries
    return;
  }
  for (int y = y0; y <= y1; ++y)
    for (int x = x0; x <= x1; ++x) tri_sample(a, T, t, x, y);
}

__global__ __launch_bounds__(256) void k_render_large(RenderArgs a) {
  render_counts(a);
  const uint32_t n = min(*a.qcount, a.ntri);
  for (uint32_t q = blockIdx.x; q < n; q += gridDim.x) {
    const uint32_t t = a.queue[q];
    Tri T;
    int x0, x1, y0, y1;
    if (t >= a.ntri || !tri_setup(a, t, &T) || !tri_box(a, T, &x0, &x1, &y0, &y1)) continue;
    const uint32_t bw = (uint32_t)(x1 - x0 + 1), cnt = bw * (uint32_t)(y1 - y0 + 1);
    for (uint32_t s = threadIdx.x; s < cnt; s += 256) tri_sample(a, T, t, x0 + (int)(s % bw), y0 + (int)(s / bw));
  }
}

__device__ __forceinline__ int packed_int(const float c) { return (c > -2147483648.0f && c < 2147483648.0f) ? (int)c : 0; }
__device__ __forceinline__ float interp(float w0, float w1, float w2, float z, float a0, float a1, float a2) {
  return (w0 * a0 + (w1 * a1 + w2 * a2)) * z;
}
__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + t * (b - a); }
// the two taps and the weight of one axis
__device__ __forceinline__ void tex_axis(float u, int n, int* i0, int* i1, float* t) {
  const float tc = u * (float)n - 0.5f;
  const float f = floorf(tc);
  *t = tc - f;
  const int i = (int)fminf(fmaxf(f, -1.0f), (float)n);
  *i0 = min(max(i, 0), n - 1);
  *i1 = min(max(i + 1, 0), n - 1);
}
__device__ __forceinline__ uint8_t to_u8(const float c) { return (uint8_t)(int)(fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f + 0.5f); }

__global__ __launch_bounds__(256) void k_render_resolve(RenderArgs a) {
  render_counts(a);
  const uint32_t o = blockIdx.x * 256 + threadIdx.x;
  if (o >= (uint32_t)(a.W * a.H)) return;
  const unsigned long long key = a.keys[o];
  const uint32_t t = (uint32_t)key;
  Tri T;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f, z = 0.f;
  const bool hit = key != kNoKey && t < a.ntri && tri_setup(a, t, &T) &&
                   tri_fragment(a, T, (int)(o % (uint32_t)a.W), (int)(o / (uint32_t)a.W), &w0, &w1, &w2, &z);
  if (a.depth) a.depth[o] = hit ? z : 0.f;
  if (a.tri) a.tri[o] = hit ? (int32_t)t : -1;
  if (!a.rgba) return;
  uchar4 out = make_uchar4(0, 0, 0, 0);
  if (hit) {
    const float* v0 = a.vtx + 12 * (size_t)T.i0;
    const float* v1 = a.vtx + 12 * (size_t)T.i1;
    const float* v2 = a.vtx + 12 * (size_t)T.i2;
    float c[3];
    if (a.mode == 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = interp(w0, w1, w2, z, -v0[8 + k], -v1[8 + k], -v2[8 + k]);
    } else if (a.mode == 2 || v0[11] != 0.0f) {
      const int p0 = packed_int(v0[4]), p1 = packed_int(v1[4]), p2 = packed_int(v2[4]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int sh = 16 - 8 * k;
        c[k] = interp(w0, w1, w2, z, (float)((p0 >> sh) & 0xFF) / 255.0f, (float)((p1 >> sh) & 0xFF) / 255.0f,
                      (float)((p2 >> sh) & 0xFF) / 255.0f);
      }
    } else {
      const float u = interp(w0, w1, w2, z, v0[6], v1[6], v2[6]), vv = interp(w0, w1, w2, z, v0[7], v1[7], v2[7]);
      int x0, x1, y0, y1;
      float tx, ty;
      tex_axis(u, a.tw, &x0, &x1, &tx);
      tex_axis(vv, a.th, &y0, &y1, &ty);
      const uint8_t* r0 = a.tex + (size_t)y0 * a.tw * 3;
      const uint8_t* r1 = a.tex + (size_t)y1 * a.tw * 3;
      const int p0 = packed_int(v0[5]), p1 = packed_int(v1[5]), p2 = packed_int(v2[5]);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float t00 = (float)r0[3 * (size_t)x0 + k] / 255.0f, t10 = (float)r0[3 * (size_t)x1 + k] / 255.0f;
        const float t01 = (float)r1[3 * (size_t)x0 + k] / 255.0f, t11 = (float)r1[3 * (size_t)x1 + k] / 255.0f;
        c[k] = lerp1(lerp1(t00, t10, tx), lerp1(t01, t11, tx), ty);
        if (a.mode == 3) {
          const int sh = 18 - 9 * k;
          c[k] = c[k] + interp(w0, w1, w2, z, (float)((p0 >> sh) & 0x1FF) / 255.0f - 1.0f,
                               (float)((p1 >> sh) & 0x1FF) / 255.0f - 1.0f, (float)((p2 >> sh) & 0x1FF) / 255.0f - 1.0f);
        }
      }
    }
    out = make_uchar4(to_u8(c[0]), to_u8(c[1]), to_u8(c[2]), 255);
  }
  reinterpret_cast<uchar4*>(a.rgba)[o] = out;
}

}  // namespace tf

using namespace tf;

namespace {

struct RenderCam { float fx, fy, cx, cy; int W, H; };

int render_check(tf_volume* v, int64_t n_vertices, int64_t n_indices, const void* tex, int tex_w, int tex_h,
                 const float* pose, float near_plane, float far_plane, int mode, const void* rgba, const void* depth,
                 const void* tri, RenderCam* cam) {
  if (!v || !pose) { set_error("null argument"); return TF_ERR_INVALID; }
  if (mode < 1 || mode > 4) { set_error("render mode: 1 normals, 2 vertex colour, 3 texture + delta, 4 texture"); return TF_ERR_INVALID; }
  if (n_vertices < 0 || n_vertices > 0x7FFFFFFFll || n_indices < 0 || n_indices > 3 * 0x7FFFFFFFll) {
    set_error("vertex / index count out of range");
    return TF_ERR_INVALID;
  }
  if (n_indices % 3) { set_error("n_indices is not a multiple of 3"); return TF_ERR_INVALID; }
  if (!(near_plane >= 0.f) || !(far_plane > near_plane) || !isfinite(far_plane)) {
    set_error("need 0 <= near < far < inf");
    return TF_ERR_INVALID;
  }
  for (int i = 0; i < 12; ++i)
    if (!isfinite(pose[i])) { set_error("pose is not finite"); return TF_ERR_INVALID; }
  if (!rgba && !depth && !tri) { set_error("no output"); return TF_ERR_INVALID; }
  if (v->ray_w > 0) *cam = {v->ray_fx, v->ray_fy, v->ray_cx, v->ray_cy, v->ray_w, v->ray_h};
  else *cam = {v->cam.fxi, v->cam.fyi, v->cam.cxi, v->cam.cyi, v->cam.W, v->cam.H};
  if (cam->W <= 0 || cam->H <= 0 || !(cam->fx > 0.f) || !(cam->fy > 0.f)) {
    set_error("no camera (tf_set_camera / tf_raycast_camera)");
    return TF_ERR_INVALID;
  }
  if (mode >= 3 && rgba) {
    if (tex ? (tex_w <= 0 || tex_h <= 0) : (!v->dev.atlas || v->atlas.aw <= 0 || v->atlas.ah <= 0)) {
      set_error(tex ? "texture size must be positive" : "no atlas to sample");
      return TF_ERR_INVALID;
    }
  }
  return TF_OK;
}

// device scratch of one render behind `head` bytes of the caller's own: keys | queue | queue count
struct RenderScratch { size_t o_keys, o_queue, o_cnt; };
RenderScratch render_layout(Layout& L, const RenderCam& cam, size_t ntri) {
  RenderScratch s;
  s.o_keys = L.take(8 * (size_t)cam.W * cam.H);
  s.o_queue = L.take(4 * ntri);
  s.o_cnt = L.take(16);
  return s;
}

int render_launch(tf_volume* v, const RenderCam& cam, const float* d_vtx, int64_t nv, const uint32_t* d_idx, int64_t ni,
                  const uint8_t* d_tex, int tw, int th, const float* pose, float near_plane, float far_plane, int mode,
                  uint8_t* scratch, const RenderScratch& rs, uint8_t* d_rgba, float* d_depth, int32_t* d_tri,
                  const uint32_t* d_counts = nullptr) {
  RenderArgs a;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a.R[3 * r + c] = pose[4 * r + c];
    a.t[r] = pose[4 * r + 3];
  }
  a.fx = cam.fx; a.fy = cam.fy; a.cxs = cam.cx + 0.5f; a.cys = cam.cy + 0.5f;
  a.W = cam.W; a.H = cam.H; a.near_p = near_plane; a.far_p = far_plane; a.mode = mode;
  a.vtx = d_vtx; a.nv = (uint32_t)nv; a.idx = d_idx; a.ntri = (uint32_t)(ni / 3);
  a.tex = d_tex ? d_tex : v->dev.atlas;
  a.tw = d_tex ? tw : v->atlas.aw;
  a.th = d_tex ? th : v->atlas.ah;
  a.keys = reinterpret_cast<unsigned long long*>(scratch + rs.o_keys);
  a.queue = reinterpret_cast<uint32_t*>(scratch + rs.o_queue);
  a.qcount = reinterpret_cast<uint32_t*>(scratch + rs.o_cnt);
  a.counts = d_counts;
  a.rgba = d_rgba; a.depth = d_depth; a.tri = d_tri;
  const size_t P = (size_t)cam.W * cam.H;
  TF_HIP(hipMemsetAsync(a.keys, 0xFF, 8 * P, v->stream));  // kNoKey
  TF_HIP(hipMemsetAsync(a.qcount, 0, 16, v->stream));
  if (a.ntri) {
    hipLaunchKernelGGL(k_render_bin, dim3((a.ntri + 255) / 256), dim3(256), 0, v->stream, a);
    hipLaunchKernelGGL(k_render_large, dim3(std::min(a.ntri, kLargeGrid)), dim3(256), 0, v->stream, a);
  }
  hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, v->stream, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// outputs of a host-form render: staged behind `L`'s earlier blocks, copied out after the launch
struct RenderOut { size_t o_c, o_d, o_t, end; };
RenderOut out_layout(Layout& L, size_t P, bool c, bool d, bool t) {
  RenderOut o;
  o.o_c = L.take(c ? 4 * P : 0); o.o_d = L.take(d ? 4 * P : 0); o.o_t = L.take(t ? 4 * P : 0);
  o.end = L.size;
  return o;
}
int out_fetch(tf_volume* v, const Stage& sg, const RenderOut& o, size_t P, uint8_t* rgba, float* depth, int32_t* tri) {
  TF_HIP(hipMemcpyAsync(sg.h + o.o_c, sg.d + o.o_c, o.end - o.o_c, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (rgba) memcpy(rgba, sg.h + o.o_c, 4 * P);
  if (depth) memcpy(depth, sg.h + o.o_d, 4 * P);
  if (tri) memcpy(tri, sg.h + o.o_t, 4 * P);
  return TF_OK;
}

// The model's stream for a render (tf_model.hip).  Current: no pack, no wait -- the lengths are the host's when it has read
// them, else the capacity with the control block as d_counts.  Not current: the synchronous pack, one wait.
struct ModelView { const float* vtx; const uint32_t* idx; const uint32_t* counts; int64_t nv, ni; };
int model_view(tf_volume* v, ModelView* out) {
  ModelState& m = v->model;
  if (m.packed && m.gen == v->model_gen) ++m.hits;
  else if (const int rc = model_stream_sync(v)) return rc;
  out->vtx = m.vtx.as<float>(); out->idx = m.idx.as<uint32_t>();
  out->counts = m.counted ? nullptr : m.ctl.as<uint32_t>();
  out->nv = m.counted ? m.nv : m.cap_v;
  out->ni = m.counted ? m.ni : m.cap_i - m.cap_i % 3;
  return TF_OK;
}

}  // namespace

extern "C" {

int tf_render_stream_device(tf_volume* v, const float* d_vertices, int64_t n_vertices, const uint32_t* d_indices,
                            int64_t n_indices, const uint8_t* d_texture, int32_t tex_w, int32_t tex_h, const float pose[12],
                            float near_plane, float far_plane, int32_t mode, uint8_t* d_rgba, float* d_depth, int32_t* d_tri) {
  RenderCam cam;
  int rc = render_check(v, n_vertices, n_indices, d_texture, tex_w, tex_h, pose, near_plane, far_plane, mode, d_rgba,
                        d_depth, d_tri, &cam);
  if (rc) return rc;
  if ((n_vertices > 0 && !d_vertices) || (n_indices > 0 && !d_indices)) { set_error("null stream"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  Layout L;
  const RenderScratch rs = render_layout(L, cam, (size_t)(n_indices / 3));
  // (no stage_begin: nothing touches the pool's host half, and the stream orders this render behind every earlier user of
  // the device half -- the pool only waits for the device when it has to grow)
  if ((rc = reserve(v, v->scratch, L.size, 0))) return rc;
  return render_launch(v, cam, d_vertices, n_vertices, d_indices, n_indices, d_texture, tex_w, tex_h, pose, near_plane,
                       far_plane, mode, v->scratch.d.as<uint8_t>(), rs, d_rgba, d_depth, d_tri);
}

int tf_render_stream(tf_volume* v, const float* vertices, int64_t n_vertices, const uint32_t* indices, int64_t n_indices,
                     const uint8_t* texture, int32_t tex_w, int32_t tex_h, const float pose[12], float near_plane,
                     float far_plane, int32_t mode, uint8_t* rgba, float* depth, int32_t* tri) {
  RenderCam cam;
  int rc = render_check(v, n_vertices, n_indices, texture, tex_w, tex_h, pose, near_plane, far_plane, mode, rgba, depth,
                        tri, &cam);
  if (rc) return rc;
  if ((n_vertices > 0 && !vertices) || (n_indices > 0 && !indices)) { set_error("null stream"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const size_t P = (size_t)cam.W * cam.H;
  const size_t bv = 48 * (size_t)n_vertices, bi = 4 * (size_t)n_indices;
  const size_t bt = texture && tex_w > 0 && tex_h > 0 ? 3 * (size_t)tex_w * tex_h : 0;
  // staging: vertices | indices | texture | rgba | depth | tri (both halves), then the device-only scratch
  Layout L;
  const size_t o_v = L.take(bv), o_i = L.take(bi), o_t = L.take(bt);
  const RenderOut ro = out_layout(L, P, rgba, depth, tri);
  const size_t host_bytes = L.size;
  const RenderScratch rs = render_layout(L, cam, (size_t)(n_indices / 3));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, host_bytes, &sg))) return rc;
  if (bv && (rc = stage_in(v, sg, o_v, vertices, bv))) return rc;
  if (bi && (rc = stage_in(v, sg, o_i, indices, bi))) return rc;
  if (bt && (rc = stage_in(v, sg, o_t, texture, bt))) return rc;
  rc = render_launch(v, cam, sg.dp<const float>(o_v), n_vertices, sg.dp<const uint32_t>(o_i), n_indices,
                     bt ? sg.d + o_t : nullptr, tex_w, tex_h, pose, near_plane, far_plane, mode, sg.d, rs,
                     rgba ? sg.d + ro.o_c : nullptr, depth ? sg.dp<float>(ro.o_d) : nullptr,
                     tri ? sg.dp<int32_t>(ro.o_t) : nullptr);
  if (rc) return rc;
  return out_fetch(v, sg, ro, P, rgba, depth, tri);
}

int tf_render_model_device(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t mode,
                           uint8_t* d_rgba, float* d_depth, int32_t* d_tri) {
  RenderCam cam;
  int rc = render_check(v, 0, 0, nullptr, 0, 0, pose, near_plane, far_plane, mode, d_rgba, d_depth, d_tri, &cam);
  if (rc) return rc;
  TF_DEV_READER(v);
  ModelView mv;
  if ((rc = model_view(v, &mv))) return rc;
  Layout L;
  const RenderScratch rs = render_layout(L, cam, (size_t)(mv.ni / 3));
  if ((rc = reserve(v, v->scratch, L.size, 0))) return rc;
  return render_launch(v, cam, mv.vtx, mv.nv, mv.idx, mv.ni, nullptr, 0, 0, pose, near_plane, far_plane, mode,
                       v->scratch.d.as<uint8_t>(), rs, d_rgba, d_depth, d_tri, mv.counts);
}

int tf_render_model(tf_volume* v, const float pose[12], float near_plane, float far_plane, int32_t mode, uint8_t* rgba,
                    float* depth, int32_t* tri) {
  RenderCam cam;
  int rc = render_check(v, 0, 0, nullptr, 0, 0, pose, near_plane, far_plane, mode, rgba, depth, tri, &cam);
  if (rc) return rc;
  TF_DEV_READER(v);
  ModelView mv;
  if ((rc = model_view(v, &mv))) return rc;
  const size_t P = (size_t)cam.W * cam.H;
  Layout L;
  const RenderOut ro = out_layout(L, P, rgba, depth, tri);
  const size_t host_bytes = L.size;
  const RenderScratch rs = render_layout(L, cam, (size_t)(mv.ni / 3));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, host_bytes, &sg))) return rc;
  rc = render_launch(v, cam, mv.vtx, mv.nv, mv.idx, mv.ni, nullptr, 0, 0, pose, near_plane, far_plane, mode,
                     sg.d, rs, rgba ? sg.d + ro.o_c : nullptr, depth ? sg.dp<float>(ro.o_d) : nullptr,
                     tri ? sg.dp<int32_t>(ro.o_t) : nullptr, mv.counts);
  if (rc) return rc;
  return out_fetch(v, sg, ro, P, rgba, depth, tri);
}

}  // extern "C"
