// tf_align_icp_pyramid.hip -- the projective ICP on a depth pyramid: KinectFusion's coarse levels.  A setting of the handle
// (tf_align_icp_set_pyramid), off by default; with it on, a level of stride s = 2^k of a call that raycasts the model
// itself is an image of its own -- W >> k x H >> k block means of the caller's image, with its own camera and its own
// model maps -- handed to the rows kernels as they are (tf_align_icp.hip: k_icp_rows, tf_align_icp_gate.hip: k_gated_rows)
// at stride 1.  This file builds the images and owns the level buffers; the raycasts and the schedule stay in
// tf_align_icp.hip.  tests/align_icp_pyramid_ref.py restates this file.
//
//   k_depth_pyramid    one wave per 8 x 8 tile of level-0 pixels (lane = 8 y + x), one launch for every level a call needs
//                      (up to three): the image is read once, a level comes from the one below by three lane exchanges
//   k_pyramid_spread   tf_align_icp_residuals' level-sized maps spread over the caller's full-size ones
//
// Pixel (X, Y) of level l from a = (2X, 2Y), b = (2X + 1, 2Y), c = (2X, 2Y + 1), d = (2X + 1, 2Y + 1) of level l - 1, all f32,
// every operation rounded on its own (-ffp-contract=off):
//   valid iff each of the four is finite and > 0, and max(a, b, c, d) - min(a, b, c, d) <= max_depth_jump
//   value = ((a + b) + (c + d)) * 0.25f where valid, else 0
// All four or nothing: a mean over the valid ones alone would sit off the block's centre ray.  Level 0 is the caller's
// image, untouched; a level exists where 2^l divides W and H.
// In the wave: the lane's pixel of the level below is v; its block's other three come by __shfl_xor over the horizontal
// partner (lane bit 0, 1, 2 for levels 1, 2, 3), then over the vertical one (lane bit 3, 4, 5) of both.  a + b == b + a and
// (a + b) + (c + d) == (c + d) + (a + b) exactly, so every lane of a block ends with the block's value: level 2 goes on
// among all lanes alike, and the lane whose level-0 pixel is the block's first stores.  Every lane executes every
// exchange; a lane outside the image carries 0, which is "invalid".  No LDS, no atomics, no private memory.
// The level camera (include/tf_fusion.h has the derivation): fx / s, fy / s, (cx + 1) / s - 1, (cy + 1) / s - 1.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include "tf_align_icp_pyramid.h"
#include "tf_devpose.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct PyrArgs {
  const float* depth;
  float *l1, *l2, *l3;  // levels 1 to 3, the first n_levels of them
  int W, H, tiles_x, n_levels;
  float max_jump;
};

__device__ __forceinline__ bool pyr_valid(float z) { return isfinite(z) && z > 0.f; }
// one level up (this file's header): v is the lane's pixel of the level below, bx and by the lane bits of the block's
// horizontal and vertical partner
__device__ __forceinline__ float pyr_up(float v, int bx, int by, float max_jump) {
  const float h = __shfl_xor(v, bx);  // the horizontal pair first
  const float c = __shfl_xor(v, by), d = __shfl_xor(h, by);
  const bool four = pyr_valid(v) && pyr_valid(h) && pyr_valid(c) && pyr_valid(d);
  const float hi = fmaxf(fmaxf(v, h), fmaxf(c, d)), lo = fminf(fminf(v, h), fminf(c, d));
  const float mean = ((v + h) + (c + d)) * 0.25f;
  return (four && hi - lo <= max_jump) ? mean : 0.f;
}

// (resources: tests/test_kernel_resources_align_icp_pyramid.py)
__global__ __launch_bounds__(64) void k_depth_pyramid(PyrArgs a, const tf_device_pose* __restrict__ cell) {
  if (cell && !devpose_ok(cell)) return;  // (uniform: the whole wave leaves)
  const int lane = threadIdx.x;
  const int x = (blockIdx.x % a.tiles_x) * 8 + (lane & 7), y = (blockIdx.x / a.tiles_x) * 8 + (lane >> 3);
  float z = 0.f;
  if (x < a.W && y < a.H) z = a.depth[(size_t)y * a.W + x];
  const float r1 = pyr_up(z, 1, 8, a.max_jump);
  const int W1 = a.W >> 1, H1 = a.H >> 1;
  if (!((x | y) & 1) && (x >> 1) < W1 && (y >> 1) < H1) a.l1[(size_t)(y >> 1) * W1 + (x >> 1)] = r1;
  if (a.n_levels < 2) return;  // (a kernel argument: no lane stays behind)
  const float r2 = pyr_up(r1, 2, 16, a.max_jump);
  const int W2 = a.W >> 2, H2 = a.H >> 2;
  if (!((x | y) & 3) && (x >> 2) < W2 && (y >> 2) < H2) a.l2[(size_t)(y >> 2) * W2 + (x >> 2)] = r2;
  if (a.n_levels < 3) return;
  const float r3 = pyr_up(r2, 4, 32, a.max_jump);
  const int W3 = a.W >> 3, H3 = a.H >> 3;
  if (lane == 0 && (x >> 3) < W3 && (y >> 3) < H3) a.l3[(size_t)(y >> 3) * W3 + (x >> 3)] = r3;
}

struct SpreadArgs {
  const float* lr;
  const uint32_t* lf;
  const int32_t* la;
  float* r;
  uint32_t* flags;
  int32_t* assoc;
  int W, Wk, k;
  size_t n;  // W * H
};
// a lane per pixel of the full-size maps
__global__ __launch_bounds__(256) void k_pyramid_spread(SpreadArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int x = (int)(i % (size_t)a.W), y = (int)(i / (size_t)a.W);
  const bool at = !((x | y) & ((1 << a.k) - 1));
  const size_t o = at ? (size_t)(y >> a.k) * a.Wk + (size_t)(x >> a.k) : 0;  // < Wk * Hk: 2^k divides W and H
  if (a.r) a.r[i] = at ? a.lr[o] : 0.f;
  if (a.flags) a.flags[i] = at ? a.lf[o] : 0u;
  if (a.assoc) a.assoc[i] = at ? a.la[o] : -1;
}

bool pyr_ok(const tf_align_icp_pyramid* p) {
  if (!(p->max_depth_jump > 0.f)) { set_error("align icp pyramid: max_depth_jump must be > 0"); return false; }
  return true;
}

size_t level_pixels(const AlignCam& c, int k) { return (size_t)(c.W >> k) * (size_t)(c.H >> k); }
// where level k >= 1 starts in a buffer that holds levels 1 .. in order, in level pixels
size_t level_offset(const AlignCam& c, int k) {
  size_t o = 0;
  for (int j = 1; j < k; ++j) o += level_pixels(c, j);
  return o;
}

// the launch: levels 1..n_levels of d_depth (of camera c, whose size 2^n_levels divides) into d_out[0..n_levels)
void pyramid_launch(tf_volume* v, const AlignCam& c, const float* d_depth, int n_levels, float max_jump, float* const d_out[3],
                    const tf_device_pose* d_cell) {
  PyrArgs a{};
  a.depth = d_depth;
  a.l1 = d_out[0]; a.l2 = n_levels >= 2 ? d_out[1] : nullptr; a.l3 = n_levels >= 3 ? d_out[2] : nullptr;
  a.W = c.W; a.H = c.H; a.tiles_x = (c.W + 7) / 8; a.n_levels = n_levels;
  a.max_jump = max_jump;
  const unsigned tiles = (unsigned)(a.tiles_x * ((c.H + 7) / 8));
  hipLaunchKernelGGL(k_depth_pyramid, dim3(tiles), dim3(64), 0, v->stream, a, d_cell);
}

// what tf_align_icp_pyramid_depth(_device) refuses a call for
int depth_check(tf_volume* v, const float* depth, int32_t n_levels, const tf_align_icp_pyramid* p, float* const levels[3]) {
  if (!v || !depth || !p || !levels) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n_levels < 1 || n_levels > 3) { set_error("align icp pyramid: n_levels must be 1..3"); return TF_ERR_INVALID; }
  for (int l = 0; l < n_levels; ++l)
    if (!levels[l]) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!pyr_ok(p)) return TF_ERR_INVALID;
  const AlignCam c = align_cam(v);
  if (c.W <= 0 || c.H <= 0) { set_error("no camera (tf_set_camera / tf_raycast_camera)"); return TF_ERR_INVALID; }
  const int m = (1 << n_levels) - 1;
  if ((c.W & m) || (c.H & m)) { set_error("align icp pyramid: 2^n_levels must divide the image's width and height"); return TF_ERR_INVALID; }
  return TF_OK;
}

}  // namespace

bool icp_pyramid_on(const tf_volume* v) { return v->align_icp.pyr_on; }

AlignCam icp_level_cam(const AlignCam& c, int k) {
  const float s = (float)(1 << k);
  return {c.fx / s, c.fy / s, (c.cx + 1.0f) / s - 1.0f, (c.cy + 1.0f) / s - 1.0f, c.W >> k, c.H >> k};
}

int icp_pyramid_check(const tf_volume* v, const tf_align_params& geo, int n_levels) {
  const AlignCam c = align_cam(v);
  for (int l = 0; l < n_levels; ++l) {
    const int s = geo.stride[l];
    if (s != 1 && s != 2 && s != 4 && s != 8) {
      set_error("align icp pyramid: with the pyramid on a stride must be 1, 2, 4 or 8");
      return TF_ERR_INVALID;
    }
    if (c.W % s || c.H % s) {
      set_error("align icp pyramid: a stride does not divide the image's width and height");
      return TF_ERR_INVALID;
    }
  }
  return TF_OK;
}

int icp_pyramid_enqueue(tf_volume* v, const float* d_depth, const tf_align_params& geo, int n_levels,
                        const tf_device_pose* d_cell, IcpLevels* out) {
  AlignIcpState& s = v->align_icp;
  const AlignCam c = align_cam(v);
  IcpLevels L{};
  int top = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int k = __builtin_ctz((unsigned)geo.stride[l]);
    L.used |= 1u << k;
    top = k > top ? k : top;
  }
  L.cam[0] = c;
  L.depth[0] = d_depth;
  if (top > 0) {
    const size_t px = level_offset(c, top + 1);  // pixels of levels 1..top
    int rc = fit(s.pyr_img, 4 * px, v->stream);
    if (rc || (rc = fit(s.pyr_maps, 24 * px, v->stream))) return rc;
    float* lv[3] = {nullptr, nullptr, nullptr};
    for (int k = 1; k <= top; ++k) {
      const size_t o = level_offset(c, k), pk = level_pixels(c, k);
      lv[k - 1] = s.pyr_img.as<float>(4 * o);
      L.cam[k] = icp_level_cam(c, k);
      L.depth[k] = lv[k - 1];
      L.vm[k] = s.pyr_maps.as<float>(24 * o);
      L.nm[k] = s.pyr_maps.as<float>(24 * o + 12 * pk);
    }
    pyramid_launch(v, c, d_depth, top, s.pyr.max_depth_jump, lv, d_cell);
    TF_HIP(hipGetLastError());
  }
  *out = L;
  return TF_OK;
}

int icp_pyramid_residual_maps(tf_volume* v, int k, float** d_r, uint32_t** d_flags, int32_t** d_assoc) {
  AlignIcpState& s = v->align_icp;
  const size_t pk = level_pixels(align_cam(v), k);
  const int rc = fit(s.pyr_res, 12 * pk, v->stream);
  if (rc) return rc;
  *d_r = s.pyr_res.as<float>();
  *d_flags = s.pyr_res.as<uint32_t>(4 * pk);
  *d_assoc = s.pyr_res.as<int32_t>(8 * pk);
  return TF_OK;
}

int icp_pyramid_spread(tf_volume* v, int k, float* d_r, uint32_t* d_flags, int32_t* d_assoc) {
  const AlignIcpState& s = v->align_icp;
  const AlignCam c = align_cam(v);
  const size_t pk = level_pixels(c, k);
  SpreadArgs a{};
  a.lr = s.pyr_res.as<float>(); a.lf = s.pyr_res.as<uint32_t>(4 * pk); a.la = s.pyr_res.as<int32_t>(8 * pk);
  a.r = d_r; a.flags = d_flags; a.assoc = d_assoc;
  a.W = c.W; a.Wk = c.W >> k; a.k = k;
  a.n = (size_t)c.W * (size_t)c.H;
  hipLaunchKernelGGL(k_pyramid_spread, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, v->stream, a);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_align_icp_pyramid_default(tf_align_icp_pyramid* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  out->max_depth_jump = 0.1f;  // tf_align_icp_gate_default's jump
  return TF_OK;
}

int tf_align_icp_set_pyramid(tf_volume* v, const tf_align_icp_pyramid* p) {
  if (!v) { set_error("null argument"); return TF_ERR_INVALID; }
  if (p && !pyr_ok(p)) return TF_ERR_INVALID;
  v->align_icp.pyr_on = p != nullptr;
  v->align_icp.pyr = p ? *p : tf_align_icp_pyramid{};
  return TF_OK;
}

int tf_align_icp_get_pyramid(tf_volume* v, tf_align_icp_pyramid* out, int32_t* on) {
  if (!v || !out || !on) { set_error("null argument"); return TF_ERR_INVALID; }
  *on = v->align_icp.pyr_on ? 1 : 0;
  if (v->align_icp.pyr_on) *out = v->align_icp.pyr;
  else tf_align_icp_pyramid_default(out);
  return TF_OK;
}

int tf_align_icp_pyramid_camera(tf_volume* v, int32_t level, float cam4[4], int32_t* width, int32_t* height) {
  if (!v || !cam4 || !width || !height) { set_error("null argument"); return TF_ERR_INVALID; }
  const AlignCam c = align_cam(v);
  if (c.W <= 0 || c.H <= 0 || !(c.fx > 0.f) || !(c.fy > 0.f)) {
    set_error("no camera (tf_set_camera / tf_raycast_camera)");
    return TF_ERR_INVALID;
  }
  if (level < 0 || level > 3) { set_error("align icp pyramid: level must be 0..3"); return TF_ERR_INVALID; }
  const int m = (1 << level) - 1;
  if ((c.W & m) || (c.H & m)) { set_error("align icp pyramid: 2^level must divide the image's width and height"); return TF_ERR_INVALID; }
  const AlignCam l = icp_level_cam(c, level);
  cam4[0] = l.fx; cam4[1] = l.fy; cam4[2] = l.cx; cam4[3] = l.cy;
  *width = l.W; *height = l.H;
  return TF_OK;
}

int tf_align_icp_pyramid_depth_device(tf_volume* v, const float* d_depth, int32_t n_levels, const tf_align_icp_pyramid* p,
                                      float* const d_levels[3]) {
  const int rc = depth_check(v, d_depth, n_levels, p, d_levels);
  if (rc) return rc;
  TF_DEV_READER(v);
  pyramid_launch(v, align_cam(v), d_depth, n_levels, p->max_depth_jump, d_levels, nullptr);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int tf_align_icp_pyramid_depth(tf_volume* v, const float* depth, int32_t n_levels, const tf_align_icp_pyramid* p,
                               float* const levels[3]) {
  int rc = depth_check(v, depth, n_levels, p, levels);
  if (rc) return rc;
  TF_DEV_READER(v);
  const AlignCam c = align_cam(v);
  const size_t P = (size_t)c.W * (size_t)c.H;
  Layout L;
  const size_t o_d = L.take(4 * P);
  size_t o_l[3] = {0, 0, 0};
  for (int l = 0; l < n_levels; ++l) o_l[l] = L.take(4 * level_pixels(c, l + 1));
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P))) return rc;
  float* d_out[3] = {nullptr, nullptr, nullptr};
  for (int l = 0; l < n_levels; ++l) d_out[l] = sg.dp<float>(o_l[l]);
  pyramid_launch(v, c, sg.dp<const float>(o_d), n_levels, p->max_depth_jump, d_out, nullptr);
  TF_HIP(hipGetLastError());
  if ((rc = stage_out(v, sg, o_l[0], L.size - o_l[0], nullptr))) return rc;
  for (int l = 0; l < n_levels; ++l) memcpy(levels[l], sg.h + o_l[l], 4 * level_pixels(c, l + 1));
  return TF_OK;
}

}  // extern "C"
