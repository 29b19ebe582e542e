// tf_reloc.hip -- relocalising a lost camera against the cached keyframes: small-image retrieval on the device, then
// verification by tf_track_frame as it is.  include/tf_fusion.h defines the descriptor and the score; tf_reloc_score.h
// holds the score's f64 expressions; tests/reloc_ref.py restates both.
//
//   k_reloc_describe  the descriptor blocks of a batch of images (blockIdx.y = image): 1 << lg lanes per block of bw x bh
//                     pixels (lg chosen so that a block of 16 x 16 gets a wave and a block of one pixel a lane), the lanes'
//                     integer sums folded by a butterfly inside the group; G and Z of the block stored by its first lane
//   k_reloc_total     one wave per image: S = the sum of its G (the blocks of an image are spread over workgroups, and this
//                     file has no atomics)
//   k_reloc_score     one wave per indexed row: the three integer sums of the query against the row, the butterfly, the
//                     f64 score by the first lane
//
// Every sum is an integer sum, so no order has to be fixed; nothing is accumulated in floating point.  An image of a
// batch is named by its entry in the device keyframe table, which carries the image pointers and the RGB pixel stride; the
// query's image comes as kernel arguments.  The index is one block (reloc_carve): row r of G and Z for r < cap_rows, the
// query's descriptor as row cap_rows, and behind them what a query downloads, 12 bytes per row.
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tf_devpose.h"
#include "tf_reloc_score.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

constexpr int kRlThreads = 256;

struct RelocDev {
  uint32_t* G;   // [cap_rows + 1][n]
  int32_t* Z;    // [cap_rows + 1][n]
  uint64_t* S;   // [cap_rows + 1]
  uint8_t* out;  // [12 * cap_rows]: f64 score[rows] and behind it i32 m[rows], for the rows there are at the query
};

struct RelocDescArgs {
  const KfDev* tab;     // the keyframe table
  const int2* jobs;     // per image {table entry, row}; null: the image below into row `row`
  const uint8_t* rgb;
  const float* depth;
  int stride, row;
  uint32_t* G;
  int32_t* Z;
  int W, tw, bw, bh, n, lg;
  float min_depth, max_depth;
};
struct RelocTotalArgs {
  const int2* jobs;
  int row, n;
  const uint32_t* G;
  uint64_t* S;
};
struct RelocScoreArgs {
  const uint32_t* G;
  const int32_t* Z;
  int qrow, n_rows, n, bw, bh, min_overlap;
  float grey_weight, depth_weight;
  double* score;
  int32_t* m;
};

// (resources: tests/test_kernel_resources_reloc.py)
__global__ __launch_bounds__(kRlThreads) void k_reloc_describe(RelocDescArgs a) {
  const uint8_t* rgb = a.rgb;
  const float* depth = a.depth;
  int stride = a.stride, row = a.row;
  if (a.jobs) {
    const int2 j = a.jobs[blockIdx.y];
    const KfDev k = a.tab[j.x];
    rgb = k.rgb; depth = k.depth; stride = k.stride; row = j.y;
  }
  const uint32_t L = 1u << a.lg;
  const uint32_t t = blockIdx.x * (uint32_t)kRlThreads + threadIdx.x;
  const uint32_t blk = t >> a.lg, sub = t & (L - 1u);
  const bool in = blk < (uint32_t)a.n;
  const uint32_t npx = (uint32_t)a.bw * (uint32_t)a.bh;
  uint32_t g = 0, c = 0, zs = 0;
  if (in) {
    const uint32_t by = blk / (uint32_t)a.tw, bx = blk - by * (uint32_t)a.tw;
    const size_t o0 = (size_t)(by * (uint32_t)a.bh) * (size_t)a.W + (size_t)(bx * (uint32_t)a.bw);  // the block lies inside W x H
    for (uint32_t p = sub; p < npx; p += L) {
      const uint32_t py = p / (uint32_t)a.bw, px = p - py * (uint32_t)a.bw;
      const size_t o = o0 + (size_t)py * (size_t)a.W + px;
      const float z = depth[o];
      const uint8_t* c3 = rgb + o * (size_t)stride;
      g += 77u * c3[0] + 150u * c3[1] + 29u * c3[2];
      if (isfinite(z) && z >= a.min_depth && z <= a.max_depth) {
        c += 1u;
        zs += (uint32_t)rintf(z * 1000.0f);
      }
    }
  }
  for (uint32_t o = L >> 1; o; o >>= 1) {  // the group's lanes are neighbours in one wave: L divides 64
    g += (uint32_t)__shfl_xor((int)g, (int)o);
    c += (uint32_t)__shfl_xor((int)c, (int)o);
    zs += (uint32_t)__shfl_xor((int)zs, (int)o);
  }
  if (in && sub == 0u) {
    const size_t at = (size_t)row * (size_t)a.n + blk;
    a.G[at] = g;
    a.Z[at] = 2u * c >= npx ? (int32_t)(zs / c) : -1;
  }
}

__global__ __launch_bounds__(64) void k_reloc_total(RelocTotalArgs a) {
  const int row = a.jobs ? a.jobs[blockIdx.x].y : a.row;
  const uint32_t* G = a.G + (size_t)row * (size_t)a.n;
  unsigned long long s = 0ull;
  for (int i = threadIdx.x; i < a.n; i += 64) s += G[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (threadIdx.x == 0) a.S[row] = s;
}

__global__ __launch_bounds__(kRlThreads) void k_reloc_score(RelocScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kRlThreads / 64) + (threadIdx.x >> 6);
  if (row >= a.n_rows) return;  // (the whole wave)
  const uint32_t* Gq = a.G + (size_t)a.qrow * (size_t)a.n;
  const int32_t* Zq = a.Z + (size_t)a.qrow * (size_t)a.n;
  const uint32_t* Gk = a.G + (size_t)row * (size_t)a.n;
  const int32_t* Zk = a.Z + (size_t)row * (size_t)a.n;
  long long sd = 0;
  unsigned long long sd2 = 0ull, sz2 = 0ull;
  uint32_t m = 0;
  for (int i = lane; i < a.n; i += 64) {
    const long long d = (long long)Gq[i] - (long long)Gk[i];
    const unsigned long long ad = (unsigned long long)(d < 0 ? -d : d);
    sd += d;
    sd2 += ad * ad;
    const int32_t zq = Zq[i], zk = Zk[i];
    if (zq >= 0 && zk >= 0) {
      const long long dz = (long long)zq - (long long)zk;
      sz2 += (unsigned long long)(dz * dz);
      m += 1u;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sd += __shfl_xor(sd, o);
    sd2 += __shfl_xor(sd2, o);
    sz2 += __shfl_xor(sz2, o);
    m += (uint32_t)__shfl_xor((int)m, o);
  }
  if (lane == 0) {
    a.score[row] = reloc_score((uint64_t)sd2, (int64_t)sd, (uint64_t)sz2, m, (uint32_t)a.n, (uint32_t)a.bw, (uint32_t)a.bh,
                               a.grey_weight, a.depth_weight, a.min_overlap);
    a.m[row] = (int32_t)m;
  }
}

// the index as it lies in RelocState::block (base == null: its size)
RelocDev reloc_carve(void* base, size_t cap_rows, size_t n, size_t* bytes) {
  RelocDev d{};
  Carver c(base);
  c.take(d.G, (cap_rows + 1) * n);
  c.take(d.Z, (cap_rows + 1) * n);
  c.take(d.S, cap_rows + 1);
  c.take(d.out, 12 * cap_rows + 16);
  if (bytes) *bytes = c.L.size;
  return d;
}

size_t reloc_n(const RelocState& s) { return (size_t)s.p.tiny_w * (size_t)s.p.tiny_h; }
size_t reloc_pixels(const RelocState& s) { return (size_t)s.W * (size_t)s.H; }

// what a configuration is refused for on a camera of W x H
bool reloc_params_ok(const tf_reloc_params& p, int W, int H) {
  if (W <= 0 || H <= 0) { set_error("reloc: no camera (tf_set_camera)"); return false; }
  if (p.tiny_w < 1 || p.tiny_h < 1 || W % p.tiny_w || H % p.tiny_h) {
    set_error("reloc: the camera's " + std::to_string(W) + " x " + std::to_string(H) + " pixels do not divide into " +
              std::to_string(p.tiny_w) + " x " + std::to_string(p.tiny_h) + " blocks");
    return false;
  }
  const double px = (double)(W / p.tiny_w) * (double)(H / p.tiny_h);
  // a block sum of 65280 per pixel stays a u32, and the n squared differences stay below 2^63
  if (px > 65536.0 || (double)W * (double)H * px * 65280.0 * 65280.0 >= 9.2e18) {
    set_error("reloc: blocks too large for the integer sums");
    return false;
  }
  const float f[4] = {p.min_depth, p.max_depth, p.grey_weight, p.depth_weight};
  if (!finite_all(f, 4) || p.min_depth > p.max_depth || p.max_depth > 60.f || p.grey_weight < 0.f || p.depth_weight < 0.f ||
      p.min_overlap < 0) {
    set_error("reloc: need min_depth <= max_depth <= 60, weights >= 0, min_overlap >= 0");
    return false;
  }
  return true;
}

// every call but tf_reloc_configure: configured, and for the camera that is set now
int reloc_ready(tf_volume* v) {
  const RelocState& s = v->reloc;
  if (!s.on) { set_error("reloc: not configured (tf_reloc_configure)"); return TF_ERR_INVALID; }
  if (s.W != v->cam.W || s.H != v->cam.H) {
    set_error("reloc: the camera has changed since tf_reloc_configure");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

bool stride_ok(int32_t stride) {
  if (stride == 3 || stride == 4) return true;
  set_error("rgb_pixel_stride must be 3 or 4");
  return false;
}

// room for `rows` rows; the rows there are move into a larger block
int reloc_ensure(tf_volume* v, size_t rows, RelocDev* d) {
  RelocState& s = v->reloc;
  const size_t n = reloc_n(s);
  if (!s.block || s.cap_rows < rows) {
    size_t cap = s.cap_rows ? s.cap_rows : 64;
    while (cap < rows) cap *= 2;
    size_t bytes = 0;
    reloc_carve(nullptr, cap, n, &bytes);
    DevMem nb;
    const int rc = nb.alloc(bytes);
    if (rc) return rc;
    const size_t have = s.kf_ids.size();
    if (s.block && have) {
      const RelocDev from = reloc_carve(s.block.p, s.cap_rows, n, nullptr), to = reloc_carve(nb.p, cap, n, nullptr);
      TF_HIP(hipMemcpyAsync(to.G, from.G, have * n * 4, hipMemcpyDeviceToDevice, v->stream));
      TF_HIP(hipMemcpyAsync(to.Z, from.Z, have * n * 4, hipMemcpyDeviceToDevice, v->stream));
      TF_HIP(hipMemcpyAsync(to.S, from.S, have * 8, hipMemcpyDeviceToDevice, v->stream));
    }
    if (s.block) TF_HIP(hipStreamSynchronize(v->stream));
    s.block = std::move(nb);
    s.cap_rows = cap;
  }
  *d = reloc_carve(s.block.p, s.cap_rows, n, nullptr);
  return TF_OK;
}

int reloc_lg(const RelocState& s) {
  const size_t npx = reloc_pixels(s) / reloc_n(s);
  int lg = 0;
  while (lg < 6 && ((size_t)1 << lg) < npx) ++lg;
  return lg;
}

RelocDescArgs reloc_desc_args(const tf_volume* v, const RelocDev& d) {
  const RelocState& s = v->reloc;
  RelocDescArgs a{};
  a.tab = v->dev.kf_tab;
  a.stride = 3;
  a.G = d.G; a.Z = d.Z;
  a.W = s.W; a.tw = s.p.tiny_w; a.bw = s.W / s.p.tiny_w; a.bh = s.H / s.p.tiny_h; a.n = (int)reloc_n(s);
  a.lg = reloc_lg(s);
  a.min_depth = s.p.min_depth; a.max_depth = s.p.max_depth;
  return a;
}

// describe + total of n_img images: jobs (device) or the one image of `a` into a.row
void reloc_describe_launch(tf_volume* v, const RelocDev& d, RelocDescArgs a, uint32_t n_img) {
  // n groups of 1 << lg lanes: fewer than 2 W H threads, and reloc_params_ok keeps W H (bw bh) below 2^31.1
  const uint32_t threads = (uint32_t)a.n << a.lg;
  RelocTotalArgs t{a.jobs, a.row, a.n, d.G, d.S};
  constexpr uint32_t kBatch = 32768;  // images per launch (gridDim.y)
  for (uint32_t i0 = 0; i0 < n_img; i0 += kBatch) {
    const uint32_t m = std::min(kBatch, n_img - i0);
    if (a.jobs) { a.jobs += i0 ? kBatch : 0; t.jobs = a.jobs; }
    hipLaunchKernelGGL(k_reloc_describe, dim3((threads + kRlThreads - 1) / kRlThreads, m), dim3(kRlThreads), 0, v->stream, a);
    hipLaunchKernelGGL(k_reloc_total, dim3(m), dim3(64), 0, v->stream, t);
  }
}

struct RelocCand {
  int32_t kf_id, overlap;
  double score;
};

// the query's image (device) described, every row scored, the scores downloaded through the stage at o_out (12 bytes per
// row), one wait, the live rows with a finite score ranked
int reloc_query_run(tf_volume* v, const Stage& sg, size_t o_out, const float* d_depth, const uint8_t* d_rgb, int32_t stride,
                    std::vector<RelocCand>* out) {
  RelocState& s = v->reloc;
  out->clear();
  const size_t rows = s.kf_ids.size();
  if (!rows) return TF_OK;
  RelocDev d;
  int rc = reloc_ensure(v, rows, &d);
  if (rc) return rc;
  RelocDescArgs a = reloc_desc_args(v, d);
  a.rgb = d_rgb; a.depth = d_depth; a.stride = stride; a.row = (int)s.cap_rows;
  reloc_describe_launch(v, d, a, 1);
  RelocScoreArgs sa{};
  sa.G = d.G; sa.Z = d.Z; sa.qrow = (int)s.cap_rows; sa.n_rows = (int)rows; sa.n = a.n; sa.bw = a.bw; sa.bh = a.bh;
  sa.min_overlap = s.p.min_overlap; sa.grey_weight = s.p.grey_weight; sa.depth_weight = s.p.depth_weight;
  sa.score = reinterpret_cast<double*>(d.out);
  sa.m = reinterpret_cast<int32_t*>(d.out + 8 * rows);
  hipLaunchKernelGGL(k_reloc_score, dim3(((uint32_t)rows + 3) / 4), dim3(kRlThreads), 0, v->stream, sa);
  TF_HIP(hipGetLastError());
  TF_HIP(hipMemcpyAsync(sg.h + o_out, d.out, 12 * rows, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  const double* score = sg.hp<double>(o_out);
  const int32_t* m = sg.hp<int32_t>(o_out + 8 * rows);
  const AtlasState& at = v->atlas;
  for (size_t r = 0; r < rows; ++r) {
    const auto it = at.keyframes.find(s.kf_ids[r]);
    if (it == at.keyframes.end() || !it->second.has_pose) continue;  // released since, or no pose yet
    if (!isfinite(score[r])) continue;
    out->push_back({s.kf_ids[r], m[r], score[r]});
  }
  std::sort(out->begin(), out->end(), [](const RelocCand& x, const RelocCand& y) {
    return x.score != y.score ? x.score < y.score : x.kf_id < y.kf_id;
  });
  return TF_OK;
}

// host images staged, then reloc_query_run
int reloc_query_host(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t stride, std::vector<RelocCand>* out) {
  const RelocState& s = v->reloc;
  const size_t P = reloc_pixels(s), rows = s.kf_ids.size();
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take((size_t)stride * P), o_out = L.take(12 * rows + 16);
  Stage sg;
  int rc;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgb, (size_t)stride * P)))
    return rc;
  return reloc_query_run(v, sg, o_out, sg.dp<const float>(o_d), sg.dp<const uint8_t>(o_c), stride, out);
}

int reloc_candidates_out(const std::vector<RelocCand>& c, int32_t* kf_ids, double* scores, int32_t* overlap, int64_t cap,
                         int64_t* n) {
  *n = (int64_t)c.size();
  const int64_t m = std::min<int64_t>(*n, cap);
  for (int64_t i = 0; i < m; ++i) {
    if (kf_ids) kf_ids[i] = c[(size_t)i].kf_id;
    if (scores) scores[i] = c[(size_t)i].score;
    if (overlap) overlap[i] = c[(size_t)i].overlap;
  }
  return TF_OK;
}

// [R^T | -R^T t] of a row-major 4 x 4 [R t; 0 1], in f64, rounded to f32
void rigid_inverse(const float T[16], float pose[12]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) pose[4 * r + c] = T[4 * c + r];
    const double t = ((double)T[r] * (double)T[3] + (double)T[4 + r] * (double)T[7]) + (double)T[8 + r] * (double)T[11];
    pose[4 * r + 3] = (float)-t;
  }
}

}  // namespace

void reloc_release(tf_volume* v) { v->reloc = RelocState{}; }

}  // namespace tf

using namespace tf;

extern "C" {

int tf_reloc_default_params(tf_reloc_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_reloc_params p{};
  p.tiny_w = 40; p.tiny_h = 30;
  p.min_depth = 0.05f; p.max_depth = 5.0f;
  p.grey_weight = 1.0f; p.depth_weight = 2.55e4f;
  p.min_overlap = 40 * 30 / 4;
  *out = p;
  return TF_OK;
}

int tf_reloc_configure(tf_volume* v, const tf_reloc_params* params) {
  if (!v || !params) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!reloc_params_ok(*params, v->cam.W, v->cam.H)) return TF_ERR_INVALID;
  TF_DEV_READER(v);
  RelocState& s = v->reloc;
  if (s.block) TF_HIP(hipStreamSynchronize(v->stream));
  s = RelocState{};
  s.on = true;
  s.p = *params;
  s.W = v->cam.W; s.H = v->cam.H;
  return TF_OK;
}

int tf_reloc_index_add(tf_volume* v, const int32_t* kf_ids, int64_t n) {
  if (!v || n < 0 || (n > 0 && !kf_ids)) { set_error("null argument"); return TF_ERR_INVALID; }
  int rc = reloc_ready(v);
  if (rc) return rc;
  RelocState& s = v->reloc;
  const AtlasState& at = v->atlas;
  const size_t P = reloc_pixels(s);
  for (int64_t i = 0; i < n; ++i) {
    const auto it = at.keyframes.find(kf_ids[i]);
    if (it == at.keyframes.end()) {
      set_error("keyframe " + std::to_string(kf_ids[i]) + " is not cached (tf_keyframe_cache)");
      return TF_ERR_INVALID;
    }
    const KeyframeSlot& ks = it->second;  // the handle's own copies may be those of a smaller camera
    if (ks.rgb && (ks.rgb.bytes < 3 * P || ks.depth.bytes < 4 * P)) {
      set_error("keyframe " + std::to_string(kf_ids[i]) + " was cached for a smaller camera");
      return TF_ERR_INVALID;
    }
  }
  if (!n) return TF_OK;
  TF_DEV_READER(v);
  // rows: the one a keyframe has, or new ones behind the last; an id named twice is described once
  std::vector<int2> jobs;
  std::vector<int32_t> fresh;
  std::unordered_map<int32_t, int32_t> seen;
  for (int64_t i = 0; i < n; ++i) {
    if (!seen.emplace(kf_ids[i], 0).second) continue;
    const auto it = s.row_of.find(kf_ids[i]);
    int row;
    if (it != s.row_of.end()) row = it->second;
    else { row = (int)(s.kf_ids.size() + fresh.size()); fresh.push_back(kf_ids[i]); }
    jobs.push_back(make_int2(at.keyframes.find(kf_ids[i])->second.slot, row));
  }
  RelocDev d;
  if ((rc = reloc_ensure(v, s.kf_ids.size() + fresh.size(), &d))) return rc;
  Stage sg;
  const size_t bytes = jobs.size() * sizeof(int2);
  if ((rc = stage_begin(v, v->scratch, bytes, bytes, &sg)) || (rc = stage_in(v, sg, 0, jobs.data(), bytes))) return rc;
  RelocDescArgs a = reloc_desc_args(v, d);
  a.jobs = sg.dp<const int2>(0);
  reloc_describe_launch(v, d, a, (uint32_t)jobs.size());
  TF_HIP(hipGetLastError());
  for (const int32_t id : fresh) {
    s.row_of[id] = (int32_t)s.kf_ids.size();
    s.kf_ids.push_back(id);
  }
  return TF_OK;
}

int tf_reloc_index_remove(tf_volume* v, const int32_t* kf_ids, int64_t n) {
  if (!v || n < 0 || (n > 0 && !kf_ids)) { set_error("null argument"); return TF_ERR_INVALID; }
  int rc = reloc_ready(v);
  if (rc) return rc;
  TF_DEV_READER(v);
  RelocState& s = v->reloc;
  const size_t nb = reloc_n(s);
  for (int64_t i = 0; i < n; ++i) {
    const auto it = s.row_of.find(kf_ids[i]);
    if (it == s.row_of.end()) continue;
    const size_t row = (size_t)it->second, last = s.kf_ids.size() - 1;
    s.row_of.erase(it);
    if (row != last) {  // the last row moves into the gap (stream order keeps it behind whatever wrote either)
      const RelocDev d = reloc_carve(s.block.p, s.cap_rows, nb, nullptr);
      TF_HIP(hipMemcpyAsync(d.G + row * nb, d.G + last * nb, nb * 4, hipMemcpyDeviceToDevice, v->stream));
      TF_HIP(hipMemcpyAsync(d.Z + row * nb, d.Z + last * nb, nb * 4, hipMemcpyDeviceToDevice, v->stream));
      TF_HIP(hipMemcpyAsync(d.S + row, d.S + last, 8, hipMemcpyDeviceToDevice, v->stream));
      s.kf_ids[row] = s.kf_ids[last];
      s.row_of[s.kf_ids[row]] = (int32_t)row;
    }
    s.kf_ids.pop_back();
  }
  return TF_OK;
}

int tf_reloc_index_clear(tf_volume* v) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  int rc = reloc_ready(v);
  if (rc) return rc;
  v->reloc.kf_ids.clear();
  v->reloc.row_of.clear();
  return TF_OK;
}

int tf_reloc_index_count(tf_volume* v, int64_t* n) {
  if (!v || !n) { set_error("null argument"); return TF_ERR_INVALID; }
  int rc = reloc_ready(v);
  if (rc) return rc;
  *n = (int64_t)v->reloc.kf_ids.size();
  return TF_OK;
}

int tf_reloc_describe(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride, uint32_t* G, int32_t* Z,
                      uint64_t* S) {
  if (!v || !depth || !rgb) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!stride_ok(rgb_pixel_stride)) return TF_ERR_INVALID;
  int rc = reloc_ready(v);
  if (rc) return rc;
  TF_DEV_READER(v);
  RelocState& s = v->reloc;
  const size_t P = reloc_pixels(s), n = reloc_n(s);
  RelocDev d;
  if ((rc = reloc_ensure(v, s.kf_ids.size(), &d))) return rc;
  Layout L;
  const size_t o_d = L.take(4 * P), o_c = L.take((size_t)rgb_pixel_stride * P);
  const size_t o_g = L.take(4 * n), o_z = L.take(4 * n), o_s = L.take(8);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg)) || (rc = stage_in(v, sg, o_d, depth, 4 * P)) ||
      (rc = stage_in(v, sg, o_c, rgb, (size_t)rgb_pixel_stride * P)))
    return rc;
  RelocDescArgs a = reloc_desc_args(v, d);
  a.rgb = sg.dp<const uint8_t>(o_c); a.depth = sg.dp<const float>(o_d); a.stride = rgb_pixel_stride; a.row = (int)s.cap_rows;
  reloc_describe_launch(v, d, a, 1);
  TF_HIP(hipGetLastError());
  const size_t q = s.cap_rows;
  TF_HIP(hipMemcpyAsync(sg.h + o_g, d.G + q * n, 4 * n, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipMemcpyAsync(sg.h + o_z, d.Z + q * n, 4 * n, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipMemcpyAsync(sg.h + o_s, d.S + q, 8, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (G) memcpy(G, sg.h + o_g, 4 * n);
  if (Z) memcpy(Z, sg.h + o_z, 4 * n);
  if (S) memcpy(S, sg.h + o_s, 8);
  return TF_OK;
}

int tf_reloc_descriptor_download(tf_volume* v, int32_t kf_id, uint32_t* G, int32_t* Z, uint64_t* S) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  int rc = reloc_ready(v);
  if (rc) return rc;
  RelocState& s = v->reloc;
  const auto it = s.row_of.find(kf_id);
  if (it == s.row_of.end()) {
    set_error("keyframe " + std::to_string(kf_id) + " is not in the index (tf_reloc_index_add)");
    return TF_ERR_INVALID;
  }
  TF_DEV_READER(v);
  const size_t n = reloc_n(s), row = (size_t)it->second;
  const RelocDev d = reloc_carve(s.block.p, s.cap_rows, n, nullptr);
  Layout L;
  const size_t o_g = L.take(4 * n), o_z = L.take(4 * n), o_s = L.take(8);
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, L.size, &sg))) return rc;
  TF_HIP(hipMemcpyAsync(sg.h + o_g, d.G + row * n, 4 * n, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipMemcpyAsync(sg.h + o_z, d.Z + row * n, 4 * n, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipMemcpyAsync(sg.h + o_s, d.S + row, 8, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  if (G) memcpy(G, sg.h + o_g, 4 * n);
  if (Z) memcpy(Z, sg.h + o_z, 4 * n);
  if (S) memcpy(S, sg.h + o_s, 8);
  return TF_OK;
}

int tf_reloc_query(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride, int32_t* out_kf_ids,
                   double* out_scores, int32_t* out_overlap, int64_t cap, int64_t* n) {
  if (!v || !depth || !rgb || !n || cap < 0) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!stride_ok(rgb_pixel_stride)) return TF_ERR_INVALID;
  int rc = reloc_ready(v);
  if (rc) return rc;
  TF_DEV_READER(v);
  std::vector<RelocCand> c;
  if ((rc = reloc_query_host(v, depth, rgb, rgb_pixel_stride, &c))) return rc;
  return reloc_candidates_out(c, out_kf_ids, out_scores, out_overlap, cap, n);
}

int tf_reloc_query_device(tf_volume* v, const float* d_depth, const uint8_t* d_rgb, int32_t rgb_pixel_stride,
                          int32_t* out_kf_ids, double* out_scores, int32_t* out_overlap, int64_t cap, int64_t* n) {
  if (!v || !d_depth || !d_rgb || !n || cap < 0) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!stride_ok(rgb_pixel_stride)) return TF_ERR_INVALID;
  int rc = reloc_ready(v);
  if (rc) return rc;
  TF_DEV_READER(v);
  const size_t bytes = 12 * v->reloc.kf_ids.size() + 16;
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, bytes, bytes, &sg))) return rc;
  std::vector<RelocCand> c;
  if ((rc = reloc_query_run(v, sg, 0, d_depth, d_rgb, rgb_pixel_stride, &c))) return rc;
  return reloc_candidates_out(c, out_kf_ids, out_scores, out_overlap, cap, n);
}

int tf_relocalise_default_params(tf_relocalise_params* out) {
  if (!out) { set_error("null argument"); return TF_ERR_INVALID; }
  tf_relocalise_params p{};
  p.max_tries = 3;
  p.min_stage = 2;
  p.min_valid_fraction = 0.5f;
  p.max_rms = 0.01f;
  int rc = tf_align_icp_default_params(&p.icp);
  if (rc || (rc = tf_align_default_params(&p.sdf))) return rc;
  *out = p;
  return TF_OK;
}

int tf_relocalise(tf_volume* v, const float* depth, const uint8_t* rgb, int32_t rgb_pixel_stride,
                  const tf_relocalise_params* params, tf_relocalise_result* result) {
  if (!v || !depth || !rgb || !params || !result) { set_error("null argument"); return TF_ERR_INVALID; }
  if (!stride_ok(rgb_pixel_stride)) return TF_ERR_INVALID;
  const tf_relocalise_params& p = *params;
  if (p.max_tries < 1 || p.max_tries > TF_RELOC_MAX_TRIES || p.min_stage < 1 || p.min_stage > 2 ||
      !(p.min_valid_fraction >= 0.f && p.min_valid_fraction <= 1.f) || !(p.max_rms >= 0.f) || !isfinite(p.max_rms)) {
    set_error("relocalise: need max_tries 1..8, min_stage 1..2, min_valid_fraction in [0, 1], max_rms finite and >= 0");
    return TF_ERR_INVALID;
  }
  const float eye[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};  // the tries' poses are finite: checked below
  int rc = track_check(v, depth, eye, &p.icp, &p.sdf);
  if (rc || (rc = reloc_ready(v))) return rc;
  if (v->ray_w > 0 && (v->ray_w != v->cam.W || v->ray_h != v->cam.H)) {
    set_error("relocalise: the raycast camera's size differs from tf_set_camera's");
    return TF_ERR_INVALID;
  }
  std::vector<RelocCand> c;
  {
    TF_DEV_READER(v);
    if ((rc = reloc_query_host(v, depth, rgb, rgb_pixel_stride, &c))) return rc;
  }
  tf_relocalise_result out{};
  out.status = TF_RELOC_NO_CANDIDATE;
  out.kf_id = -1;
  out.rank = -1;
  const AtlasState& at = v->atlas;
  int32_t rank = -1;
  for (const RelocCand& k : c) {
    ++rank;
    if (out.n_tried == p.max_tries) break;
    float pose[12];
    rigid_inverse(at.h_kf[(size_t)at.keyframes.find(k.kf_id)->second.slot].T, pose);
    if (!finite_all(pose, 12)) continue;  // a keyframe with such a pose is no start
    if (out.status == TF_RELOC_NO_CANDIDATE) {
      out.status = TF_RELOC_NOT_FOUND;
      out.kf_id = k.kf_id;
      memcpy(out.pose, pose, sizeof(pose));
    }
    tf_reloc_try& t = out.tries[out.n_tried++];
    t.kf_id = k.kf_id; t.overlap = k.overlap; t.score = k.score;
    if ((rc = tf_track_frame(v, depth, pose, &p.icp, &p.sdf, &t.track))) return rc;
    if (track_accepted(t.track, p.min_stage, p.min_valid_fraction, p.max_rms)) {  // (tf_devpose.h: the device tracker's test too)
      out.status = TF_RELOC_FOUND;
      out.kf_id = k.kf_id;
      out.rank = rank;
      memcpy(out.pose, t.track.pose, sizeof(out.pose));
      break;
    }
  }
  *result = out;
  return TF_OK;
}

}  // extern "C"
