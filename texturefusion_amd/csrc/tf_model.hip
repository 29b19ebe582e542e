// tf_model.hip -- the model's DrawMeshes stream (Structure/Chisel.cpp:288-355), resident in the handle: packed with nothing
// crossing to the host, its counts in device words, kept until the model changes (tf_volume::model_gen).
//
//   k_model_list   every alive chunk whose mesh is in the map and whose patch is complete() -> {chunk key, slot, nv, nt,
//                  DrawPatch flags}, appended in whatever order the atomics hand out; the count stays on the device
//   k_model_rank   the list's ranks in ascending chunk key by comparison counting (k_ccd_rank's shape, the compares of an
//   k_model_place  entry dealt over 16 workgroups), then every entry to its rank.  pack_id biases each axis
//                  by 2^20, so key order is ascending (x, y, z) id order: the order tf_draw_meshes sorts into on the host
//   k_model_scan   one workgroup: exclusive prefix sums of nv and 3 nt in rank order -> the DrawPatch table; the totals
//                  and the verdict on the capacity -> the control block
//   k_model_write  tf_draw_body.h per patch, k_draw's text: workgroups stride over the device-side patch count
//
// The host knows no count: every grid is a function of max_chunks alone, every kernel reads the lengths from the control
// block and clamps them to the capacity of what it indexes.  A model that does not fit writes nothing: the scan leaves
// n_vertices = n_indices = n_patches = 0 and what was needed in need_*, so k_model_write has no patch to stride over and
// the buffers keep what they held.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tf_draw_body.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct ModelEntry {
  unsigned long long key;  // HEntry::key of the chunk (the packed id): what the list is ranked by
  uint32_t slot, nv, nt, flags;
};
struct ModelCtl {
  // what tf_model_stream_get hands out as d_counts
  uint32_t n_vertices, n_indices, n_patches, status, need_vertices, need_indices, zero[2];
  // the pack's own
  uint32_t n_raw;  // patches k_model_list met
  uint32_t pad[7];
};
struct ModelDev {
  ModelCtl* ctl;
  ModelEntry* raw;   // [cap] as listed
  ModelEntry* list;  // [cap] ranked
  uint32_t* rank;    // [cap] position of raw[i] in the ranked list, summed from partial counts
  DrawPatch* rec;    // [cap] ranked, with output positions
  float* vtx;
  uint32_t* idx;
  uint32_t cap;                     // max_chunks
  unsigned long long cap_v, cap_i;  // vertices / indices the buffers hold
  uint32_t sticky;                  // an overflow goes into the volume's status word (the asynchronous form)
};

__global__ __launch_bounds__(256) void k_model_list(VolumeDev v, ModelDev m) {
  const uint32_t nent = v.hmask + 1u;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nent; i += gridDim.x * 256) {
    const HEntry h = v.hent[i];
    if (h.key == kEmptyKey || !(h.alive & 1u) || h.slot == kInvalidSlot) continue;
    const MeshRec r = v.mesh_rec[h.slot];
    if (!(r.state & kMsInMap) || !(r.pflags & kPfHasPatch) || !draw_complete(r.nv, r.state, r.pflags, r.frameid)) continue;
    const uint32_t p = atomicAdd(&m.ctl->n_raw, 1u);
    if (p >= m.cap) continue;
    ModelEntry e;
    e.key = h.key; e.slot = h.slot; e.nv = r.nv; e.nt = r.nt; e.flags = draw_flags(r.pflags);
    m.raw[p] = e;
  }
}

// entry i goes to position #{j : key_j < key_i}; keys are distinct (one hash entry per chunk).  Tiles of 256 keys through LDS.
// The compares of one entry are dealt over gridDim.y workgroups (workgroup y takes the key tiles y, y + gridDim.y, ...) and
// their partial counts are added up in rank[i] (zeroed before the launch; integer atomics: the sum does not depend on
// their order): with the whole list on one lane, ceil(n / 256) workgroups walked n keys each and the rank was 81 % of the
// pack.  k_model_place then moves every entry to its rank.
__global__ __launch_bounds__(256) void k_model_rank(ModelDev m) {
  __shared__ unsigned long long tile[256];
  const uint32_t n = min(m.ctl->n_raw, m.cap);
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const unsigned long long key = i < n ? m.raw[i].key : 0ull;
    uint32_t rank = 0;
    for (uint32_t t0 = blockIdx.y * 256u; t0 < n; t0 += gridDim.y * 256u) {
      __syncthreads();
      const uint32_t j = t0 + threadIdx.x;
      if (j < n) tile[threadIdx.x] = m.raw[j].key;
      __syncthreads();
      const uint32_t c = min(256u, n - t0);
      for (uint32_t k = 0; k < c; ++k) rank += (uint32_t)(tile[k] < key);
    }
    if (i < n && rank) atomicAdd(&m.rank[i], rank);
  }
}
__global__ __launch_bounds__(256) void k_model_place(ModelDev m) {
  const uint32_t n = min(m.ctl->n_raw, m.cap);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t r = m.rank[i];
    if (r < n) m.list[r] = m.raw[i];
  }
}

// Thread t takes the ranks [t per, (t + 1) per): its own sums, an exclusive scan of the 1024 sums (wave scan + the 16 wave
// totals through LDS), then its ranks again with the running positions.
__global__ __launch_bounds__(1024) void k_model_scan(VolumeDev v, ModelDev m) {
  __shared__ unsigned long long wv[16], wi[16];
  const uint32_t n = min(m.ctl->n_raw, m.cap);
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t b = min(t * per, n), e = min(b + per, n);
  unsigned long long sv = 0, si = 0;
  for (uint32_t i = b; i < e; ++i) { sv += m.list[i].nv; si += 3ull * m.list[i].nt; }
  unsigned long long iv = sv, ii = si;  // inclusive over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long pv = __shfl_up(iv, o), pi = __shfl_up(ii, o);
    if (lane >= (uint32_t)o) { iv += pv; ii += pi; }
  }
  if (lane == 63u) { wv[w] = iv; wi[w] = ii; }
  __syncthreads();
  unsigned long long bv = 0, bi = 0, tv = 0, ti = 0;
  for (uint32_t k = 0; k < 16u; ++k) {
    if (k < w) { bv += wv[k]; bi += wi[k]; }
    tv += wv[k]; ti += wi[k];
  }
  unsigned long long vout = bv + iv - sv, iout = bi + ii - si;
  for (uint32_t i = b; i < e; ++i) {
    const ModelEntry en = m.list[i];
    DrawPatch P;
    P.slot = en.slot; P.nv = en.nv; P.nt = en.nt; P.flags = en.flags; P.vout = vout; P.iout = iout;
    m.rec[i] = P;
    vout += en.nv; iout += 3ull * en.nt;
  }
  if (t == 0) {
    const bool fits = tv <= m.cap_v && ti <= m.cap_i;
    ModelCtl* c = m.ctl;
    c->n_vertices = fits ? (uint32_t)tv : 0u;
    c->n_indices = fits ? (uint32_t)ti : 0u;
    c->n_patches = fits ? n : 0u;
    c->status = fits ? 0u : kStModelFull;
    c->need_vertices = (uint32_t)min(tv, 0xFFFFFFFFull);
    c->need_indices = (uint32_t)min(ti, 0xFFFFFFFFull);
    c->zero[0] = 0u; c->zero[1] = 0u;
    if (!fits && m.sticky) atomicOr(&v.vctl->status, kStModelFull);
  }
}

__global__ __launch_bounds__(256) void k_model_write(VolumeDev v, ModelDev m) {
  const uint32_t n = min(m.ctl->n_patches, m.cap);
  for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
    const DrawPatch P = m.rec[p];
    if (P.vout + P.nv > m.cap_v || P.iout + 3ull * P.nt > m.cap_i) continue;  // (the scan let nothing through that does not fit)
    draw_patch_body(v, P, m.vtx, m.idx);
  }
}

constexpr unsigned kModelGrid = 1024;
constexpr unsigned kModelRankSplit = 16;  // workgroups that share the compares of one tile of entries

// list / rank / records / control block: first use (a handle that never comes here holds none of this)
int model_ensure(tf_volume* v) {
  ModelState& m = v->model;
  if (m.ctl) return TF_OK;
  const size_t mc = v->dev.max_chunks;
  int rc;
  if ((rc = m.list.alloc(2 * mc * sizeof(ModelEntry))) || (rc = m.rank.alloc(mc * sizeof(uint32_t))) ||
      (rc = m.rec.alloc(mc * sizeof(DrawPatch))) ||
      (rc = m.h_ctl.alloc(32)) || (rc = m.ctl.alloc(sizeof(ModelCtl))))
    return rc;
  TF_HIP(hipMemsetAsync(m.ctl.p, 0, sizeof(ModelCtl), v->stream));
  return TF_OK;
}

// the stream buffers at exactly this capacity; what they held is gone
int model_capacity(tf_volume* v, int64_t cap_v, int64_t cap_i) {
  ModelState& m = v->model;
  int rc = model_ensure(v);
  if (rc) return rc;
  if (m.vtx && cap_v == m.cap_v && cap_i == m.cap_i) return TF_OK;
  if (m.vtx) TF_HIP(hipStreamSynchronize(v->stream));  // launches on it may still read or write the old buffers
  m.packed = false;
  m.cap_v = m.cap_i = 0;
  if ((rc = m.vtx.alloc(std::max<size_t>((size_t)cap_v * 48, 48))) || (rc = m.idx.alloc(std::max<size_t>((size_t)cap_i * 4, 16)))) {
    m.vtx.release(); m.idx.release();
    return rc;
  }
  m.cap_v = cap_v; m.cap_i = cap_i;
  return TF_OK;
}

ModelDev model_dev(const tf_volume* v, bool sticky) {
  const ModelState& m = v->model;
  ModelDev d;
  d.ctl = m.ctl.as<ModelCtl>();
  d.raw = m.list.as<ModelEntry>();
  d.list = d.raw + v->dev.max_chunks;
  d.rank = m.rank.as<uint32_t>();
  d.rec = m.rec.as<DrawPatch>();
  d.vtx = m.vtx.as<float>(); d.idx = m.idx.as<uint32_t>();
  d.cap = v->dev.max_chunks;
  d.cap_v = (unsigned long long)m.cap_v; d.cap_i = (unsigned long long)m.cap_i;
  d.sticky = sticky ? 1u : 0u;
  return d;
}

// ev: null, or five events recorded around the four stages
int pack_enqueue(tf_volume* v, bool sticky, hipEvent_t* ev) {
  ModelState& m = v->model;
  const ModelDev d = model_dev(v, sticky);
  hipStream_t s = v->stream;
  const size_t mc = v->dev.max_chunks;
  const unsigned rank_grid = (unsigned)std::min<size_t>(std::max<size_t>((mc + 255) / 256, 1), kModelGrid);
  TF_HIP(hipMemsetAsync(&d.ctl->n_raw, 0, 4, s));
  if (ev) TF_HIP(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_model_list, dim3(kModelGrid), dim3(256), 0, s, v->dev, d);
  if (ev) TF_HIP(hipEventRecord(ev[1], s));
  TF_HIP(hipMemsetAsync(d.rank, 0, mc * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_model_rank, dim3(rank_grid, kModelRankSplit), dim3(256), 0, s, d);
  hipLaunchKernelGGL(k_model_place, dim3(rank_grid), dim3(256), 0, s, d);
  if (ev) TF_HIP(hipEventRecord(ev[2], s));
  hipLaunchKernelGGL(k_model_scan, dim3(1), dim3(1024), 0, s, v->dev, d);
  if (ev) TF_HIP(hipEventRecord(ev[3], s));
  hipLaunchKernelGGL(k_model_write, dim3(kModelGrid), dim3(256), 0, s, v->dev, d);
  if (ev) TF_HIP(hipEventRecord(ev[4], s));
  TF_HIP(hipGetLastError());
  m.packed = true; m.gen = v->model_gen; m.counted = false;
  ++m.packs;
  return TF_OK;
}

}  // namespace

void model_release(tf_volume* v) {
  const uint64_t packs = v->model.packs, hits = v->model.hits;  // (the counters are the handle's, not the buffers')
  v->model = ModelState{};
  v->model.packs = packs; v->model.hits = hits;
}

int model_pack_enqueue(tf_volume* v) { return pack_enqueue(v, true, nullptr); }

int model_stream_sync(tf_volume* v) {
  ModelState& m = v->model;
  int rc = model_ensure(v);
  if (rc) return rc;
  if (!m.vtx && (rc = model_capacity(v, 1 << 16, 3 << 16))) return rc;
  for (int pass = 0; pass < 2; ++pass) {
    if ((rc = pack_enqueue(v, false, nullptr))) return rc;
    TF_HIP(hipMemcpyAsync(m.h_ctl.p, m.ctl.p, 32, hipMemcpyDeviceToHost, v->stream));
    TF_HIP(hipStreamSynchronize(v->stream));
    const uint32_t* c = m.h_ctl.as<uint32_t>();
    if (!c[3]) {
      m.counted = true; m.nv = c[0]; m.ni = c[1];
      return TF_OK;
    }
    int64_t cv = 1 << 16, ci = 3 << 16;  // grown to a power of two
    while (cv < (int64_t)c[4]) cv <<= 1;
    while (ci < (int64_t)c[5]) ci <<= 1;
    if ((rc = model_capacity(v, std::max(cv, m.cap_v), std::max(ci, m.cap_i)))) return rc;
  }
  set_error("model stream: the model grew between two packs");
  return TF_ERR_CAPACITY;
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_model_stream_reserve(tf_volume* v, int64_t cap_vertices, int64_t cap_indices) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  if (cap_vertices < 0 || cap_indices < 0 || cap_vertices > 0x7FFFFFFFll || cap_indices > 0xFFFFFFFFll) {
    set_error("model stream capacity out of range");
    return TF_ERR_INVALID;
  }
  TF_DEV_READER(v);
  ModelState& m = v->model;
  if (m.packed && m.gen == v->model_gen) {  // never below a stream that is current
    cap_vertices = std::max(cap_vertices, m.counted ? m.nv : m.cap_v);
    cap_indices = std::max(cap_indices, m.counted ? m.ni : m.cap_i);
  }
  return model_capacity(v, cap_vertices, cap_indices);
}

int tf_model_stream_update_device(tf_volume* v) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!v->model.vtx) { set_error("model stream has no capacity (tf_model_stream_reserve / tf_model_stream_update)"); return TF_ERR_INVALID; }
  return model_pack_enqueue(v);
}

int tf_model_stream_update(tf_volume* v, int64_t* n_vertices, int64_t* n_indices) {
  if (n_vertices) *n_vertices = 0;
  if (n_indices) *n_indices = 0;
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  const int rc = model_stream_sync(v);
  if (rc) return rc;
  if (n_vertices) *n_vertices = v->model.nv;
  if (n_indices) *n_indices = v->model.ni;
  return TF_OK;
}

int tf_model_stream_get(tf_volume* v, const float** d_vertices, const uint32_t** d_indices, const uint32_t** d_counts,
                        int64_t* cap_vertices, int64_t* cap_indices) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  const ModelState& m = v->model;  // (host state only: no device is bound, nothing is flushed, the generation stays)
  if (!m.vtx) { set_error("no model stream (tf_model_stream_reserve / tf_model_stream_update)"); return TF_ERR_INVALID; }
  if (d_vertices) *d_vertices = m.vtx.as<const float>();
  if (d_indices) *d_indices = m.idx.as<const uint32_t>();
  if (d_counts) *d_counts = m.ctl.as<const uint32_t>();
  if (cap_vertices) *cap_vertices = m.cap_v;
  if (cap_indices) *cap_indices = m.cap_i;
  return TF_OK;
}

int tf_model_stream_stats(tf_volume* v, int64_t out[4]) {
  if (!v || !out) { set_error("null argument"); return TF_ERR_INVALID; }
  const ModelState& m = v->model;
  out[0] = (int64_t)m.packs; out[1] = (int64_t)m.hits; out[2] = m.cap_v; out[3] = m.cap_i;
  return TF_OK;
}

int tf_model_stream_release(tf_volume* v) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  TF_HIP(hipStreamSynchronize(v->stream));  // launches on it may still use the buffers
  model_release(v);
  return TF_OK;
}

int tf_model_stream_time(tf_volume* v, double us[4]) {
  if (!v || !us) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV_READER(v);
  if (!v->model.vtx) { set_error("model stream has no capacity (tf_model_stream_reserve / tf_model_stream_update)"); return TF_ERR_INVALID; }
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = TF_OK;
  for (int k = 0; k < 5 && !rc; ++k)
    if (hipEventCreate(&ev[k]) != hipSuccess) { set_error("hipEventCreate failed"); rc = TF_ERR_HIP; }
  if (!rc) rc = pack_enqueue(v, false, ev);  // (not sticky: a timing run on too small a buffer leaves the status word alone)
  if (!rc && hipStreamSynchronize(v->stream) != hipSuccess) { set_error("hipStreamSynchronize failed"); rc = TF_ERR_HIP; }
  for (int k = 0; k < 4 && !rc; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) != hipSuccess) { set_error("hipEventElapsedTime failed"); rc = TF_ERR_HIP; }
    us[k] = 1000.0 * (double)ms;
  }
  for (int k = 0; k < 5; ++k)
    if (ev[k]) hipEventDestroy(ev[k]);
  return rc;
}

}  // extern "C"
