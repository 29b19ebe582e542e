// tf_cc.hip -- Chisel::CompensateColor (Structure/Chisel.cpp:198-286) with nothing crossing to the host: the patch list,
// the clusters, both reductions, the per-cluster solve and the transfer all stay on the handle's stream.
//
//   k_ccd_list        every mesh of the map that has a patch without has_adjusted -> {chunk key, slot, nv, frameid, wrong},
//                     appended in whatever order the atomics hand out; the count stays on the device
//   k_ccd_rank        the list in ascending chunk key by comparison counting (k_tm_rank's shape); clears as much of the
//                     cluster table as this list needs
//   k_ccd_cluster     open-addressing table keyed by frame id; a cluster is named by the smallest rank among its patches
//   k_ccd_partial<P>  one wave per patch: sums (P = 0) / centred second moments (P = 1) over its vertices, f64, lane-strided
//                     in vertex order + a fixed butterfly
//   k_ccd_combine<P>  one wave per cluster: its patches' partial sums in rank order -> means (P = 0) / covariances and the
//                     transfer matrix, solved by lane 0 (P = 1)
//   k_ccd_apply       one wave per patch: labs = T (texcolor - mean_src) + mean_tar, has_adjusted
//
// Reproducible: every sum is taken in an order that is a function of the SET of patches (rank = position by chunk key,
// vertices by index, lanes by a fixed butterfly); the order in which k_ccd_list's atomics handed out positions and the
// slot a frame id found in the table only decide where a value is stored, never what is added to what.
// The host knows no count: every grid is a function of max_chunks alone (1024 workgroups; k_ccd_rank and k_ccd_cluster
// min(ceil(max_chunks / 256), 1024), both grid-stride), every kernel reads the list's length from the control block and
// clamps it to the capacity of the buffer it indexes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "tf_cc_solve.h"
#include "tf_device.h"
#include "tf_volume.h"

#pragma clang fp contract(off)

namespace tf {
namespace {

struct CcdEntry {
  unsigned long long key;  // HEntry::key of the chunk (the packed id): what the list is ranked by
  uint32_t slot;
  uint32_t nvw;            // vertices | wrong_mapping << 31
  int32_t frameid;
  uint32_t cluster;        // rank of the first patch of its cluster (k_ccd_partial<0>), ~0 = none
};
struct CcdCtl {
  uint32_t n_raw;       // patches k_ccd_list met (may exceed the capacity)
  uint32_t n;           // min(n_raw, capacity): the ranked list's length
  uint32_t n_clusters;
  uint32_t tmask;       // the part of the table this list uses, minus one (a power of two >= 2 n)
  uint32_t n_out;       // tf_compensate_color_device_count: the word it hands the call as d_n_clusters
  uint32_t pad[3];
};
struct CcdCluster {
  float X[16];  // T[9], mean_src[3], mean_tar[3], learnt (k_cc_apply's record)
  float cnt;    // vertices of the patches that are not wrongly mapped
  float pad[3];
};
struct CcdDev {
  CcdCtl* ctl;
  CcdEntry* raw;    // [cap] as listed (lies in `part`: read by k_ccd_rank only, before any partial sum is written)
  CcdEntry* list;   // [cap] ranked
  double* part;     // [cap][12] per patch
  CcdCluster* clus; // [cap] by the cluster's name
  unsigned long long* tkey;  // [tab_cap] (uint32_t)frameid, ~0 = free
  uint32_t* trep;            // [tab_cap] smallest rank that carries the key
  uint32_t cap, tab_cap;
};
constexpr unsigned long long kCcdFree = ~0ull;
constexpr uint32_t kCcdGrid = 1024;  // workgroups of the wave-per-patch kernels: 4096 waves, one resident round of the part

__device__ __forceinline__ uint32_t ccd_hash(const unsigned long long k) { return (uint32_t)k * 2654435761u >> 7; }
__device__ __forceinline__ uint32_t ccd_len(const CcdDev& c) { return min(c.ctl->n, c.cap); }
__device__ __forceinline__ uint32_t ccd_tmask(const CcdDev& c) { return min(c.ctl->tmask, c.tab_cap - 1u); }
// the cluster of a frame id: the smallest rank among its patches; ~0 if the id is not in the table
__device__ __forceinline__ uint32_t ccd_rep(const CcdDev& c, const int32_t frameid, const uint32_t tmask) {
  const unsigned long long k = (uint32_t)frameid;
  uint32_t h = ccd_hash(k) & tmask;
  for (uint32_t probe = 0; probe <= tmask; ++probe, h = (h + 1u) & tmask) {
    const unsigned long long t = c.tkey[h];
    if (t == k) return c.trep[h];
    if (t == kCcdFree) break;
  }
  return ~0u;
}
template <int N>
__device__ __forceinline__ void ccd_wave_sum(double (&a)[N]) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] += __shfl_xor(a[i], o);
}

__global__ __launch_bounds__(256) void k_ccd_list(VolumeDev v, CcdDev c) {
  const uint32_t nent = v.hmask + 1u;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nent; i += gridDim.x * 256) {
    const HEntry h = v.hent[i];
    if (h.key == kEmptyKey || !(h.alive & 1u) || h.slot == kInvalidSlot) continue;
    const MeshRec m = v.mesh_rec[h.slot];
    if (!(m.state & kMsInMap) || !(m.pflags & kPfHasPatch) || (m.pflags & kPfAdjusted)) continue;  // Chisel.cpp:203
    const uint32_t p = atomicAdd(&c.ctl->n_raw, 1u);
    if (p >= c.cap) continue;
    CcdEntry e;
    e.key = h.key; e.slot = h.slot; e.nvw = (uint32_t)m.nv | ((m.pflags & kPfWrong) ? 0x80000000u : 0u);
    e.frameid = m.frameid; e.cluster = ~0u;
    c.raw[p] = e;
  }
}

// entry i goes to position #{j : key_j < key_i}; keys are distinct (one hash entry per chunk).  Tiles of 256 keys through LDS.
__global__ __launch_bounds__(256) void k_ccd_rank(CcdDev c) {
  __shared__ unsigned long long tile[256];
  const uint32_t n = min(c.ctl->n_raw, c.cap);
  uint32_t tcap = 64u;
  while (tcap < c.tab_cap && tcap < 2u * n) tcap <<= 1;
  if (blockIdx.x == 0 && threadIdx.x == 0) { c.ctl->n = n; c.ctl->tmask = tcap - 1u; }
  for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < tcap; j += gridDim.x * 256u) { c.tkey[j] = kCcdFree; c.trep[j] = ~0u; }
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    CcdEntry e{};
    if (i < n) e = c.raw[i];
    uint32_t rank = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {
      __syncthreads();
      const uint32_t j = t0 + threadIdx.x;
      if (j < n) tile[threadIdx.x] = c.raw[j].key;
      __syncthreads();
      const uint32_t m = min(256u, n - t0);
      for (uint32_t k = 0; k < m; ++k) rank += (uint32_t)(tile[k] < e.key);
    }
    if (i < n && rank < n) c.list[rank] = e;
  }
}

__global__ __launch_bounds__(256) void k_ccd_cluster(CcdDev c) {
  const uint32_t n = ccd_len(c), tmask = ccd_tmask(c);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const unsigned long long k = (uint32_t)c.list[i].frameid;
    uint32_t h = ccd_hash(k) & tmask;
    for (uint32_t probe = 0; probe <= tmask; ++probe, h = (h + 1u) & tmask) {  // (the table has at least n free entries)
      const unsigned long long old = atomicCAS(&c.tkey[h], kCcdFree, k);
      if (old == kCcdFree || old == k) { atomicMin(&c.trep[h], i); break; }
    }
  }
}

// computeMeanAndCov (Patch.cpp:342-348) over one patch: pass 0 the sums of texcolor / mesh colour -> part[i][0..5], pass 1 the
// centred second moments (6 unique entries each, every term rounded to f32 as the reference forms it) -> part[i][0..11]
template <int PASS>
__global__ __launch_bounds__(256) void k_ccd_partial(VolumeDev v, CcdDev c) {
  constexpr int NV = PASS == 0 ? 6 : 12;
  const uint32_t n = ccd_len(c), tmask = ccd_tmask(c);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
    const CcdEntry e = c.list[i];
    uint32_t rep = e.cluster;
    if constexpr (PASS == 0) {
      rep = ccd_rep(c, e.frameid, tmask);
      if (lane == 0) {
        c.list[i].cluster = rep;
        if (rep == i) atomicAdd(&c.ctl->n_clusters, 1u);
      }
    }
    if ((e.nvw >> 31) || rep >= n) continue;  // wrongly mapped: no part of the statistics (Chisel.cpp:226)
    const uint32_t nv = e.nvw, blk = v.mesh_rec[e.slot].block;
    float m[6] = {0, 0, 0, 0, 0, 0};
    if constexpr (PASS == 1)
#pragma unroll
      for (int a = 0; a < 6; ++a) m[a] = c.clus[rep].X[9 + a];
    double acc[NV];
#pragma unroll
    for (int a = 0; a < NV; ++a) acc[a] = 0.0;
    for (uint32_t k = lane; k < nv; k += 64u) {
      const float s0 = mesh_plane(v, blk, kMpTcol)[k], s1 = mesh_plane(v, blk, kMpTcol + 1)[k],
                  s2 = mesh_plane(v, blk, kMpTcol + 2)[k];
      const float t0 = mesh_plane(v, blk, kMpCol)[k], t1 = mesh_plane(v, blk, kMpCol + 1)[k],
                  t2 = mesh_plane(v, blk, kMpCol + 2)[k];
      if constexpr (PASS == 0) {
        acc[0] += (double)s0; acc[1] += (double)s1; acc[2] += (double)s2;
        acc[3] += (double)t0; acc[4] += (double)t1; acc[5] += (double)t2;
      } else {
        const float a = s0 - m[0], b = s1 - m[1], d = s2 - m[2];
        const float f = t0 - m[3], g = t1 - m[4], h = t2 - m[5];
        acc[0] += (double)(a * a); acc[1] += (double)(a * b); acc[2] += (double)(a * d);
        acc[3] += (double)(b * b); acc[4] += (double)(b * d); acc[5] += (double)(d * d);
        acc[6] += (double)(f * f); acc[7] += (double)(f * g); acc[8] += (double)(f * h);
        acc[9] += (double)(g * g); acc[10] += (double)(g * h); acc[11] += (double)(h * h);
      }
    }
    ccd_wave_sum(acc);
    if (lane < (uint32_t)NV) {
      double mine = acc[0];
#pragma unroll
      for (int a = 1; a < NV; ++a) mine = lane == (uint32_t)a ? acc[a] : mine;
      c.part[(size_t)i * 12u + lane] = mine;
    }
  }
}

// One wave per cluster (the wave of the cluster's first patch): the partial sums of its patches in rank order, lane l
// taking ranks first + l, first + l + 64, ...  Pass 0 leaves the means and the vertex count; pass 1 the covariances
// (divisor N - 1) and, by lane 0, the transfer of Chisel.cpp:250-268.
template <int PASS>
__global__ __launch_bounds__(256) void k_ccd_combine(CcdDev c, uint32_t* __restrict__ out_n_clusters) {
  constexpr int NV = PASS == 0 ? 6 : 12;
  const uint32_t n = ccd_len(c);
  const uint32_t lane = threadIdx.x & 63u;
  if (PASS == 1 && out_n_clusters && blockIdx.x == 0 && threadIdx.x == 0) *out_n_clusters = c.ctl->n_clusters;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
    if (c.list[i].cluster != i) continue;
    double acc[NV];
#pragma unroll
    for (int a = 0; a < NV; ++a) acc[a] = 0.0;
    uint32_t cnt = 0;
    for (uint32_t j = i + lane; j < n; j += 64u) {
      const CcdEntry e = c.list[j];
      if (e.cluster != i || (e.nvw >> 31)) continue;
      cnt += e.nvw;
#pragma unroll
      for (int a = 0; a < NV; ++a) acc[a] += c.part[(size_t)j * 12u + a];
    }
    ccd_wave_sum(acc);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane != 0) continue;
    CcdCluster& C = c.clus[i];
    if constexpr (PASS == 0) {
      const float fc = (float)cnt;
      C.cnt = fc;
#pragma unroll
      for (int a = 0; a < 9; ++a) C.X[a] = 0.0f;
#pragma unroll
      for (int a = 0; a < 6; ++a) C.X[9 + a] = cnt ? (float)(acc[a] / (double)cnt) : 0.0f;
      C.X[15] = 0.0f;
    } else {
      const float fc = C.cnt;
      if (fc <= 0.0f) continue;  // Chisel.cpp:242: empty cluster, has_adjusted stays false
      const double nm1 = (double)(fc - 1.0f);
      float cs[9], ct[9], T[9];
      constexpr int idx[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
#pragma unroll
      for (int a = 0; a < 9; ++a) { cs[a] = (float)(acc[idx[a]] / nm1); ct[a] = (float)(acc[6 + idx[a]] / nm1); }
      color_transfer(cs, ct, T);
#pragma unroll
      for (int a = 0; a < 9; ++a) C.X[a] = T[a];
      C.X[15] = 1.0f;
    }
  }
}

// labs[k] = T (texcolor[k] - mean_src) + mean_tar (Chisel.cpp:274); has_adjusted = true (:280)
__global__ __launch_bounds__(256) void k_ccd_apply(VolumeDev v, CcdDev c) {
  const uint32_t n = ccd_len(c);
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
    const CcdEntry e = c.list[i];
    if (e.cluster >= n) continue;
    const float* X = c.clus[e.cluster].X;
    if (X[15] == 0.0f) continue;  // nothing was learnt for this cluster (:242): has_adjusted stays false
    if (lane == 0) v.mesh_rec[e.slot].pflags |= kPfAdjusted;
    if (e.nvw >> 31) continue;  // labs cleared (:277-279)
    const uint32_t nv = e.nvw, blk = v.mesh_rec[e.slot].block;
    for (uint32_t k = lane; k < nv; k += 64u) {
      const float d0 = mesh_plane(v, blk, kMpTcol)[k] - X[9], d1 = mesh_plane(v, blk, kMpTcol + 1)[k] - X[10],
                  d2 = mesh_plane(v, blk, kMpTcol + 2)[k] - X[11];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float s = X[3 * a] * d0;
        s = s + X[3 * a + 1] * d1;
        s = s + X[3 * a + 2] * d2;
        mesh_plane(v, blk, kMpLabs + a)[k] = s + X[12 + a];
      }
    }
  }
}

// the buffers in the order they lie in the handle's one block (base == null: the block's size)
CcdDev cc_carve(void* base, size_t max_chunks, size_t* bytes) {
  CcdDev c{};
  size_t tab = 64;
  while (tab < 2 * max_chunks) tab <<= 1;
  c.cap = (uint32_t)max_chunks;
  c.tab_cap = (uint32_t)tab;
  Layout L;
  uint8_t* b = static_cast<uint8_t*>(base);
  const auto take = [&](auto*& p, size_t count) {
    const size_t at = L.take(count * sizeof(*p));
    p = b ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(b + at) : nullptr;
  };
  take(c.ctl, 1);
  take(c.list, max_chunks);
  take(c.part, max_chunks * 12);
  take(c.clus, max_chunks);
  take(c.tkey, tab);
  take(c.trep, tab);
  c.raw = reinterpret_cast<CcdEntry*>(c.part);
  if (bytes) *bytes = L.size;
  return c;
}

// first use (a handle that never comes here holds none of this)
int cc_ensure(tf_volume* v) {
  if (v->cc.block) return TF_OK;
  size_t bytes = 0;
  cc_carve(nullptr, v->dev.max_chunks, &bytes);
  return v->cc.block.alloc(bytes);
}

}  // namespace

void cc_release(tf_volume* v) { v->cc = CcState{}; }

// Chisel::CompensateColor enqueued on the handle's stream: no wait, nothing read back
int cc_enqueue(tf_volume* v, uint32_t* d_n_clusters) {
  const size_t mc = v->dev.max_chunks;
  const int rc = cc_ensure(v);
  if (rc) return rc;
  const CcdDev c = cc_carve(v->cc.block.p, mc, nullptr);
  hipStream_t s = v->stream;
  const unsigned per_thread = (unsigned)std::min<size_t>(std::max<size_t>((mc + 255) / 256, 1), kCcdGrid);
  TF_HIP(hipMemsetAsync(c.ctl, 0, 16, s));  // n_raw, n, n_clusters, tmask
  hipLaunchKernelGGL(k_ccd_list, dim3(1024), dim3(256), 0, s, v->dev, c);
  hipLaunchKernelGGL(k_ccd_rank, dim3(per_thread), dim3(256), 0, s, c);
  hipLaunchKernelGGL(k_ccd_cluster, dim3(per_thread), dim3(256), 0, s, c);
  hipLaunchKernelGGL(k_ccd_partial<0>, dim3(kCcdGrid), dim3(256), 0, s, v->dev, c);
  hipLaunchKernelGGL(k_ccd_combine<0>, dim3(kCcdGrid), dim3(256), 0, s, c, (uint32_t*)nullptr);
  hipLaunchKernelGGL(k_ccd_partial<1>, dim3(kCcdGrid), dim3(256), 0, s, v->dev, c);
  hipLaunchKernelGGL(k_ccd_combine<1>, dim3(kCcdGrid), dim3(256), 0, s, c, d_n_clusters);
  hipLaunchKernelGGL(k_ccd_apply, dim3(kCcdGrid), dim3(256), 0, s, v->dev, c);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_compensate_color_device(tf_volume* v, uint32_t* d_n_clusters) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV(v);
  return cc_enqueue(v, d_n_clusters);
}

// the same with a device word of the handle's own as d_n_clusters, then tf_sync and that word read back
int tf_compensate_color_device_count(tf_volume* v, int64_t* out_n_clusters) {
  if (!v || !out_n_clusters) { set_error("null argument"); return TF_ERR_INVALID; }
  *out_n_clusters = 0;
  TF_DEV(v);
  int rc = cc_ensure(v);
  if (rc) return rc;
  uint32_t* d_word = &cc_carve(v->cc.block.p, v->dev.max_chunks, nullptr).ctl->n_out;
  if ((rc = cc_enqueue(v, d_word)) || (rc = tf_sync(v))) return rc;
  uint32_t n = 0;
  TF_HIP(hipMemcpy(&n, d_word, 4, hipMemcpyDeviceToHost));
  *out_n_clusters = (int64_t)n;
  return TF_OK;
}

}  // extern "C"
