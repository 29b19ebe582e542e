// tf_texmap.hip -- TexMap (Structure/TexMap.{h,cpp}) resident on the device: chunkGraph (Structure/uni_graph.cpp), dataCost
// (Structure/sparse_matrix.cpp) and labelstorage per pool slot, the MRF problem of TexMap::view_selection assembled from them
// on the device, its solved labels assigned there -- the piece between Chunk::observations / Mesh::adj (already in HBM) and
// the solve (tf_mrf.hip) that used to travel through the host for every chunk.
//
// State (tf_volume::tm, handed to the kernels as TmDev; every pointer null until the first tf_texmap_* call, freed by
// tf_volume_reset / tf_volume_destroy).  node .. ctl are ONE device allocation laid out by the table tm_arrays, which first
// use (all or nothing), tf_texmap_clear and the release share:
//   node   [max_chunks] u32   bit 0: the chunk is a node (UniGraph::chunks); bits 1..6: an edge across face k of
//                             chisel::neighbourhood, kept on both ends (UniGraph::adj_lists); bit 7: the node had an entry
//                             of labelstorage at the last full solve (i < labelstorage.size())
//   label  [max_chunks] i32   UniGraph::labels: a keyframe index, 0 = none
//   stored [max_chunks] i32   labelstorage[i]: row + 1, or 0
//   key/q  open addressing    dataCost: key = (pool slot << 32 | keyframe FRAME INDEX) -> f32 quality, quality 0 = removed.
//                             Keyed by frame index and not by row, so that retraction needs no row lookup; rows (kflist
//                             positions) enter only when a problem is assembled, through kf_row.
//   ctl                       "a full solve has run" (!labelstorage.empty()), the size of the problem being assembled
// What grows is a Scratch grown by reserve() (TexMapState), which drains the stream before it frees a buffer in use:
//   kf     [n_rows + 64]      kf_row = kflist[r].keyFrameIndex (device half; the pinned half stages its upload), 64 words
//                             behind the rows for the tail's keyframes to update.  The dense inverse (frameIndexToKeyframeDB,
//                             MobileFusion.cpp:293-296) stays on the host (kf_inv): it only checks the frames an update names
//   pn, pz                    the problem assembled last, per node and per label (TmProb::take_nodes / take_labels)
// Pool slots never move and hash entries are never removed, so a slot is a chunk id for the life of the
// volume and per-slot state needs no relocation.  The reference's `statistic` vector is written and never read
// (TexMap.cpp:71-75,95): it is not kept.
//
// Assembly (tm_select): nodes are collected into a compact list (their numbering is free: the solver's
// labels, rounds and f64 trace do not depend on it), one wave per node walks the keyframe rows in ascending order and
// probes the cost table (tm_for_rows) -- the ballot order of the lanes IS the ascending row order of std::map -- a
// single-workgroup scan turns the column lengths into col_off, the host reads {n_nodes, nnz} once to size the solver's
// scratch, a second pass per node writes labels (row + 1), costs 1.0f - q / column_max (IEEE divide, no contraction), the
// neighbour indices and the warm start.  mrf_begin / mrf_enqueue_rounds solve it; k_tm_assign maps labels back to keyframe
// indices (TexMap.cpp:227-246).
#include <stddef.h>
#include <string.h>

#include <algorithm>

#include "tf_devfn.h"
#include "tf_mrf.h"
#include "tf_voxel_math.h"
#include "tf_volume.h"

namespace tf {
namespace {

constexpr int kTmMaxRounds = 4096;

// block `count` elements long out of the staging area L at base d (d == null: only L grows, by what the block needs)
template <typename T>
void tm_carve(T*& p, void* d, Layout& L, size_t count) {
  const size_t at = L.take(count * sizeof(T));
  p = d ? reinterpret_cast<T*>(static_cast<uint8_t*>(d) + at) : nullptr;
}

// the problem assembled last (device arrays; TexMapState::pn / pz)
struct TmProb {
  uint32_t cap;        // room for this many nodes
  uint32_t* slot;      // [cap] pool slot of node p
  int32_t* ids;        // [3 cap]
  int32_t* nbr;        // [6 cap]
  long long* col_off;  // [cap + 1]
  uint32_t* cnt;       // [cap] entries of the node's column (0 = the single label 0)
  int32_t* init;       // [cap]
  int32_t* off;        // [cap]
  int32_t* rounds;     // [4]
  double* energy;      // [kTmMaxRounds + 1]
  int32_t* labels;     // [nnz]
  float* costs;        // [nnz]
  // the per-node arrays for c nodes out of d (TexMapState::pn), the per-label arrays for c labels (pz)
  void take_nodes(Layout& L, void* d, size_t c) {
    cap = (uint32_t)c;
    tm_carve(slot, d, L, c); tm_carve(ids, d, L, 3 * c); tm_carve(nbr, d, L, 6 * c); tm_carve(col_off, d, L, c + 1);
    tm_carve(cnt, d, L, c); tm_carve(init, d, L, c); tm_carve(off, d, L, c); tm_carve(rounds, d, L, 4);
    tm_carve(energy, d, L, (size_t)kTmMaxRounds + 1);
  }
  void take_labels(Layout& L, void* d, size_t c) { tm_carve(labels, d, L, c); tm_carve(costs, d, L, c); }
};

__device__ __forceinline__ uint32_t tm_slot_of(const VolumeDev& v, int x, int y, int z) {
  const uint32_t e = hash_find(v, pack_id(x, y, z));
  if (e == kInvalidSlot) return kInvalidSlot;
  const uint32_t s = v.hent[e].slot;
  return s < v.max_chunks ? s : kInvalidSlot;
}
__device__ __forceinline__ int4 tm_face(int4 id, int k) {  // chisel::neighbourhood: -x +x -y +y -z +z
  const int d = (k & 1) ? 1 : -1;
  if ((k >> 1) == 0) id.x += d; else if ((k >> 1) == 1) id.y += d; else id.z += d;
  return id;
}
__device__ __forceinline__ uint32_t tm_find(const TmDev& v, unsigned long long key, bool insert) {
  uint32_t i = hash_key(key) & v.tm.mask;
  for (uint32_t probe = 0; probe <= v.tm.mask; ++probe) {
    unsigned long long cur = v.tm.key[i];
    if (cur == kEmptyKey) {
      if (!insert) return kInvalidSlot;
      cur = atomicCAS(&v.tm.key[i], kEmptyKey, key);
      if (cur == kEmptyKey) return i;
    }
    if (cur == key) return i;
    i = (i + 1) & v.tm.mask;
  }
  if (insert) atomicOr(&v.vctl->status, kStHashFull);
  return kInvalidSlot;
}
__device__ __forceinline__ float tm_cost(const TmDev& v, uint32_t slot, int32_t frame) {
  const uint32_t at = tm_find(v, obs_pack(slot, frame), false);
  return at == kInvalidSlot ? 0.0f : v.tm.q[at];
}
__device__ __forceinline__ float tm_obs(const VolumeDev& v, uint32_t slot, int32_t frame) {
  const uint32_t at = obs_find(v, obs_pack(slot, frame), false);
  return at == kInvalidSlot ? 0.0f : v.obs_q[at];
}
__device__ __forceinline__ bool tm_in_map(const VolumeDev& v, uint32_t slot) { return (v.mesh_rec[slot].state & kMsInMap) != 0; }
__device__ __forceinline__ bool tm_is_node(const TmDev& v, uint32_t slot) { return (v.tm.node[slot] & kTmNode) != 0; }

// The chunk-hash entry of this thread (one thread per entry, blocks of 256): false beyond the table, for an empty entry and
// for one without a pool slot; the kernels over the hash start here.
__device__ __forceinline__ bool tm_entry(const TmDev& v, HEntry* h) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e > v.hmask) return false;
  *h = v.hent[e];
  return h->key != kEmptyKey && h->slot < v.max_chunks;
}

// The column of a pool slot, walked by one wave: the keyframe rows in blocks of 64, lane = row within the block, every lane
// probing the cost table.  Per block fn(r, frame, q, present, before): the lane's row, frame index and quality (0: none),
// the ballot of the lanes with an entry (q > 0) and the entries of the blocks before -- before + popc(present & lanes
// below) is the entry's position in the column, rows ascending (the order of std::map).  Returns the column's length.
template <typename F>
__device__ __forceinline__ uint32_t tm_for_rows(const TmDev& v, uint32_t slot, int lane, F fn) {
  uint32_t before = 0;
  for (int32_t r0 = 0; r0 < v.tm.n_rows; r0 += 64) {
    const int32_t r = r0 + lane;
    const int32_t f = r < v.tm.n_rows ? v.tm.kf_row[r] : 0;
    const float q = r < v.tm.n_rows ? tm_cost(v, slot, f) : 0.0f;
    const unsigned long long present = __ballot(q > 0.0f);
    fn(r, f, q, present, before);
    before += (uint32_t)__popcll(present);
  }
  return before;
}

// UniGraph::add_node for every listed chunk (TexMap.cpp:53-55); all nodes are there before any edge is looked at
__global__ __launch_bounds__(256) void k_tm_add_nodes(TmDev v, const int4* __restrict__ ids, uint32_t n, const uint32_t* __restrict__ dn) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (dn) n = min(n, *dn);  // (a list whose length only the device knows: n is then its bound)
  if (i >= n) return;
  const int4 id = ids[i];
  const uint32_t slot = tm_slot_of(v, id.x, id.y, id.z);
  if (slot == kInvalidSlot) { atomicOr(&v.vctl->status, kStMissing); return; }
  atomicOr(&v.tm.node[slot], kTmNode);
}

// add_edge_by_node(id, mesh->adj) (TexMap.cpp:56-60, uni_graph.cpp:41-49) on threads k < 6 of a chunk's eight, and the
// chunk's column (update_datacost, TexMap.cpp:67-104) on thread 6: add_value keeps an existing entry, set_value
// overwrites, an absent observation removes.  A column is written by its own chunk's thread only.
__global__ __launch_bounds__(256) void k_tm_update(TmDev v, const int4* __restrict__ ids, uint32_t n, int32_t frame_index,
                                                   const int32_t* __restrict__ frames, int32_t m, const uint32_t* __restrict__ dn) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint32_t i = t >> 3, k = t & 7u;
  if (dn) n = min(n, *dn);
  if (i >= n || k == 7u) return;
  const int4 id = ids[i];
  const uint32_t slot = tm_slot_of(v, id.x, id.y, id.z);
  if (slot == kInvalidSlot) return;
  if (k < 6u) {
    const uint32_t st = v.mesh_rec[slot].state;
    if (!(st & kMsInMap) || !((st >> (kMsAdjShift + k)) & 1u)) return;
    const int4 q = tm_face(id, (int)k);
    const uint32_t ns = tm_slot_of(v, q.x, q.y, q.z);
    if (ns == kInvalidSlot || !(v.tm.node[ns] & kTmNode)) return;
    atomicOr(&v.tm.node[slot], 1u << (kTmEdgeShift + k));
    atomicOr(&v.tm.node[ns], 1u << (kTmEdgeShift + (k ^ 1u)));
    return;
  }
  const uint32_t os = hash_slot_alive(v, pack_id(id.x, id.y, id.z));  // (a parked chunk has no observations)
  const float q0 = os == kInvalidSlot ? 0.0f : tm_obs(v, os, frame_index);
  if (q0 > 0.0f) {
    const uint32_t at = tm_find(v, obs_pack(slot, frame_index), true);
    if (at != kInvalidSlot && !(v.tm.q[at] > 0.0f)) v.tm.q[at] = q0;
  }
  for (int32_t j = 0; j < m; ++j) {
    const int32_t f = frames[j];
    const float q = os == kInvalidSlot ? 0.0f : tm_obs(v, os, f);
    const uint32_t at = tm_find(v, obs_pack(slot, f), q > 0.0f);
    if (at != kInvalidSlot) v.tm.q[at] = q > 0.0f ? q : 0.0f;
  }
}

// MobileFusion::RetractObservations' data-cost half (MobileFusion.cpp:261-267)
__global__ __launch_bounds__(256) void k_tm_retract(TmDev v, int32_t kf_id, const int4* __restrict__ ids, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int4 id = ids[i];
  const uint32_t slot = hash_slot_alive(v, pack_id(id.x, id.y, id.z));  // !HasChunk -> continue (:258)
  if (slot == kInvalidSlot) return;
  const uint32_t at = tm_find(v, obs_pack(slot, kf_id), false);
  if (at != kInvalidSlot) v.tm.q[at] = 0.0f;
}

// MobileFusion.cpp:330-342 over the chunk hash: a mesh in the map whose patch has wrong_mapping loses the entry of the
// keyframe its patch was cut from.  ctl->n_removed counts the entries that were there.
__global__ __launch_bounds__(256) void k_tm_wrong_mapping(TmDev v) {
  HEntry h;
  if (!tm_entry(v, &h) || !(h.alive & 1u)) return;
  const MeshRec* r = &v.mesh_rec[h.slot];
  if (!(r->state & kMsInMap) || (r->pflags & (kPfHasPatch | kPfWrong)) != (kPfHasPatch | kPfWrong)) return;
  if (!tm_is_node(v, h.slot)) return;  // (the reference dereferences chunks.find() unchecked here)
  const uint32_t at = tm_find(v, obs_pack(h.slot, r->frameid), false);
  if (at != kInvalidSlot && v.tm.q[at] > 0.0f) {
    v.tm.q[at] = 0.0f;
    atomicAdd(&v.tm.ctl->n_removed, 1u);
  }
}

// TexMap::check_graph (TexMap.cpp:107-118): UniGraph::remove_node for every node whose mesh has left allMeshes -- its
// edges go on both ends, it stays a node (uni_graph.cpp:89-107) -- ...
__global__ __launch_bounds__(256) void k_tm_check_nodes(TmDev v) {
  HEntry h;
  if (!tm_entry(v, &h)) return;
  const uint32_t w = v.tm.node[h.slot];
  if (!(w & kTmNode) || tm_in_map(v, h.slot)) return;
  atomicAdd(&v.tm.ctl->n_removed, 1u);
  if (!(w & kTmEdges)) return;
  const int4 id = unpack_id(h.key);
  for (int k = 0; k < 6; ++k) {
    if (!((w >> (kTmEdgeShift + k)) & 1u)) continue;
    const int4 q = tm_face(id, k);
    const uint32_t ns = tm_slot_of(v, q.x, q.y, q.z);
    if (ns != kInvalidSlot) atomicAnd(&v.tm.node[ns], ~(1u << (kTmEdgeShift + (k ^ 1))));
  }
  atomicAnd(&v.tm.node[h.slot], ~kTmEdges);
}
// ... and SparseMat::remove_node: its column is emptied (sparse_matrix.h:67-70), over the cost table
__global__ __launch_bounds__(256) void k_tm_check_costs(TmDev v) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i > v.tm.mask) return;
  const unsigned long long key = v.tm.key[i];
  if (key == kEmptyKey) return;
  const uint32_t slot = (uint32_t)(key >> 32);
  if (slot >= v.max_chunks || !(v.tm.q[i] > 0.0f)) return;
  if ((v.tm.node[slot] & kTmNode) && !tm_in_map(v, slot)) v.tm.q[i] = 0.0f;
}

// ---- the problem --------------------------------------------------------------------------------------------------
// every node of the graph (TexMap.cpp:122), off the chunk hash: the hash entry holds the id the solver's checks want
__global__ __launch_bounds__(256) void k_tm_collect_all(TmDev v, TmProb P) {
  HEntry h;
  if (!tm_entry(v, &h) || !tm_is_node(v, h.slot)) return;
  const uint32_t p = atomicAdd(&v.tm.ctl->n_nodes, 1u);
  if (p >= P.cap) return;
  const int4 id = unpack_id(h.key);
  P.slot[p] = h.slot;
  P.ids[3 * p] = id.x; P.ids[3 * p + 1] = id.y; P.ids[3 * p + 2] = id.z;
  v.tm.idx[h.slot] = p;
}
// `concerns`: the listed chunks that are nodes (TexMap.cpp:261-267); a chunk listed twice is one node
__global__ __launch_bounds__(256) void k_tm_collect_ids(TmDev v, TmProb P, const int4* __restrict__ ids, uint32_t n, const uint32_t* __restrict__ dn) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (dn) n = min(n, *dn);
  if (i >= n) return;
  const int4 id = ids[i];
  const uint32_t slot = tm_slot_of(v, id.x, id.y, id.z);
  if (slot == kInvalidSlot || !(v.tm.node[slot] & kTmNode)) return;
  if (atomicOr(&v.tm.node[slot], kTmTmp) & kTmTmp) return;
  const uint32_t p = atomicAdd(&v.tm.ctl->n_nodes, 1u);
  if (p >= P.cap) return;
  P.slot[p] = slot;
  P.ids[3 * p] = id.x; P.ids[3 * p + 1] = id.y; P.ids[3 * p + 2] = id.z;
  v.tm.idx[slot] = p;
}

// One wave per node: the entries of its column, rows ascending (lane = row within a block of 64 rows).
__global__ __launch_bounds__(256) void k_tm_count(TmDev v, TmProb P) {
  const uint32_t n = min(v.tm.ctl->n_nodes, P.cap);
  const int lane = (int)(threadIdx.x & 63u);
  for (uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6); p < n; p += gridDim.x * 4u) {
    const uint32_t slot = P.slot[p];
    const uint32_t K = tm_for_rows(v, slot, lane, [](int32_t, int32_t, float, unsigned long long, uint32_t) {});
    if (lane == 0) {
      P.cnt[p] = K;
      if (v.tm.node[slot] & kTmTmp) atomicAnd(&v.tm.node[slot], ~kTmTmp);
    }
  }
}

// col_off = exclusive scan of max(cnt, 1) (an empty column is the single label 0), nnz into the control block
__global__ __launch_bounds__(1024) void k_tm_scan(TmDev v, TmProb P) {
  __shared__ unsigned long long part[1024];
  const uint32_t n = min(v.tm.ctl->n_nodes, P.cap);
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t a = min(t * per, n), b = min(a + per, n);
  unsigned long long s = 0;
  for (uint32_t p = a; p < b; ++p) s += P.cnt[p] ? P.cnt[p] : 1u;
  part[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < 1024u; d <<= 1) {
    const unsigned long long add = t >= d ? part[t - d] : 0ull;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  unsigned long long at = part[t] - s;
  for (uint32_t p = a; p < b; ++p) {
    P.col_off[p] = (long long)at;
    at += P.cnt[p] ? P.cnt[p] : 1u;
  }
  if (t == 1023u) {
    P.col_off[n] = (long long)part[1023];
    v.tm.ctl->nnz = part[1023];
  }
}

// One wave per node: labels, costs, neighbours, warm start -- as tf_chisel.hpp's TexMap::solve builds them on the host
// (TexMap.cpp:123-180, :208-217).
__global__ __launch_bounds__(256) void k_tm_fill(TmDev v, TmProb P, uint32_t n, int full) {
  const int lane = (int)(threadIdx.x & 63u);
  // the full overload starts from the stored labels once a full solve has run (TexMap.cpp:200-217: !labelstorage.empty());
  // before that, and in the sub-problem, from the cheapest label of every node, lowest offset -- written here as well, so
  // that the start is always an explicit labelling
  const int warm = full && v.tm.ctl->solved;
  if (blockIdx.x == 0 && threadIdx.x == 0) P.rounds[1] = warm;
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (uint32_t p = blockIdx.x * 4u + (threadIdx.x >> 6); p < n; p += gridDim.x * 4u) {
    const uint32_t slot = P.slot[p];
    const uint32_t K = P.cnt[p];
    const long long c0 = P.col_off[p];
    const uint32_t word = v.tm.node[slot];
    int init = 0;
    if (K == 0) {  // :145-146, :165-166
      if (lane == 0) { P.labels[c0] = 0; P.costs[c0] = 1.0f; }
    } else {
      float mx = 0.0f;  // column_max (:168-170; qualities are > 0)
      tm_for_rows(v, slot, lane, [&](int32_t, int32_t, float q, unsigned long long, uint32_t) { mx = fmaxf(mx, q); });
#pragma unroll
      for (int d = 32; d; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
      const int32_t want = (warm && (word & kTmHadLabel)) ? v.tm.stored[slot] : -1;
      // tm_for_rows' walk written out and to be kept like it: in helper form this pass costs the kernel a 43rd VGPR
      uint32_t pos = 0;
      float cbest = INFINITY;
      uint32_t jbest = 0xFFFFFFFFu;
      for (int32_t r0 = 0; r0 < v.tm.n_rows; r0 += 64) {
        const int32_t r = r0 + lane;
        const float q = r < v.tm.n_rows ? tm_cost(v, slot, v.tm.kf_row[r]) : 0.0f;
        const bool have = q > 0.0f;
        const unsigned long long m = __ballot(have);
        const uint32_t j = pos + (uint32_t)__popcll(m & lt);
        if (have) {
          const float c = 1.0f - q / mx;                  // :173-174
          P.labels[c0 + j] = (int32_t)(uint16_t)(r + 1);  // :150-151
          P.costs[c0 + j] = c;
          if (c < cbest) { cbest = c; jbest = j; }        // (a lane's offsets ascend)
        }
        const unsigned long long hit = __ballot(have && r + 1 == want);
        if (hit) init = (int)(pos + (uint32_t)__popcll(m & (hit - 1ull)));  // (one lane at most)
        pos += (uint32_t)__popcll(m);
      }
      if (!warm) {  // the cheapest label, lowest offset
#pragma unroll
        for (int d = 32; d; d >>= 1) {
          const float oc = __shfl_xor(cbest, d);
          const uint32_t oj = __shfl_xor(jbest, d);
          if (oc < cbest || (oc == cbest && oj < jbest)) { cbest = oc; jbest = oj; }
        }
        init = (int)jbest;
      }
    }
    // :126-135: an edge needs both ends in the problem, both with entries in their columns
    if (lane < 6) {
      int nb = -1;
      if (K && ((word >> (kTmEdgeShift + lane)) & 1u)) {
        int4 id = make_int4(P.ids[3 * p], P.ids[3 * p + 1], P.ids[3 * p + 2], 0);
        id = tm_face(id, lane);
        const uint32_t ns = tm_slot_of(v, id.x, id.y, id.z);
        if (ns != kInvalidSlot) {
          const uint32_t pp = v.tm.idx[ns];
          if (pp < n && P.slot[pp] == ns && P.cnt[pp]) nb = (int)pp;
        }
      }
      P.nbr[6 * p + lane] = nb;
    }
    if (lane == 0) P.init[p] = init;
  }
}

// chunksToUpdate in ascending chunk id (the order the path defines for Atlas::AddPatch) by comparison
// counting: entry i goes to position #{j : key_j < key_i}; keys are distinct (a dirty set).  Tiles of 256 keys through LDS.
__global__ __launch_bounds__(256) void k_tm_rank(TmDev v, const int4* __restrict__ in, const uint32_t* __restrict__ dn, uint32_t cap,
                                                 int4* __restrict__ out) {
  __shared__ unsigned long long tile[256];
  const uint32_t n = min(*dn, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) v.tm.ctl->n_list = n;
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const int4 id = i < n ? in[i] : make_int4(0, 0, 0, 0);
    const unsigned long long key = pack_id(id.x, id.y, id.z);
    uint32_t rank = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {
      __syncthreads();
      const uint32_t j = t0 + threadIdx.x;
      if (j < n) { const int4 q = in[j]; tile[threadIdx.x] = pack_id(q.x, q.y, q.z); }
      __syncthreads();
      const uint32_t m = min(256u, n - t0);
      for (uint32_t k = 0; k < m; ++k) rank += (uint32_t)(tile[k] < key);
    }
    if (i < n) out[rank] = make_int4(id.x, id.y, id.z, 0);
  }
}

// TexMap.cpp:227-246 (:386-405): label 0 keeps the chunk's label, or takes the keyframe before the newest when the chunk
// never had one; the full overload replaces labelstorage.  Nothing is written when the solver's check refused the problem.
__global__ __launch_bounds__(256) void k_tm_assign(TmDev v, TmProb P, uint32_t n, int full, const MrfCtl* mc) {
  if (mc->bad != ~0ull) return;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0 && full) v.tm.ctl->solved = 1u;
  if (p >= n) return;
  const uint32_t slot = P.slot[p];
  const int32_t label = P.labels[P.col_off[p] + P.off[p]];
  if (label == 0) {
    if (v.tm.label[slot] == 0 && v.tm.n_rows >= 2) v.tm.label[slot] = v.tm.kf_row[v.tm.n_rows - 2];
  } else if (label <= v.tm.n_rows) {
    v.tm.label[slot] = v.tm.kf_row[label - 1];
  }
  if (full) {
    v.tm.stored[slot] = label;
    v.tm.node[slot] |= kTmHadLabel;
  }
}

// ---- mirrors ---------------------------------------------------------------------------------------------------------
// per listed chunk: info[4 i ..] = {node word (0: no node), chunk label, stored label, column entries}; the column as
// (frame index, quality) in ascending row at [i * n_rows ..]
__global__ __launch_bounds__(256) void k_tm_download(TmDev v, const int4* __restrict__ ids, uint32_t n, int32_t* __restrict__ info,
                                                     int32_t* __restrict__ col_frame, float* __restrict__ col_q) {
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += gridDim.x * 4u) {
    const int4 id = ids[i];
    const uint32_t slot = tm_slot_of(v, id.x, id.y, id.z);
    const uint32_t word = slot == kInvalidSlot ? 0u : v.tm.node[slot];
    uint32_t pos = 0;
    if (word & kTmNode)
      pos = tm_for_rows(v, slot, lane, [&](int32_t, int32_t f, float q, unsigned long long m, uint32_t before) {
        if (q > 0.0f) {
          const size_t at = (size_t)i * (size_t)v.tm.n_rows + before + (uint32_t)__popcll(m & lt);
          col_frame[at] = f;
          col_q[at] = q;
        }
      });
    if (lane == 0) {
      info[4 * i] = (int32_t)(word & kTmNode ? word & (kTmNode | kTmEdges | kTmHadLabel) : 0u);
      info[4 * i + 1] = (word & kTmNode) ? v.tm.label[slot] : 0;
      info[4 * i + 2] = (word & kTmNode) ? v.tm.stored[slot] : 0;
      info[4 * i + 3] = (int32_t)pos;
    }
  }
}

// Chisel::GeneratePatches' labelset lookup (Chisel.cpp:159-160) for the patch work list: the keyframe of entry i is its
// chunk's resident label, w = the keyframe-table entry that caches it.  The first entry with a mesh that is no node, or
// whose label names no cached keyframe, is recorded; k_tm_work_cut takes it and everything behind it out of the stage.
__global__ __launch_bounds__(256) void k_tm_work_labels(TmDev v, uint32_t n, int kf_cap, uint32_t* first_fail) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = v.work_slot[i];
  if (slot == kInvalidSlot) return;  // !HasMesh -> continue (:157)
  int kf = -1;
  if (v.tm.node[slot] & kTmNode) {
    const int32_t label = v.tm.label[slot];
    for (int s = 0; s < kf_cap; ++s)
      if (v.kf_tab[s].kf_id == label && v.kf_tab[s].rgb) { kf = s; break; }
  }
  if (kf < 0) { atomicMin(first_fail, i); return; }
  v.work_ids[i].w = kf;
}
__global__ __launch_bounds__(256) void k_tm_work_cut(TmDev v, uint32_t n, const uint32_t* first_fail) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t ff = *first_fail;
  if (ff == 0xFFFFFFFFu) return;
  if (i == 0) atomicOr(&v.vctl->status, kStInvalid);
  if (i >= ff && i < n) v.work_slot[i] = kInvalidSlot;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The map's device arrays in the order they lie in its one block (node first: the block's base) as fn(member, bytes, fill)
template <typename F>
void tm_arrays(TexMapDev& t, size_t max_chunks, F fn) {
  const size_t mc = max_chunks, cap = (size_t)t.mask + 1;  // (the cost table is as large as the observation table it mirrors)
  fn(t.node, 4 * mc, 0); fn(t.label, 4 * mc, 0); fn(t.stored, 4 * mc, 0); fn(t.idx, 4 * mc, 0xFF);
  fn(t.key, 8 * cap, 0xFF); fn(t.q, 4 * cap, 0); fn(t.ctl, sizeof(TexMapCtl), 0);
}

int tm_fill(tf_volume* v) {
  hipError_t e = hipSuccess;
  tm_arrays(v->tm, v->dev.max_chunks, [&](auto* p, size_t bytes, int fill) {
    if (e == hipSuccess) e = hipMemsetAsync(p, fill, bytes, v->stream);
  });
  TF_HIP(e);
  return TF_OK;
}

// First use, all or nothing: one that fails gives back what it took, so node != null says that the whole map is there
int tm_ensure(tf_volume* v) {
  TexMapDev& t = v->tm;
  if (t.node) return TF_OK;
  t.mask = v->dev.obs_mask;
  void* d = nullptr;
  Layout L;
  const auto carve = [&](auto*& p, size_t bytes, int) { tm_carve(p, d, L, bytes / sizeof(*p)); };
  tm_arrays(t, v->dev.max_chunks, carve);  // (d == null: the block's size)
  int rc;
  if (!(rc = v->tmx.block.alloc(L.size)) && !(rc = v->tmx.h_ctl.alloc(sizeof(TexMapCtl)))) {
    d = v->tmx.block.p;
    L = Layout{};
    tm_arrays(t, v->dev.max_chunks, carve);
    rc = tm_fill(v);
  }
  if (rc) texmap_release(v);
  return rc;
}

// room for `want` nodes in TexMapState::pn (per_node) or labels in pz: a power of two of at least 1024 that never shrinks
int tm_room(tf_volume* v, bool per_node, size_t want) {
  TexMapState& x = v->tmx;
  size_t& cap = per_node ? x.pn_cap : x.pz_cap;
  size_t c = std::max<size_t>(cap, 1024);
  while (c < want) c <<= 1;
  TmProb P{};
  Layout L;
  if (per_node) P.take_nodes(L, nullptr, c); else P.take_labels(L, nullptr, c);
  const int rc = reserve(v, per_node ? x.pn : x.pz, L.size, 0);
  if (!rc) cap = c;
  return rc;
}

TmProb tm_prob(const TexMapState& x) {
  TmProb P{};
  Layout N, Z;
  P.take_nodes(N, x.pn.d.p, x.pn_cap);
  P.take_labels(Z, x.pz.d.p, x.pz_cap);
  return P;
}

unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }
unsigned wave_blocks(size_t n) { return (unsigned)std::min<size_t>(std::max<size_t>((n + 3) / 4, 1), 8192); }

}  // namespace

void texmap_release(tf_volume* v) {
  if (v->tmx.kf_ev) hipEventDestroy(v->tmx.kf_ev);
  v->tm = TexMapDev{};
  v->tmx = TexMapState{};  // (its owners free the map's block, the control block's pinned copy, the pools and the lists)
}

void launch_tm_work_labels(tf_volume* v, uint32_t n, uint32_t* d_first_fail) {
  hipStream_t s = v->stream;
  hipMemsetAsync(d_first_fail, 0xFF, 4, s);
  hipLaunchKernelGGL(k_tm_work_labels, dim3(blocks_of(n, 256)), dim3(256), 0, s, tm_dev(v), n, v->atlas.kf_cap, d_first_fail);
  hipLaunchKernelGGL(k_tm_work_cut, dim3(blocks_of(n, 256)), dim3(256), 0, s, tm_dev(v), n, d_first_fail);
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_texmap_set_keyframes(tf_volume* v, const int32_t* key_frame_index, int32_t n_rows) {
  if (!v || !key_frame_index) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n_rows < 1 || n_rows > 65534) { set_error("texmap: n_rows must be 1 .. 65534 (labels are cast to uint16_t, TexMap.cpp:150-151)"); return TF_ERR_INVALID; }
  int32_t top = -1;
  for (int32_t r = 0; r < n_rows; ++r) {
    if (key_frame_index[r] < 0 || key_frame_index[r] >= (1 << 24)) { set_error("texmap: a keyframe's frame index must be 0 .. 2^24 - 1"); return TF_ERR_INVALID; }
    top = std::max(top, key_frame_index[r]);
  }
  std::vector<int32_t> inv((size_t)top + 1, -1);
  for (int32_t r = 0; r < n_rows; ++r) {
    if (inv[(size_t)key_frame_index[r]] >= 0) { set_error("texmap: frame indices of the keyframe list must be distinct"); return TF_ERR_INVALID; }
    inv[(size_t)key_frame_index[r]] = r;
  }
  TF_DEV(v);
  int rc = tm_ensure(v);
  if (rc) return rc;
  TexMapState& x = v->tmx;
  if (!x.kf_ev) TF_HIP(hipEventCreateWithFlags(&x.kf_ev, hipEventDisableTiming));
  else TF_HIP(hipEventSynchronize(x.kf_ev));  // the previous upload has left the staging buffer
  const size_t bytes = 4 * std::max<size_t>((size_t)n_rows + 64, 256);  // (64 words behind the rows: the tail's keyframes to update)
  if ((rc = reserve(v, x.kf, bytes, bytes))) { v->tm.kf_row = nullptr; v->tm.n_rows = 0; return rc; }
  memcpy(x.kf.h.p, key_frame_index, 4 * (size_t)n_rows);
  TF_HIP(hipMemcpyAsync(x.kf.d.p, x.kf.h.p, 4 * (size_t)n_rows, hipMemcpyHostToDevice, v->stream));
  TF_HIP(hipEventRecord(x.kf_ev, v->stream));
  x.kf_row.assign(key_frame_index, key_frame_index + n_rows);
  x.kf_inv.swap(inv);
  v->tm.kf_row = x.kf.d.as<const int32_t>();
  v->tm.n_rows = n_rows;
  return TF_OK;
}

// the two device lists of chunksToUpdate (first use): one allocation
static int tm_list_buffers(tf_volume* v) {
  TexMapState& x = v->tmx;
  if (x.d_ctu) return TF_OK;
  const size_t mc = v->dev.max_chunks;
  const int rc = x.ctu.alloc(2 * mc * 16);
  if (!rc) x.d_ctu = x.ctu.as<int4>() + mc;
  return rc;
}
// frames_to_update of the tail: into the tail of the keyframe table's device half, through its pinned half
static int tm_frames_upload(tf_volume* v, const int32_t* frames, int32_t n, const int32_t** d_out) {
  TexMapState& x = v->tmx;
  const size_t rows = (size_t)v->tm.n_rows;
  if (rows + (size_t)n > x.kf.d.bytes / 4) { set_error("texmap: more keyframes to update than the keyframe table has room behind its rows"); return TF_ERR_CAPACITY; }
  int32_t *h = x.kf.h.as<int32_t>() + rows, *d = x.kf.d.as<int32_t>() + rows;
  TF_HIP(hipEventSynchronize(x.kf_ev));
  memcpy(h, frames, 4 * (size_t)n);
  TF_HIP(hipMemcpyAsync(d, h, 4 * (size_t)n, hipMemcpyHostToDevice, v->stream));
  TF_HIP(hipEventRecord(x.kf_ev, v->stream));
  *d_out = d;
  return TF_OK;
}

// the two launches of an update over a device list of n entries (dn != null: at most n, the device knows how many)
static int tm_update_enqueue(tf_volume* v, const int4* d_ids, uint32_t n, const uint32_t* dn, int32_t frame_index,
                             const int32_t* d_frames, int32_t n_frames) {
  hipLaunchKernelGGL(k_tm_add_nodes, dim3(blocks_of((size_t)n, 256)), dim3(256), 0, v->stream, tm_dev(v), d_ids, n, dn);
  hipLaunchKernelGGL(k_tm_update, dim3(blocks_of((size_t)n * 8, 256)), dim3(256), 0, v->stream, tm_dev(v), d_ids, n, frame_index,
                     d_frames, n_frames, dn);
  TF_HIP(hipGetLastError());
  v->tmx.nodes_bound = std::min<int64_t>(v->tmx.nodes_bound + n, (int64_t)v->dev.max_chunks);
  return TF_OK;
}

// the keyframe of an update and its n keyframes to update must be in the keyframe table
static int tm_frames_known(const tf_volume* v, int32_t frame_index, const int32_t* frames, int32_t n) {
  const std::vector<int32_t>& inv = v->tmx.kf_inv;
  for (int32_t j = -1; j < n; ++j) {
    const int32_t f = j < 0 ? frame_index : frames[j];
    if (f >= 0 && (size_t)f < inv.size() && inv[(size_t)f] >= 0) continue;
    set_error("texmap: frame index " + std::to_string(f) + " is not in the keyframe table (tf_texmap_set_keyframes)");
    return TF_ERR_INVALID;
  }
  return TF_OK;
}

int tf_texmap_update(tf_volume* v, const int32_t* ids, int64_t n, int32_t frame_index, const int32_t* frames_to_update,
                     int32_t n_frames) {
  if (!v || (n > 0 && !ids) || n_frames < 0 || (n_frames > 0 && !frames_to_update)) { set_error("invalid argument"); return TF_ERR_INVALID; }
  int rc = tm_frames_known(v, frame_index, frames_to_update, n_frames);
  if (rc) return rc;
  if (n > (int64_t)v->dev.max_chunks) { set_error("chunk list longer than tf_config.max_chunks"); return TF_ERR_CAPACITY; }
  TF_DEV(v);
  if ((rc = tm_ensure(v))) return rc;
  if (n <= 0) return TF_OK;
  Layout L;
  L.take((size_t)n * 16);
  const size_t o_fr = L.take((size_t)n_frames * 4);
  Stage sg;
  if ((rc = stage_ids(v, v->scratch, L.size, ids, n, &sg))) return rc;
  if (n_frames && (rc = stage_in(v, sg, o_fr, frames_to_update, (size_t)n_frames * 4))) return rc;
  return tm_update_enqueue(v, sg.dp<const int4>(0), (uint32_t)n, nullptr, frame_index, sg.dp<const int32_t>(o_fr), n_frames);
}

int tf_texmap_retract(tf_volume* v, int32_t keyframe_id, const int32_t* ids, int64_t n) {
  if (!v || (n > 0 && !ids)) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (n <= 0 || !v->tm.node) return TF_OK;  // no map: no column to retract from
  Stage sg;
  int rc = stage_ids(v, v->scratch, (size_t)n * 16, ids, n, &sg);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tm_retract, dim3(blocks_of((size_t)n, 256)), dim3(256), 0, v->stream, tm_dev(v), keyframe_id,
                     sg.dp<const int4>(0), (uint32_t)n);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// MobileFusion.cpp:330-342 and TexMap::check_graph on the stream; TexMapCtl::n_removed counts what the pass removed
static int tm_wrong_mapping_enqueue(tf_volume* v) {
  TF_HIP(hipMemsetAsync(&v->tm.ctl->n_removed, 0, 4, v->stream));
  hipLaunchKernelGGL(k_tm_wrong_mapping, dim3(blocks_of((size_t)v->dev.hmask + 1, 256)), dim3(256), 0, v->stream, tm_dev(v));
  TF_HIP(hipGetLastError());
  return TF_OK;
}
static int tm_check_graph_enqueue(tf_volume* v) {
  TF_HIP(hipMemsetAsync(&v->tm.ctl->n_removed, 0, 4, v->stream));
  hipLaunchKernelGGL(k_tm_check_nodes, dim3(blocks_of((size_t)v->dev.hmask + 1, 256)), dim3(256), 0, v->stream, tm_dev(v));
  hipLaunchKernelGGL(k_tm_check_costs, dim3(blocks_of((size_t)v->tm.mask + 1, 256)), dim3(256), 0, v->stream, tm_dev(v));
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// the entry point around one of the two passes; n_removed != NULL: waits for the count
static int tm_removal(tf_volume* v, int (*enqueue)(tf_volume*), int64_t* n_removed) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (n_removed) *n_removed = 0;
  if (!v->tm.node) return TF_OK;
  const int rc = enqueue(v);
  if (rc || !n_removed) return rc;
  TF_HIP(hipMemcpyAsync(v->tmx.h_ctl.p, v->tm.ctl, sizeof(TexMapCtl), hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  *n_removed = v->tmx.h_ctl.as<TexMapCtl>()->n_removed;
  return TF_OK;
}

int tf_texmap_remove_wrong_mapping(tf_volume* v, int64_t* n_removed) { return tm_removal(v, tm_wrong_mapping_enqueue, n_removed); }
int tf_texmap_check_graph(tf_volume* v, int64_t* n_removed) { return tm_removal(v, tm_check_graph_enqueue, n_removed); }

struct TmWant {  // what a caller of tm_select wants back (null: not wanted)
  double* energy;    // the f64 trace [0 .. rounds]; needs rounds
  int32_t* rounds;   // (waits for the solve)
  int64_t* n_nodes;
  uint32_t* list_n;  // TexMapCtl::n_list as the one wait read it
};
// n_nodes and nnz of the control block, the problem being assembled, are zeroed as one
constexpr size_t kTmCtlProblem = offsetof(TexMapCtl, n_removed) - offsetof(TexMapCtl, n_nodes);
static_assert(offsetof(TexMapCtl, nnz) == offsetof(TexMapCtl, n_nodes) + 4 && kTmCtlProblem == 12, "n_nodes and nnz are adjacent");

// The assembly, the solve and the assignment.  d_ids == null: the full overload; else the sub-problem over a device list of
// n entries (dn != null: at most n).  Contains the one wait.
static int tm_select(tf_volume* v, const int4* d_ids, uint32_t n, const uint32_t* dn, int32_t max_rounds, const TmWant& want) {
  TexMapState& x = v->tmx;
  const bool full = d_ids == nullptr;
  const int64_t bound = full ? x.nodes_bound : (int64_t)n;
  x.n = x.nnz = 0;
  hipStream_t s = v->stream;
  TexMapCtl* ctl = v->tm.ctl;
  int rc;
  if (bound <= 0) {  // (tsdfFusion asks num_nodes() > 0 first; `concerns.empty()` returns)
    if (want.list_n) {
      TF_HIP(hipMemcpyAsync(x.h_ctl.p, ctl, sizeof(TexMapCtl), hipMemcpyDeviceToHost, s));
      TF_HIP(hipStreamSynchronize(s));
      *want.list_n = x.h_ctl.as<TexMapCtl>()->n_list;
    }
    return TF_OK;
  }
  if ((rc = tm_room(v, true, (size_t)bound))) return rc;
  TF_HIP(hipMemsetAsync(&ctl->n_nodes, 0, kTmCtlProblem, s));
  TmProb P = tm_prob(x);
  if (full) hipLaunchKernelGGL(k_tm_collect_all, dim3(blocks_of((size_t)v->dev.hmask + 1, 256)), dim3(256), 0, s, tm_dev(v), P);
  else hipLaunchKernelGGL(k_tm_collect_ids, dim3(blocks_of((size_t)n, 256)), dim3(256), 0, s, tm_dev(v), P, d_ids, n, dn);
  hipLaunchKernelGGL(k_tm_count, dim3(wave_blocks((size_t)bound)), dim3(256), 0, s, tm_dev(v), P);
  hipLaunchKernelGGL(k_tm_scan, dim3(1), dim3(1024), 0, s, tm_dev(v), P);
  TF_HIP(hipGetLastError());
  // the one wait: {n_nodes, nnz} size the solver's scratch and the launch grids
  TF_HIP(hipMemcpyAsync(x.h_ctl.p, ctl, sizeof(TexMapCtl), hipMemcpyDeviceToHost, s));
  TF_HIP(hipStreamSynchronize(s));
  if (want.list_n) *want.list_n = x.h_ctl.as<TexMapCtl>()->n_list;
  const int64_t nn = std::min<int64_t>(x.h_ctl.as<TexMapCtl>()->n_nodes, (int64_t)P.cap), nnz = (int64_t)x.h_ctl.as<TexMapCtl>()->nnz;
  if (want.n_nodes) *want.n_nodes = nn;
  if (nn == 0) return TF_OK;
  if ((rc = tm_room(v, false, (size_t)nnz))) return rc;
  P = tm_prob(x);
  TF_HIP(hipMemsetAsync(P.rounds, 0xFF, 16, s));  // [0] = -1: the checking launch refused the problem; [1]: started warm (k_tm_fill)
  hipLaunchKernelGGL(k_tm_fill, dim3(wave_blocks((size_t)nn)), dim3(256), 0, s, tm_dev(v), P, (uint32_t)nn, full ? 1 : 0);
  const int R = max_rounds ? max_rounds : kMrfDefaultRounds;
  MrfArgs a{};
  a.n = (int32_t)nn; a.nnz = nnz; a.ids = P.ids; a.nbr = P.nbr; a.col_off = reinterpret_cast<const int64_t*>(P.col_off);
  a.labels = P.labels; a.costs = P.costs; a.init = P.init; a.w = 0.5f * 1.0f;  // adjacent_cost * pairwise_cost (TexMap.h:53-54)
  a.off = P.off; a.energy = P.energy; a.rounds = P.rounds;
  if ((rc = mrf_begin(v, a, 0)) || (rc = mrf_enqueue_rounds(v, a, 1, R))) return rc;
  hipLaunchKernelGGL(k_tm_assign, dim3(blocks_of((size_t)nn, 256)), dim3(256), 0, s, tm_dev(v), P, (uint32_t)nn, full ? 1 : 0, a.ctl);
  TF_HIP(hipGetLastError());
  x.n = nn; x.nnz = nnz;
  if (!want.rounds) return TF_OK;
  // the caller wants the trace: wait for it.  (A refused problem: k_tm_assign wrote nothing, labels and the solved flag are as before.)
  if ((rc = reserve(v, v->scratch, 0, MrfResult::bytes(R)))) return rc;
  const MrfResult* res = v->scratch.h.as<const MrfResult>();
  if ((rc = mrf_read_back(v, a, R, v->scratch.h.as<MrfResult>()))) return rc;
  *want.rounds = res->rounds[0];
  if (want.energy && res->rounds[0] >= 0) memcpy(want.energy, res->energy, 8 * (size_t)(res->rounds[0] + 1));
  return TF_OK;
}

int tf_texmap_view_selection(tf_volume* v, const int32_t* ids, int64_t n, int32_t max_rounds, double* out_energy,
                             int32_t* out_rounds, int64_t* out_n_nodes) {
  if (!v || (ids && n < 0)) { set_error("invalid argument"); return TF_ERR_INVALID; }
  if (max_rounds < 0 || max_rounds > kTmMaxRounds) { set_error("view selection: max_rounds must be 0 .. 4096"); return TF_ERR_INVALID; }
  if (out_energy && !out_rounds) { set_error("view selection: out_energy needs out_rounds"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (out_n_nodes) *out_n_nodes = 0;
  if (out_rounds) *out_rounds = 0;
  if (!v->tm.node || !v->tm.n_rows) { set_error("texmap: no keyframe table (tf_texmap_set_keyframes)"); return TF_ERR_INVALID; }
  const TmWant want{out_energy, out_rounds, out_n_nodes, nullptr};
  if (!ids) return tm_select(v, nullptr, 0, nullptr, max_rounds, want);
  if (n > (int64_t)v->dev.max_chunks) { set_error("chunk list longer than tf_config.max_chunks"); return TF_ERR_CAPACITY; }
  v->tmx.n = v->tmx.nnz = 0;
  if (n == 0) return TF_OK;
  // the list goes into a buffer of the map's own: the solver's scratch takes the pool the staging helper would use
  int rc = tm_list_buffers(v);
  if (rc) return rc;
  Stage sg;
  if ((rc = stage_ids(v, v->scratch, (size_t)n * 16, ids, n, &sg))) return rc;
  TF_HIP(hipMemcpyAsync(v->tmx.ctu.as<int4>(), sg.d, (size_t)n * 16, hipMemcpyDeviceToDevice, v->stream));
  return tm_select(v, v->tmx.ctu.as<int4>(), (uint32_t)n, nullptr, max_rounds, want);
}

// MobileFusion::tsdfFusion's tail (GCFusion/MobileFusion.cpp:330-382; CompensateColor with TF_TAIL_COMPENSATE_COLOR) in one call
int tf_texture_tail_device(tf_volume* v, int32_t frame_index, const int32_t* frames_to_update, int32_t n_frames, uint32_t flags,
                           int32_t max_rounds) {
  if (!v || n_frames < 0 || (n_frames > 0 && !frames_to_update) || (flags & ~15u)) { set_error("invalid argument"); return TF_ERR_INVALID; }
  if (max_rounds < 0 || max_rounds > kTmMaxRounds) { set_error("view selection: max_rounds must be 0 .. 4096"); return TF_ERR_INVALID; }
  int rc = tm_frames_known(v, frame_index, frames_to_update, n_frames);
  if (rc) return rc;
  TF_DEV(v);
  if ((rc = tm_ensure(v)) || (rc = tm_list_buffers(v))) return rc;
  TexMapState& x = v->tmx;
  hipStream_t s = v->stream;
  x.ctu_n = 0;
  if ((flags & TF_TAIL_WRONG_MAPPING) && (rc = tm_wrong_mapping_enqueue(v))) return rc;  // :330-342
  // :345-355 chunksToUpdate + CompressMeshes; the list sorted on the device
  uint32_t bound = 0;
  uint32_t* d_count = &v->tm.ctl->n_raw;
  if ((rc = compress_device_list(v, x.ctu.as<int4>(), v->dev.max_chunks, d_count, &bound))) return rc;
  const uint32_t rank_grid = (uint32_t)std::min<size_t>(std::max<size_t>(blocks_of(bound, 256), 1), 2048);
  hipLaunchKernelGGL(k_tm_rank, dim3(rank_grid), dim3(256), 0, s, tm_dev(v), x.ctu.as<int4>(), d_count, v->dev.max_chunks, x.d_ctu);
  const uint32_t* d_n = &v->tm.ctl->n_list;
  // :356-361 (the keyframes to update travel through the words behind the keyframe table's rows: n_frames <= 12 in the reference)
  const int32_t* d_frames = nullptr;
  if (n_frames && (rc = tm_frames_upload(v, frames_to_update, n_frames, &d_frames))) return rc;
  if (bound && (rc = tm_update_enqueue(v, x.d_ctu, bound, d_n, frame_index, d_frames, n_frames))) return rc;
  if ((flags & TF_TAIL_CHECK_GRAPH) && (rc = tm_check_graph_enqueue(v))) return rc;
  TF_HIP(hipGetLastError());
  // :362-369; its control-block read is the call's one wait and brings the list's length along
  uint32_t list_n = 0;
  const TmWant want{nullptr, nullptr, nullptr, &list_n};
  const bool sub = (flags & TF_TAIL_SUB_PROBLEM) != 0;
  if ((rc = tm_select(v, sub ? x.d_ctu : nullptr, sub ? bound : 0, sub ? d_n : nullptr, max_rounds, want))) return rc;
  x.ctu_n = list_n;
  // :374-382 GeneratePatches with the labels just assigned, UpdateAtlas
  rc = patch_stage_device(v, x.d_ctu, list_n, &v->tm.ctl->first_fail);
  // :380 CompensateColor, enqueued: it reads what GeneratePatches wrote and nothing UpdateAtlas writes
  if (!rc && (flags & TF_TAIL_COMPENSATE_COLOR)) rc = cc_enqueue(v, nullptr);
  return rc;
}

int tf_texture_tail_list(tf_volume* v, int32_t* out_ids, int64_t cap, int64_t* n) {
  if (!v || !n || cap < 0 || (cap > 0 && !out_ids)) { set_error("invalid argument"); return TF_ERR_INVALID; }
  TF_DEV(v);
  const int64_t m = v->tmx.ctu_n;
  *n = m;
  if (!out_ids || !m) return TF_OK;
  if (m > cap) { set_error("output capacity too small"); return TF_ERR_CAPACITY; }
  std::vector<int32_t> h((size_t)m * 4);
  TF_HIP(hipStreamSynchronize(v->stream));
  TF_HIP(hipMemcpy(h.data(), v->tmx.d_ctu, (size_t)m * 16, hipMemcpyDeviceToHost));
  unpack_ids(h.data(), m, out_ids);
  return TF_OK;
}

int tf_texmap_download(tf_volume* v, const int32_t* ids, int64_t n, uint8_t* is_node, uint8_t* edges, int32_t* label,
                       int32_t* stored, int64_t* col_off, int32_t* col_frame, float* col_q, int64_t cap_entries) {
  if (!v || (n > 0 && !ids) || cap_entries < 0) { set_error("invalid argument"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (col_off) col_off[0] = 0;
  if (n <= 0) return TF_OK;
  if (!v->tm.node) {  // no map: nothing is a node
    for (int64_t i = 0; i < n; ++i) {
      if (is_node) is_node[i] = 0;
      if (edges) edges[i] = 0;
      if (label) label[i] = 0;
      if (stored) stored[i] = 0;
      if (col_off) col_off[i + 1] = 0;
    }
    return TF_OK;
  }
  const size_t rows = (size_t)std::max(v->tm.n_rows, 1);
  Layout L;
  L.take((size_t)n * 16);
  const size_t o_info = L.take((size_t)n * 16), o_f = L.take((size_t)n * rows * 4), o_q = L.take((size_t)n * rows * 4);
  Stage sg;
  int rc = stage_ids(v, v->scratch, L.size, ids, n, &sg);
  if (rc) return rc;
  hipLaunchKernelGGL(k_tm_download, dim3(wave_blocks((size_t)n)), dim3(256), 0, v->stream, tm_dev(v), sg.dp<const int4>(0), (uint32_t)n,
                     sg.dp<int32_t>(o_info), sg.dp<int32_t>(o_f), sg.dp<float>(o_q));
  TF_HIP(hipGetLastError());
  TF_HIP(hipMemcpyAsync(sg.h + o_info, sg.d + o_info, L.size - o_info, hipMemcpyDeviceToHost, v->stream));
  TF_HIP(hipStreamSynchronize(v->stream));
  const int32_t* info = sg.hp<const int32_t>(o_info);
  const int32_t* hf = sg.hp<const int32_t>(o_f);
  const float* hq = sg.hp<const float>(o_q);
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t w = (uint32_t)info[4 * i];
    if (is_node) is_node[i] = (uint8_t)(w & kTmNode);
    if (edges) edges[i] = (uint8_t)((w & kTmEdges) >> kTmEdgeShift);
    if (label) label[i] = info[4 * i + 1];
    if (stored) stored[i] = (w & kTmHadLabel) ? info[4 * i + 2] : -1;
    const int64_t K = info[4 * i + 3];
    if (col_frame || col_q) {
      if (at + K > cap_entries) { set_error("output capacity too small"); return TF_ERR_CAPACITY; }
      if (col_frame) memcpy(col_frame + at, hf + (size_t)i * rows, (size_t)K * 4);
      if (col_q) memcpy(col_q + at, hq + (size_t)i * rows, (size_t)K * 4);
    }
    at += K;
    if (col_off) col_off[i + 1] = at;
  }
  return TF_OK;
}

int tf_texmap_download_problem(tf_volume* v, int64_t cap_nodes, int64_t cap_nnz, int64_t* n_nodes, int64_t* nnz, int32_t* ids,
                               int32_t* nbr, int64_t* col_off, int32_t* labels, float* costs, int32_t* init_offsets,
                               int32_t* offsets) {
  if (!v || !n_nodes || !nnz) { set_error("null argument"); return TF_ERR_INVALID; }
  TF_DEV(v);
  const TexMapState& x = v->tmx;
  *n_nodes = x.n; *nnz = x.nnz;
  if (!x.n) return TF_OK;
  if (x.n > cap_nodes || x.nnz > cap_nnz) { set_error("output capacity too small"); return TF_ERR_CAPACITY; }
  const TmProb P = tm_prob(x);
  const size_t n = (size_t)x.n, z = (size_t)x.nnz;
  TF_HIP(hipStreamSynchronize(v->stream));
  if (ids) TF_HIP(hipMemcpy(ids, P.ids, 12 * n, hipMemcpyDeviceToHost));
  if (nbr) TF_HIP(hipMemcpy(nbr, P.nbr, 24 * n, hipMemcpyDeviceToHost));
  if (col_off) TF_HIP(hipMemcpy(col_off, P.col_off, 8 * (n + 1), hipMemcpyDeviceToHost));
  if (labels) TF_HIP(hipMemcpy(labels, P.labels, 4 * z, hipMemcpyDeviceToHost));
  if (costs) TF_HIP(hipMemcpy(costs, P.costs, 4 * z, hipMemcpyDeviceToHost));
  if (init_offsets) {
    int32_t r2[4] = {0, 0, 0, 0};
    TF_HIP(hipMemcpy(r2, P.rounds, 16, hipMemcpyDeviceToHost));
    if (r2[1] == 1) TF_HIP(hipMemcpy(init_offsets, P.init, 4 * n, hipMemcpyDeviceToHost));
    else for (size_t i = 0; i < n; ++i) init_offsets[i] = -1;  // a cold start: the cheapest label of every node
  }
  if (offsets) TF_HIP(hipMemcpy(offsets, P.off, 4 * n, hipMemcpyDeviceToHost));
  return TF_OK;
}

int tf_texmap_clear(tf_volume* v) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (!v->tm.node) return TF_OK;
  v->tmx.nodes_bound = 0;
  v->tmx.n = v->tmx.nnz = 0;
  return tm_fill(v);
}

}  // extern "C"
