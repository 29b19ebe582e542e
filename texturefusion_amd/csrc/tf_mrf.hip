// tf_mrf.hip -- TexMap::view_selection's solve (Structure/TexMap.cpp:199-225: mapMAP's optimize over the chunk graph) on the
// device: tf_view_select / tf_view_select_device.
//
// The problem is mapMAP's (3rd_party/mapmap/source/tree_optimizer.impl.h:158-192, pairwise_potts.impl.h:121-134):
//   E(x) = sum_i u_i(x_i) + w * sum_(i,j) [label_i != label_j]
// over the chunk graph, a subset of the 6-connected integer lattice.  The method is NOT mapMAP's (spanning-tree sampling,
// multilevel): it is block-coordinate descent over lattice lines.  A maximal run of nodes joined by +-a edges is a chain;
// with every off-line neighbour held fixed a chain is solved exactly by dynamic programming.  Two lines of axis a are
// coupled only when their other two coordinates differ by one step, so the lines whose other two coordinates have the
// same parity sum are independent and one launch updates all of them.  A round is six launches (x, y, z; class 0, 1);
// the solve ends after the first round that changes no label, or after max_rounds.  A line of length 1 is an ICM move.
//
// Per line (one wave, lanes over the labels of the node the wave stands on, in blocks of 64):
//   c_t(l) = u_t(l) + w * float(off-line neighbours whose label != l)
//   m_t(l) = c_t(l) + min(m_{t-1}(l) if l in L_{t-1}, M_{t-1} + w),  M = min m   (ties: the same label, then the lowest offset)
// one stored choice per (t, l), backtracked from the lowest-offset minimum of the last node.  The current labelling's value
// is accumulated with the same recurrence (the same f32 operations in the same order as its path through the table, so the
// table's minimum is never above it) and the line is rewritten only when the minimum is strictly smaller.
// Arithmetic: f32, no contraction (-ffp-contract=off); a lane sums sequentially along the line, every cross-lane operation
// is a min / argmin: nothing depends on a reduction order.  The energies of the trace come from a fixed-shape f64
// reduction (kEnergyBlocks x 256 partial sums in node-stride order, two LDS trees).  No float atomics.
//
// Nothing here reads or writes chunks, meshes, atlas or observations: the handle gives the stream and the scratch pool.
#include <float.h>
#include <stdlib.h>
#include <string.h>

#include "tf_mrf.h"
#include "tf_volume.h"

namespace tf {
namespace {

constexpr int kMaxLabels = 512;      // labels of one node (the previous node's row of the table lives in LDS)
constexpr int kEnergyBlocks = kMrfEnergyBlocks;
constexpr int kDefaultRounds = kMrfDefaultRounds;
constexpr int kPhaseBlocks = 4096;   // waves of a phase launch (they stride over the phase's line heads)
constexpr int kHostBatch = 4;        // host form: rounds enqueued between two looks at the control block
constexpr int kChoiceLds = 8192;     // line arrays: back pointers of a line kept in LDS when its table has at most this many entries

enum : uint32_t {
  kBadColumn = 1,    // empty column / col_off not ascending from 0 to nnz
  kBadLabels = 2,    // labels of a node not strictly ascending, or negative
  kBadInit = 3,      // init offset outside the node's label list
  kBadNbr = 4,       // nbr entry below -1 or >= n_nodes
  kBadSym = 5,       // nbr[nbr[i][k]][k ^ 1] != i
  kBadIds = 6,       // ids[nbr[i][k]] != ids[i] + d[k]
  kBadCost = 7,      // cost not finite
  kBadTooMany = 8,   // more than kMaxLabels labels
};

__device__ __forceinline__ bool mrf_live(const MrfCtl* c) { return c->bad == ~0ull && !c->done; }

// One cheap launch in front of everything: no later launch walks a graph this one has not found consistent.
__global__ __launch_bounds__(256) void k_mrf_validate(MrfArgs a) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= a.n) return;
  uint32_t code = 0;
  const int64_t c0 = a.col_off[i], c1 = a.col_off[i + 1];
  if (c0 < 0 || c1 <= c0 || c1 > a.nnz || (i == 0 && c0 != 0) || (i == a.n - 1 && c1 != a.nnz)) {
    code = kBadColumn;
  } else if (c1 - c0 > kMaxLabels) {
    code = kBadTooMany;
  } else {
    int prev = -1;
    for (int64_t j = c0; j < c1; ++j) {
      const int l = a.labels[j];
      if (l <= prev && !code) code = kBadLabels;
      prev = l;
      if (!(fabsf(a.costs[j]) <= FLT_MAX) && !code) code = kBadCost;
    }
    if (!code && a.init) {
      const int o = a.init[i];
      if (o < 0 || o >= c1 - c0) code = kBadInit;
    }
  }
  for (int k = 0; k < 6 && !code; ++k) {
    const int nb = a.nbr[6 * i + k];
    if (nb == -1) continue;
    if (nb < 0 || nb >= a.n) { code = kBadNbr; break; }
    if (a.nbr[6 * nb + (k ^ 1)] != i) { code = kBadSym; break; }
    const int ax = k >> 1, d = (k & 1) ? 1 : -1;
    for (int c = 0; c < 3; ++c)
      if (a.ids[3 * nb + c] != a.ids[3 * i + c] + (c == ax ? d : 0)) code = kBadIds;
  }
  if (code) atomicMin(&a.ctl->bad, ((unsigned long long)i << 4) | code);
}

// Start labelling (init, or the cheapest label, lowest offset) and the line heads: the nodes without a -a neighbour.
__global__ __launch_bounds__(256) void k_mrf_init(MrfArgs a) {
  if (!mrf_live(a.ctl)) return;
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= a.n) return;
  const int64_t c0 = a.col_off[i];
  int o = 0;
  if (a.init) {
    o = a.init[i];
  } else {
    const int K = (int)(a.col_off[i + 1] - c0);
    float best = a.costs[c0];
    for (int j = 1; j < K; ++j) {
      const float u = a.costs[c0 + j];
      if (u < best) { best = u; o = j; }
    }
  }
  a.off[i] = o;
  a.cur[i] = a.labels[c0 + o];
  for (int ax = 0; ax < 3; ++ax) {
    if (a.nbr[6 * i + 2 * ax] != -1) continue;
    const int cls = (a.ids[3 * i + (ax + 1) % 3] + a.ids[3 * i + (ax + 2) % 3]) & 1;
    const uint32_t p = atomicAdd(&a.ctl->n_heads[2 * ax + cls], 1u);  // (the order of a class's heads is free: its lines are independent)
    a.heads[(int64_t)ax * a.n + (cls ? (uint32_t)a.n - 1u - p : p)] = i;
  }
}

// Where a wave stands on its line: the previous node's row of the table is in LDS row buf ^ 1.
struct LineState {
  int buf = 0, Kp = 0, argp = 0, labp = -1;
  float Mp = 0.f, e = 0.f;
  bool first = true;
};
// What the step needs of the node: its column, its offset and label under the current labelling, the labels of its four
// off-line neighbours (-1: no neighbour; labels are >= 0).  All wave-uniform.
struct NodeIn {
  int64_t c0;
  int K, co, lc, l0, l1, l2, l3;
};

// One node of the forward pass; both walking variants run exactly this.  pre: lanes below K hold the node's first 64
// labels / costs already (pl, pu).  s_c: the back pointers go to LDS at cbase (the line's fit) instead of a.choice.
__device__ __forceinline__ void mrf_node(const MrfArgs& a, float (*s_m)[kMaxLabels], int32_t (*s_l)[kMaxLabels], uint16_t* s_c,
                                         int cbase, int lane, const NodeIn& nd, bool pre, int pl, float pu, LineState& S) {
  const float w = a.w;
  const int buf = S.buf, pb = buf ^ 1;
  float lmin = INFINITY, c_cur = 0.f;
  int lidx = 0x7fffffff;
  for (int j = lane; j < nd.K; j += 64) {
    const int l = (pre && j < 64) ? pl : a.labels[nd.c0 + j];
    const float u = (pre && j < 64) ? pu : a.costs[nd.c0 + j];
    const int cnt = (int)(nd.l0 >= 0 && nd.l0 != l) + (int)(nd.l1 >= 0 && nd.l1 != l) + (int)(nd.l2 >= 0 && nd.l2 != l) +
                    (int)(nd.l3 >= 0 && nd.l3 != l);
    const float c = u + w * (float)cnt;
    float m = c;
    int ch = 0;
    if (!S.first) {
      float best = S.Mp + w;
      ch = S.argp;
      int lo = 0, hi = S.Kp;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_l[pb][mid] < l) lo = mid + 1; else hi = mid;
      }
      if (lo < S.Kp && s_l[pb][lo] == l) {
        const float st = s_m[pb][lo];
        if (st <= best) { best = st; ch = lo; }
      }
      m = c + best;
    }
    s_m[buf][j] = m;
    s_l[buf][j] = l;
    if (s_c) s_c[cbase + j] = (uint16_t)ch; else a.choice[nd.c0 + j] = ch;
    if (m < lmin) { lmin = m; lidx = j; }
    if (j == nd.co) c_cur = c;
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    const float ov = __shfl_xor(lmin, d);
    const int oi = __shfl_xor(lidx, d);
    if (ov < lmin || (ov == lmin && oi < lidx)) { lmin = ov; lidx = oi; }
  }
  const float cc = __shfl(c_cur, nd.co & 63);
  S.e = S.first ? cc : cc + (nd.lc == S.labp ? S.e : S.e + w);
  S.Mp = lmin; S.argp = lidx; S.Kp = nd.K; S.labp = nd.lc; S.first = false; S.buf = pb;
  __syncthreads();  // one wave: orders this node's LDS row against the next node's reads
}

#define MRF_RFL(x) __builtin_amdgcn_readfirstlane(x)

// One wave per line of axis AXIS and class cls, the line walked through the nodes' +a pointers: two dependent round trips
// per node forwards (the node's row, then what it points to), two backwards.
template <int AXIS>
__global__ __launch_bounds__(64) void k_mrf_phase(MrfArgs a, int cls) {
  __shared__ float s_m[2][kMaxLabels];
  __shared__ int32_t s_l[2][kMaxLabels];
  if (!mrf_live(a.ctl)) return;
  constexpr int KM = 2 * AXIS, KP = 2 * AXIS + 1;
  constexpr int O0 = (KM + 2) % 6, O1 = (KM + 3) % 6, O2 = (KM + 4) % 6, O3 = (KM + 5) % 6;  // the four off-line faces
  const uint32_t nh = a.ctl->n_heads[2 * AXIS + cls];
  const int lane = (int)threadIdx.x;
  for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
    int t = MRF_RFL(a.heads[(int64_t)AXIS * a.n + (cls ? (uint32_t)a.n - 1u - h : h)]);
    int tail = t;
    LineState S;
    while (t >= 0) {
      const int32_t* row = a.nbr + 6 * (int64_t)t;
      const int next = MRF_RFL(row[KP]);
      const int n0 = MRF_RFL(row[O0]), n1 = MRF_RFL(row[O1]), n2 = MRF_RFL(row[O2]), n3 = MRF_RFL(row[O3]);
      NodeIn nd;
      nd.c0 = a.col_off[t];
      nd.K = MRF_RFL((int)(a.col_off[t + 1] - nd.c0));
      nd.co = MRF_RFL(a.off[t]);
      nd.lc = MRF_RFL(a.cur[t]);
      nd.l0 = n0 >= 0 ? a.cur[n0] : -1; nd.l1 = n1 >= 0 ? a.cur[n1] : -1;
      nd.l2 = n2 >= 0 ? a.cur[n2] : -1; nd.l3 = n3 >= 0 ? a.cur[n3] : -1;
      mrf_node(a, s_m, s_l, nullptr, 0, lane, nd, false, 0, 0.f, S);
      tail = t; t = next;
    }
    if (S.Mp < S.e) {
      __threadfence();  // the back pointers are read back by other lanes than wrote them: coherent loads behind a fence
      int j = S.argp;
      t = tail;
      while (t >= 0) {
        const int64_t c0 = a.col_off[t];
        const int jp = __hip_atomic_load(&a.choice[c0 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) { a.off[t] = j; a.cur[t] = a.labels[c0 + j]; }
        j = MRF_RFL(jp);
        t = MRF_RFL(a.nbr[6 * (int64_t)t + KM]);
      }
      if (lane == 0) a.ctl->changed = 1;
    }
  }
}

// ---- line arrays: per axis the nodes in line order, built once per solve -------------------------------------------
// One thread per head slot of the three head lists: a first walk for the line's length and label count, room for it out
// of the axis' counter, a second walk that writes the nodes down.  (Where a line lands in the array is free.)
__global__ __launch_bounds__(256) void k_mrf_lines(MrfArgs a) {
  if (!mrf_live(a.ctl)) return;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 3 * (int64_t)a.n) return;
  const int ax = (int)(idx / a.n);
  const uint32_t s = (uint32_t)(idx % a.n);
  if (!(s < a.ctl->n_heads[2 * ax] || s >= (uint32_t)a.n - a.ctl->n_heads[2 * ax + 1])) return;
  const int head = a.heads[idx];
  uint32_t len = 0;
  int64_t tot = 0;
  for (int t = head; t >= 0; t = a.nbr[6 * (int64_t)t + 2 * ax + 1]) {
    ++len;
    tot += a.col_off[t + 1] - a.col_off[t];
  }
  const uint32_t start = atomicAdd(&a.ctl->top[ax], len);
  int32_t* o = a.order + (int64_t)ax * a.n + start;
  for (int t = head; t >= 0; t = a.nbr[6 * (int64_t)t + 2 * ax + 1]) *o++ = t;
  a.line[idx] = make_int4((int)start, (int)len, tot > 0x7fffffff ? 0x7fffffff : (int)tot, 0);
}

// The same line solve over the line arrays: a wave loads what the step needs of 64 nodes at a time, one node per lane --
// three dependent round trips per 64 nodes instead of two per node -- and the labels / costs of the next node while it
// works on this one; a line whose table has at most kChoiceLds entries keeps its back pointers in LDS, so that the
// backward pass is free of memory round trips as well.
template <int AXIS>
__global__ __launch_bounds__(64) void k_mrf_phase_lines(MrfArgs a, int cls) {
  __shared__ float s_m[2][kMaxLabels];
  __shared__ int32_t s_l[2][kMaxLabels];
  __shared__ uint16_t s_c[kChoiceLds];
  if (!mrf_live(a.ctl)) return;
  constexpr int KM = 2 * AXIS;
  constexpr int O0 = (KM + 2) % 6, O1 = (KM + 3) % 6, O2 = (KM + 4) % 6, O3 = (KM + 5) % 6;
  const uint32_t nh = a.ctl->n_heads[2 * AXIS + cls];
  const int lane = (int)threadIdx.x;
  for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
    const int4 ln = a.line[(int64_t)AXIS * a.n + (cls ? (uint32_t)a.n - 1u - h : h)];
    const int32_t* ord = a.order + (int64_t)AXIS * a.n + MRF_RFL(ln.x);
    const int len = MRF_RFL(ln.y);
    const bool in_lds = MRF_RFL(ln.z) <= kChoiceLds;
    LineState S;
    int cbase = 0;
    for (int p0 = 0; p0 < len; p0 += 64) {
      // this lane's node of the block
      const bool have = p0 + lane < len;
      const int t = have ? ord[p0 + lane] : 0;
      const int32_t* row = a.nbr + 6 * (int64_t)t;
      const int n0 = have ? row[O0] : -1, n1 = have ? row[O1] : -1, n2 = have ? row[O2] : -1, n3 = have ? row[O3] : -1;
      const int64_t v_c0 = a.col_off[t];
      const int v_K = (int)(a.col_off[t + 1] - v_c0);
      const int v_co = a.off[t], v_lc = a.cur[t];
      const int v_l0 = n0 >= 0 ? a.cur[n0] : -1, v_l1 = n1 >= 0 ? a.cur[n1] : -1;
      const int v_l2 = n2 >= 0 ? a.cur[n2] : -1, v_l3 = n3 >= 0 ? a.cur[n3] : -1;
      const int cnt = len - p0 < 64 ? len - p0 : 64;
      // the first node's labels / costs; each step then fetches the next node's while it works
      int64_t c0n = ((int64_t)__builtin_amdgcn_readlane((int)(v_c0 >> 32), 0) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v_c0, 0);
      int Kn = __builtin_amdgcn_readlane(v_K, 0);
      int pl = lane < Kn ? a.labels[c0n + lane] : 0;
      float pu = lane < Kn ? a.costs[c0n + lane] : 0.f;
      for (int i = 0; i < cnt; ++i) {
        NodeIn nd;
        nd.c0 = c0n; nd.K = Kn;
        nd.co = __builtin_amdgcn_readlane(v_co, i); nd.lc = __builtin_amdgcn_readlane(v_lc, i);
        nd.l0 = __builtin_amdgcn_readlane(v_l0, i); nd.l1 = __builtin_amdgcn_readlane(v_l1, i);
        nd.l2 = __builtin_amdgcn_readlane(v_l2, i); nd.l3 = __builtin_amdgcn_readlane(v_l3, i);
        const int cl = pl;
        const float cu = pu;
        if (i + 1 < cnt) {
          c0n = ((int64_t)__builtin_amdgcn_readlane((int)(v_c0 >> 32), i + 1) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v_c0, i + 1);
          Kn = __builtin_amdgcn_readlane(v_K, i + 1);
          pl = lane < Kn ? a.labels[c0n + lane] : 0;
          pu = lane < Kn ? a.costs[c0n + lane] : 0.f;
        }
        mrf_node(a, s_m, s_l, in_lds ? s_c : nullptr, cbase, lane, nd, true, cl, cu, S);
        cbase += nd.K;
      }
    }
    if (S.Mp < S.e) {
      if (!in_lds) __threadfence();
      int j = S.argp;
      for (int p0 = ((len - 1) >> 6) << 6; p0 >= 0; p0 -= 64) {
        const bool have = p0 + lane < len;
        const int t = have ? ord[p0 + lane] : 0;
        const int64_t v_c0 = a.col_off[t];
        const int v_K = (int)(a.col_off[t + 1] - v_c0);
        const int cnt = len - p0 < 64 ? len - p0 : 64;
        int myj = 0;
        for (int i = cnt - 1; i >= 0; --i) {
          if (lane == i) myj = j;
          const int K = __builtin_amdgcn_readlane(v_K, i);
          cbase -= K;
          if (in_lds) {
            j = MRF_RFL((int)s_c[cbase + j]);
          } else {
            const int64_t c0 = ((int64_t)__builtin_amdgcn_readlane((int)(v_c0 >> 32), i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v_c0, i);
            j = MRF_RFL(__hip_atomic_load(&a.choice[c0 + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          }
        }
        if (have) { a.off[t] = myj; a.cur[t] = a.labels[v_c0 + myj]; }
      }
      if (lane == 0) a.ctl->changed = 1;
    }
  }
}

__device__ __forceinline__ double block_sum_256(double s, double* sh) {
  const int t = (int)threadIdx.x;
  sh[t] = s;
  __syncthreads();
  for (int d = 128; d; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void k_mrf_energy(MrfArgs a) {
  __shared__ double sh[256];
  if (!mrf_live(a.ctl)) return;
  double s = 0.0;
  const double w = (double)a.w;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)kEnergyBlocks * 256) {
    s += (double)a.costs[a.col_off[i] + a.off[i]];
    const int my = a.cur[i];
    for (int k = 1; k < 6; k += 2) {  // every edge once: from its -a end
      const int nb = a.nbr[6 * i + k];
      if (nb >= 0 && a.cur[nb] != my) s += w;
    }
  }
  s = block_sum_256(s, sh);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = s;
}

// round 0 = the start labelling.  Ends the solve when the round changed nothing.
__global__ __launch_bounds__(256) void k_mrf_round_end(MrfArgs a, int round) {
  __shared__ double sh[256];
  if (!mrf_live(a.ctl)) return;
  static_assert(kEnergyBlocks == 256, "one partial sum per thread");
  const double s = block_sum_256(a.partial[threadIdx.x], sh);
  if (threadIdx.x) return;
  if (a.energy) a.energy[round] = s;
  *a.rounds = round;
  if (round) {
    if (!a.ctl->changed) a.ctl->done = 1;
    a.ctl->changed = 0;
  }
}

int mrf_check(tf_volume* v, int64_t n, const void* ids, const void* nbr, const void* col_off, const void* labels,
              const void* costs, float edge_cost, int32_t max_rounds, const void* out_offsets, const void* out_rounds) {
  if (!v) { set_error("null handle"); return TF_ERR_INVALID; }
  if (n < 0) { set_error("view selection: n_nodes < 0"); return TF_ERR_INVALID; }
  if (max_rounds < 0) { set_error("view selection: max_rounds < 0"); return TF_ERR_INVALID; }
  if (!(edge_cost >= 0.f) || !(edge_cost <= FLT_MAX)) { set_error("view selection: edge_cost must be finite and >= 0"); return TF_ERR_INVALID; }
  if (n == 0) return TF_OK;
  if (!ids || !nbr || !col_off || !labels || !costs || !out_offsets || !out_rounds) { set_error("null argument"); return TF_ERR_INVALID; }
  if (n > (int64_t)1 << 27) { set_error("view selection: more than 2^27 nodes"); return TF_ERR_CAPACITY; }
  return TF_OK;
}

}  // namespace

// TF_MRF_WALK=pointers: walk the lines through the nodes' +a pointers instead of the line arrays (tools/view_selection_time.py
// measures both; DESIGN.md s.7d has the numbers the default rests on).  Both give the same bytes.
bool mrf_line_arrays() {
  const char* e = getenv("TF_MRF_WALK");
  return !(e && strcmp(e, "pointers") == 0);
}

int mrf_begin(tf_volume* v, MrfArgs& a, size_t at) {
  Layout L{at};
  MrfScratch sc;
  sc.take(L, a.n, a.nnz);
  if (int rc = reserve(v, v->scratch, L.size, 0)) return rc;
  sc.bind(a, v->scratch.d.as<uint8_t>());
  return mrf_enqueue_start(v, a);
}

int mrf_read_back(tf_volume* v, const MrfArgs& a, int R, MrfResult* h) {
  hipStream_t s = v->stream;
  TF_HIP(hipMemcpyAsync(h->rounds, a.rounds, sizeof(h->rounds), hipMemcpyDeviceToHost, s));
  TF_HIP(hipMemcpyAsync(&h->ctl, a.ctl, sizeof(MrfCtl), hipMemcpyDeviceToHost, s));
  TF_HIP(hipMemcpyAsync(h->energy, a.energy, 8 * (size_t)(R + 1), hipMemcpyDeviceToHost, s));
  TF_HIP(hipStreamSynchronize(s));
  return h->ctl.bad != ~0ull ? mrf_bad_to_error(h->ctl.bad) : TF_OK;
}

int mrf_enqueue_start(tf_volume* v, const MrfArgs& a) {
  hipStream_t s = v->stream;
  TF_HIP(hipMemsetAsync(a.ctl, 0, sizeof(MrfCtl), s));
  TF_HIP(hipMemsetAsync(&a.ctl->bad, 0xFF, sizeof(a.ctl->bad), s));
  const unsigned nb = (unsigned)((a.n + 255) / 256);
  hipLaunchKernelGGL(k_mrf_validate, dim3(nb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mrf_init, dim3(nb), dim3(256), 0, s, a);
  if (a.order) hipLaunchKernelGGL(k_mrf_lines, dim3((unsigned)((3 * (int64_t)a.n + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mrf_energy, dim3(kEnergyBlocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mrf_round_end, dim3(1), dim3(256), 0, s, a, 0);
  TF_HIP(hipGetLastError());
  return TF_OK;
}

// rounds r0 .. r1 (1-based, inclusive); every launch is a no-op once the solve has ended
int mrf_enqueue_rounds(tf_volume* v, const MrfArgs& a, int r0, int r1) {
  hipStream_t s = v->stream;
  const unsigned g = (unsigned)(a.n < kPhaseBlocks ? a.n : kPhaseBlocks);
  for (int r = r0; r <= r1; ++r) {
    if (a.order) {
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase_lines<0>, dim3(g), dim3(64), 0, s, a, cls);
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase_lines<1>, dim3(g), dim3(64), 0, s, a, cls);
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase_lines<2>, dim3(g), dim3(64), 0, s, a, cls);
    } else {
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase<0>, dim3(g), dim3(64), 0, s, a, cls);
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase<1>, dim3(g), dim3(64), 0, s, a, cls);
      for (int cls = 0; cls < 2; ++cls) hipLaunchKernelGGL(k_mrf_phase<2>, dim3(g), dim3(64), 0, s, a, cls);
    }
    hipLaunchKernelGGL(k_mrf_energy, dim3(kEnergyBlocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_mrf_round_end, dim3(1), dim3(256), 0, s, a, r);
  }
  TF_HIP(hipGetLastError());
  return TF_OK;
}

int mrf_bad_to_error(unsigned long long bad) {
  const long long node = (long long)(bad >> 4);
  const uint32_t code = (uint32_t)(bad & 15u);
  static const char* const what[] = {
      "", "has an empty column (col_off must ascend from 0 to nnz)", "has labels that are not strictly ascending and >= 0",
      "has an init offset outside its label list", "has a nbr entry that is neither -1 nor a node index",
      "has a neighbour that does not point back (nbr[nbr[i][k]][k ^ 1] != i)",
      "has a neighbour whose chunk id is not its own plus the face's step", "has a cost that is not finite",
      "has more than 512 labels"};
  set_error("view selection: node " + std::to_string(node) + " " + (code < 9 ? what[code] : "is inconsistent"));
  return code == kBadTooMany ? TF_ERR_CAPACITY : TF_ERR_INVALID;
}

}  // namespace tf

using namespace tf;

extern "C" {

int tf_view_select_device(tf_volume* v, int64_t n_nodes, const int32_t* d_ids, const int32_t* d_nbr, const int64_t* d_col_off,
                          int64_t nnz, const int32_t* d_labels, const float* d_costs, float edge_cost,
                          const int32_t* d_init_offsets, int32_t max_rounds, int32_t* d_out_offsets, double* d_out_energy,
                          int32_t* d_out_rounds) {
  int rc = mrf_check(v, n_nodes, d_ids, d_nbr, d_col_off, d_labels, d_costs, edge_cost, max_rounds, d_out_offsets, d_out_rounds);
  if (rc) return rc;
  if (n_nodes && nnz < n_nodes) { set_error("view selection: nnz < n_nodes (a column would be empty)"); return TF_ERR_INVALID; }
  TF_DEV(v);
  if (n_nodes == 0) return TF_OK;
  MrfArgs a{};
  a.n = (int32_t)n_nodes; a.nnz = nnz; a.ids = d_ids; a.nbr = d_nbr; a.col_off = d_col_off; a.labels = d_labels;
  a.costs = d_costs; a.init = d_init_offsets; a.w = edge_cost; a.off = d_out_offsets; a.energy = d_out_energy;
  a.rounds = d_out_rounds;
  if ((rc = mrf_begin(v, a, 0))) return rc;
  return mrf_enqueue_rounds(v, a, 1, max_rounds ? max_rounds : kDefaultRounds);
}

int tf_view_select(tf_volume* v, int64_t n_nodes, const int32_t* ids, const int32_t* nbr, const int64_t* col_off,
                   const int32_t* labels, const float* costs, float edge_cost, const int32_t* init_offsets, int32_t max_rounds,
                   int32_t* out_offsets, double* out_energy, int32_t* out_rounds) {
  int rc = mrf_check(v, n_nodes, ids, nbr, col_off, labels, costs, edge_cost, max_rounds, out_offsets, out_rounds);
  if (rc) return rc;
  TF_DEV(v);
  if (n_nodes == 0) return TF_OK;
  const size_t n = (size_t)n_nodes;
  // the lengths of labels / costs come from col_off: it is looked at here, everything else on the device
  for (size_t i = 0; i < n; ++i)
    if (col_off[i] < 0 || col_off[i + 1] <= col_off[i] || (i == 0 && col_off[0] != 0))
      return mrf_bad_to_error(((unsigned long long)i << 4) | kBadColumn);
  const int64_t nnz = col_off[n];
  const int R = max_rounds ? max_rounds : kDefaultRounds;
  // staging: rounds, ctl copy, energy trace (MrfResult) | offsets || ids | nbr | col_off | labels | costs | init || device scratch
  Layout L;
  const size_t o_res = L.take(MrfResult::bytes(R)), o_off = L.take(4 * n);
  const size_t o_ids = L.take(12 * n), o_nbr = L.take(24 * n), o_co = L.take(8 * (n + 1)), o_l = L.take(4 * (size_t)nnz),
               o_u = L.take(4 * (size_t)nnz), o_i = L.take(init_offsets ? 4 * n : 0);
  const size_t host_end = L.size;
  MrfScratch().take(L, n_nodes, nnz);  // (mrf_begin lays it out at host_end again: the pool is reserved for all of it here)
  Stage sg;
  if ((rc = stage_begin(v, v->scratch, L.size, host_end, &sg)) || (rc = stage_in(v, sg, o_ids, ids, 12 * n)) ||
      (rc = stage_in(v, sg, o_nbr, nbr, 24 * n)) || (rc = stage_in(v, sg, o_co, col_off, 8 * (n + 1))) ||
      (rc = stage_in(v, sg, o_l, labels, 4 * (size_t)nnz)) || (rc = stage_in(v, sg, o_u, costs, 4 * (size_t)nnz)) ||
      (init_offsets && (rc = stage_in(v, sg, o_i, init_offsets, 4 * n))))
    return rc;
  MrfResult* res = sg.hp<MrfResult>(o_res);
  MrfArgs a{};
  a.n = (int32_t)n_nodes; a.nnz = nnz; a.ids = sg.dp<const int32_t>(o_ids); a.nbr = sg.dp<const int32_t>(o_nbr);
  a.col_off = sg.dp<const int64_t>(o_co); a.labels = sg.dp<const int32_t>(o_l); a.costs = sg.dp<const float>(o_u);
  a.init = init_offsets ? sg.dp<const int32_t>(o_i) : nullptr; a.w = edge_cost; a.off = sg.dp<int32_t>(o_off);
  a.energy = sg.dp<MrfResult>(o_res)->energy; a.rounds = sg.dp<MrfResult>(o_res)->rounds;
  if ((rc = mrf_begin(v, a, host_end))) return rc;
  // the host form waits for the result anyway: it looks at the control block every kHostBatch rounds and stops
  // enqueueing once the solve has ended (the launches behind the end would all return at once)
  for (int r = 1;; r += kHostBatch) {
    TF_HIP(hipMemcpyAsync(&res->ctl, a.ctl, sizeof(MrfCtl), hipMemcpyDeviceToHost, v->stream));
    TF_HIP(hipStreamSynchronize(v->stream));
    if (res->ctl.bad != ~0ull) return mrf_bad_to_error(res->ctl.bad);
    if (res->ctl.done || r > R) break;
    if ((rc = mrf_enqueue_rounds(v, a, r, r + kHostBatch - 1 < R ? r + kHostBatch - 1 : R))) return rc;
  }
  TF_HIP(hipMemcpyAsync(sg.h + o_off, a.off, 4 * n, hipMemcpyDeviceToHost, v->stream));
  if ((rc = mrf_read_back(v, a, R, res))) return rc;
  const int32_t rounds = res->rounds[0];
  memcpy(out_offsets, sg.h + o_off, 4 * n);
  if (out_energy) memcpy(out_energy, res->energy, 8 * (size_t)(rounds + 1));
  *out_rounds = rounds;
  return TF_OK;
}

}  // extern "C"
