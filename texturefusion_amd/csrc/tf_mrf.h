// tf_mrf.h -- what the view-selection solve (tf_mrf.hip) shares with the code that assembles its problem on the device
// (tf_texmap.hip): the argument block of its kernels, its scratch layout, how it is put on the stream and read back.
#pragma once

#include <stddef.h>

#include "tf_volume.h"

namespace tf {

constexpr int kMrfEnergyBlocks = 256;   // shape of the energy reduction: fixed, whatever n is
constexpr int kMrfDefaultRounds = 32;

struct MrfCtl {
  unsigned long long bad;  // min over the offending nodes of (node << 4 | code); ~0: the arguments are consistent
  int32_t done;            // a round changed nothing: every later launch of the solve returns at once
  int32_t changed;         // a line of the running round was rewritten
  uint32_t n_heads[6];     // [2 * axis + class]
  uint32_t top[3];         // line arrays: entries of order[axis] handed out
  int32_t pad[3];
};
static_assert(sizeof(MrfCtl) == 64, "MrfCtl");

struct MrfArgs {
  int32_t n;
  int64_t nnz;
  const int32_t* ids;
  const int32_t* nbr;
  const int64_t* col_off;
  const int32_t* labels;
  const float* costs;
  const int32_t* init;  // or null
  float w;
  int32_t* off;         // the labelling, as offsets (= out_offsets)
  double* energy;       // or null
  int32_t* rounds;
  MrfCtl* ctl;
  int32_t* cur;         // [n] label of every node under `off`
  int32_t* choice;      // [nnz] the table's back pointers
  int32_t* heads;       // [3][n] line heads of axis a: class 0 from the front, class 1 from the back
  double* partial;      // [kMrfEnergyBlocks]
  int32_t* order;       // line arrays: [3][n] the nodes of axis a in line order, or null = walk the +a pointers
  int4* line;           // [3][n] per head slot: {start in order[a], nodes, labels of all its nodes (saturated), 0}
};

// TF_MRF_WALK=pointers: walk the lines through the nodes' +a pointers instead of the line arrays
bool mrf_line_arrays();

struct MrfScratch {
  size_t ctl, cur, choice, heads, partial, order = 0, line = 0;
  bool arrays = false;
  void take(Layout& L, int64_t n, int64_t nnz) {
    arrays = mrf_line_arrays();
    ctl = L.take(sizeof(MrfCtl));
    cur = L.take(4 * (size_t)n);
    choice = L.take(4 * (size_t)nnz);
    heads = L.take(12 * (size_t)n);
    partial = L.take(8 * (size_t)kMrfEnergyBlocks);
    if (arrays) {
      order = L.take(12 * (size_t)n);
      line = L.take(48 * (size_t)n);
    }
  }
  void bind(MrfArgs& a, uint8_t* d) const {
    a.ctl = reinterpret_cast<MrfCtl*>(d + ctl);
    a.cur = reinterpret_cast<int32_t*>(d + cur);
    a.choice = reinterpret_cast<int32_t*>(d + choice);
    a.heads = reinterpret_cast<int32_t*>(d + heads);
    a.partial = reinterpret_cast<double*>(d + partial);
    a.order = arrays ? reinterpret_cast<int32_t*>(d + order) : nullptr;
    a.line = arrays ? reinterpret_cast<int4*>(d + line) : nullptr;
  }
};

struct MrfResult {     // what a solve's caller reads back, in pinned memory
  int32_t rounds[4];  // [0]: rounds run, -1 = the checking launch refused the problem
  MrfCtl ctl;
  double energy[1];   // [R + 1], of which [0 .. rounds] are written
  static size_t bytes(int R) { return offsetof(MrfResult, energy) + 8 * (size_t)(R + 1); }
};
// Every solve starts here.  `a` comes with the problem (n .. rounds, device pointers); the solver's scratch is laid out behind
// the first `at` bytes of the handle's pool (the caller's), the pool's device half reserved, the scratch members of `a`
// bound and the start put on the stream (mrf_enqueue_start).
int mrf_begin(tf_volume* v, MrfArgs& a, size_t at);
// the result of a solve of at most R rounds into h (pinned, MrfResult::bytes(R)); waits; MrfCtl::bad -> mrf_bad_to_error
int mrf_read_back(tf_volume* v, const MrfArgs& a, int R, MrfResult* h);
// the checking launch, the start labelling, the line arrays and the energy of round 0
int mrf_enqueue_start(tf_volume* v, const MrfArgs& a);
// rounds r0 .. r1 (1-based, inclusive); every launch is a no-op once the solve has ended
int mrf_enqueue_rounds(tf_volume* v, const MrfArgs& a, int r0, int r1);
// MrfCtl::bad -> tf_last_error text and the error code
int mrf_bad_to_error(unsigned long long bad);

}  // namespace tf
