// tf_align_tree.h -- the sums of one 8 x 8 tile of alignment rows, shared by the four aligners through tf_align_rows.h: the table
// of operand pairs, one level of the wave tree, and the tree itself (al_tree_sum), with the second pair table of the exposure
// row (tf_align_set_exposure; al_exposure_pairs, whose comment states its entry order) going through the same tree.  Device only; including files are built with
// -ffp-contract=off.  The order of every addition is fixed here (tf_align_rows.h's header comment states it).
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace tf {

constexpr int kAlSums = 31;  // A[21] b[6] sum_r2 sum_wr2 n_valid n_sampled
constexpr int kAlA = 0, kAlB = 21, kAlR2 = 27, kAlWr2 = 28, kAlNv = 29, kAlNs = 30;
constexpr int kAlRow = 32;  // doubles a tile's partial sums take (the 31 and one of padding)
constexpr int kAlWaves = 8;  // tiles (waves) of a workgroup of the rows kernels

// entry e of the sums = (double)left[kAlLeft[e]] * (double)right[kAlRight[e]] with
// left = {wJ_0..5, wr, r, valid, in}, right = {J_0..5, r, 1}
struct AlPairs { int l[32], r[32]; };
constexpr AlPairs al_pairs() {
  AlPairs p{};
  int e = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++e) { p.l[e] = i; p.r[e] = j; }
  for (int i = 0; i < 6; ++i, ++e) { p.l[e] = i; p.r[e] = 6; }
  p.l[kAlR2] = 7; p.r[kAlR2] = 6;
  p.l[kAlWr2] = 6; p.r[kAlWr2] = 6;
  p.l[kAlNv] = 8; p.r[kAlNv] = 7;
  p.l[kAlNs] = 9; p.r[kAlNs] = 7;
  p.l[31] = 9; p.r[31] = 7;
  return p;
}
constexpr AlPairs kAlPairs = al_pairs();
#define kAlLeft kAlPairs.l
#define kAlRight kAlPairs.r
// one level of the tree: a lane keeps the upper half of its N entries where bit o of its number is set, else the lower
// half, and adds the partner's (lane ^ o) values of the same entries
template <int N>
__device__ __forceinline__ void al_halve(double (&v)[16], int o, int lane) {
  const bool up = (lane & o) != 0;
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const double keep = up ? v[i + N / 2] : v[i], send = up ? v[i] : v[i + N / 2];
    v[i] = keep + __shfl_xor(send, o);
  }
}

// The tree over a tile's 32 entries, whatever the operands are: entry e is the f64 product of left operand tab.l[e] and right
// operand tab.r[e] (Lo, Ro: the lane's own; Lp, Rp: those of lane ^ 32).  Level 1 pairs lane l with l ^ 32: each of the two
// takes one half of the entries (bit 5 of the lane: entries 16..31) and adds its own term and its partner's, formed from
// the partner's operands.  Levels 2..5 (xor 16, 8, 4, 2) halve the entries a lane carries in the same way, level 6 (xor 1)
// adds the last pair: lane l ends up with entry al_entry(l) (bits 5, 4, 3, 2, 1 of l, most significant first; the lanes
// l and l ^ 1 hold the same).  Per entry this is the tree of ccd_wave_sum, each node computed once.
template <const AlPairs& tab, int NL, int NR>
__device__ __forceinline__ double al_tree_sum(const float (&Lo)[NL], const float (&Ro)[NR], const float (&Lp)[NL],
                                              const float (&Rp)[NR], int lane) {
  const bool hi = (lane & 32) != 0;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    // (both candidates are read by constant index before the choice, so that the operand arrays stay in registers)
    const float lo0 = Lo[tab.l[i]], lo1 = Lo[tab.l[i + 16]], ro0 = Ro[tab.r[i]], ro1 = Ro[tab.r[i + 16]];
    const float lp0 = Lp[tab.l[i]], lp1 = Lp[tab.l[i + 16]], rp0 = Rp[tab.r[i]], rp1 = Rp[tab.r[i + 16]];
    const float lo_own = hi ? lo1 : lo0, ro_own = hi ? ro1 : ro0, lo_par = hi ? lp1 : lp0, ro_par = hi ? rp1 : rp0;
    acc[i] = (double)lo_own * (double)ro_own + (double)lo_par * (double)ro_par;
  }
  al_halve<16>(acc, 16, lane);
  al_halve<8>(acc, 8, lane);
  al_halve<4>(acc, 4, lane);
  al_halve<2>(acc, 2, lane);
  return acc[0] + __shfl_xor(acc[0], 1);
}

// The 31 sums of the tile (a 32nd entry repeats n_sampled and is dropped) from each lane's row: J, weight w, residual r
// (all zero where the pixel is not valid), vf = valid, inf = inside the image, as 1.0f / 0.0f.  Entry e is the product of
// left operand kAlLeft[e] and right operand kAlRight[e], taken in f64, through al_tree_sum.
__device__ __forceinline__ double al_tile_sum(const float (&J)[6], float w, float r, float vf, float inf, int lane) {
  float Lo[10], Ro[8], Lp[10], Rp[8];
#pragma unroll
  for (int i = 0; i < 6; ++i) { Lo[i] = w * J[i]; Ro[i] = J[i]; }
  Lo[6] = w * r; Lo[7] = r; Lo[8] = vf; Lo[9] = inf; Ro[6] = r; Ro[7] = 1.0f;
#pragma unroll
  for (int i = 0; i < 10; ++i) Lp[i] = __shfl_xor(Lo[i], 32);
#pragma unroll
  for (int i = 0; i < 6; ++i) Rp[i] = __shfl_xor(Ro[i], 32);
  Rp[6] = Lp[7]; Rp[7] = 1.0f;
  return al_tree_sum<kAlPairs>(Lo, Ro, Lp, Rp, lane);
}

// The exposure row's sums of the tile (tf_align_set_exposure): the gain and offset columns of the photometric row against
// its Jacobian, themselves and its residual.  Operands, all of the photometric row and an exact zero where the pixel is not
// photometrically valid: left = {wJc_0..5, wc, wl = wc * Lf, valid}, right = {1, Lf, rc}.  Entry order:
//   0..5  P_i = wJc_i * 1      6..11 Q_i = wJc_i * Lf
//   12 S_w = wc * 1   13 S_l = wc * Lf   14 S_ll = wl * Lf   15 S_r = wc * rc   16 S_lr = wl * rc   17 n_photo = valid * 1
// (entries 18..31 repeat n_photo and are never read).
constexpr int kAlExpSums = 17;  // the sums a step reads; entry kAlExpN repeats n_photo
constexpr int kAlExpP = 0, kAlExpQ = 6, kAlExpSw = 12, kAlExpSl = 13, kAlExpSll = 14, kAlExpSr = 15, kAlExpSlr = 16, kAlExpN = 17;
constexpr AlPairs al_exposure_pairs() {
  AlPairs p{};
  for (int i = 0; i < 6; ++i) { p.l[kAlExpP + i] = i; p.r[kAlExpP + i] = 0; p.l[kAlExpQ + i] = i; p.r[kAlExpQ + i] = 1; }
  p.l[kAlExpSw] = 6; p.r[kAlExpSw] = 0;
  p.l[kAlExpSl] = 6; p.r[kAlExpSl] = 1;
  p.l[kAlExpSll] = 7; p.r[kAlExpSll] = 1;
  p.l[kAlExpSr] = 6; p.r[kAlExpSr] = 2;
  p.l[kAlExpSlr] = 7; p.r[kAlExpSlr] = 2;
  for (int e = kAlExpN; e < 32; ++e) { p.l[e] = 8; p.r[e] = 0; }
  return p;
}
constexpr AlPairs kAlExpPairs = al_exposure_pairs();
__device__ __forceinline__ double al_exposure_tile_sum(const float (&wJ)[6], float wc, float lf, float rc, float vf, int lane) {
  float Lo[9], Ro[3], Lp[9], Rp[3];
#pragma unroll
  for (int i = 0; i < 6; ++i) Lo[i] = wJ[i];
  Lo[6] = wc; Lo[7] = wc * lf; Lo[8] = vf; Ro[0] = 1.0f; Ro[1] = lf; Ro[2] = rc;
#pragma unroll
  for (int i = 0; i < 9; ++i) Lp[i] = __shfl_xor(Lo[i], 32);
  Rp[0] = 1.0f; Rp[1] = __shfl_xor(Ro[1], 32); Rp[2] = __shfl_xor(Ro[2], 32);
  return al_tree_sum<kAlExpPairs>(Lo, Ro, Lp, Rp, lane);
}
__device__ __forceinline__ int al_entry(int lane) {
  return ((lane >> 5) & 1) << 4 | ((lane >> 4) & 1) << 3 | ((lane >> 3) & 1) << 2 | ((lane >> 2) & 1) << 1 | ((lane >> 1) & 1);
}

}  // namespace tf
