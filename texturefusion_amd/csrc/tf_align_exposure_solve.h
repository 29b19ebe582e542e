// tf_align_exposure_solve.h -- the exposure pair (gain, offset) of the photometric aligners eliminated ahead of the shared
// 6 x 6 solve, and its own step afterwards: one text for the device (al_solve_color_exposure, tf_align_rows.h) and for host
// programs (tests/cpp_align_exposure/exposure_solve_print.cpp).  Everything is f64 with -ffp-contract=off.  Every loop has
// a constant trip count and is unrolled, so that on the device the arrays live in registers (tf_cc_solve.h says why).
//
// The photometric residual is rc = L - (gain * Lf + offset): its derivative by the offset is -1, by the gain -Lf.  With the
// 17 sums S of the exposure row (tf_align_tree.h: P[6] Q[6] S_w S_l S_ll S_r S_lr) the photometric normal equations in
// (xi, offset, gain) are
//   [ Ac   -C ] [ xi ]     [ bc ]
//   [ -C^T  F ] [ de ] = - [ -h ],   F = [[S_w, S_l], [S_l, S_ll]],  C = [P Q] (6 x 2),  h = (S_r, S_lr).
// The unknowns are ordered (offset, gain): the first pivot is the weight sum, the second the weighted variance of Lf.
//   thresh = 1e-12 * max(S_w, S_ll);  rank = 0
//   unknowns >= 1 and S_w > thresh:  rank = 1, l00 = sqrt(S_w)
//   unknowns == 2 and rank == 1:     l10 = S_l / l00, p1 = S_ll - l10 * l10;  p1 > max(thresh, 2^-23 * S_ll): rank = 2,
//                                    l11 = sqrt(p1)
// (The second bound: wl = wc * Lf is rounded to f32, so S_ll carries an error of up to 2^-24 * S_ll whatever the frame shows.
// On a frame of one grey level with Huber weights below 1 the second pivot is that error alone, of either sign and nine
// orders above 1e-12; a pivot below twice the bound says nothing about the gain.)
//   Y = L^-1 C_k^T (k x 6), z = L^-1 h_k by forward substitution, k = rank:
//     Y[0][i] = P_i / l00, z[0] = S_r / l00;  Y[1][i] = (Q_i - l10 * Y[0][i]) / l11, z[1] = (S_lr - l10 * z[0]) / l11
//   Ac'[ij] = Ac[ij] - sum_k Y[k][i] * Y[k][j],  bc'[i] = bc[i] - sum_k Y[k][i] * z[k]   (ascending k, one subtraction each)
// A row of Y and an entry of z beyond the rank are exact zeros, so that with rank 0 Ac' = Ac and bc' = bc bit for bit.
// After the 6 x 6 solve has given xi:
//   t_k = h_k + sum_i C[i][k] * xi[i]   (t = h_k, then one addition per i in ascending order)
//   de = L^-T L^-1 t:  u0 = t0 / l00;  rank 2: u1 = (t1 - l10 * u0) / l11, de1 = u1 / l11, de0 = (u0 - l10 * de1) / l00;
//   rank 1: de0 = u0 / l00, de1 = 0;  rank 0: de = 0
//   offset += de0 (rank >= 1);  gain = min(max(gain + de1, min_gain), max_gain) (rank == 2)
#pragma once

#include <math.h>

#include "tf_align_solve.h"

namespace tf {

constexpr double kExposurePivot = 1e-12;  // relative to the larger of the two diagonal entries
constexpr double kExposureVariance = 1.0 / 8388608.0;  // 2^-23 of S_ll: twice the f32 rounding wl = wc * Lf can put into S_ll
// the 17 sums in the order of the exposure row (tf_align_tree.h's kAlExp*)
constexpr int kExpP = 0, kExpQ = 6, kExpSw = 12, kExpSl = 13, kExpSll = 14, kExpSr = 15, kExpSlr = 16, kExpSums = 17;

struct ExposureElim {
  int rank;
  double l00, l10, l11;  // 1, 0, 1 beyond the rank
  double Y[2][6], z[2];  // zero beyond the rank
};

// The elimination: Ac (21 upper entries, tf_align_solve.h's order) and bc become Ac' and bc' in place.
TF_AL_HD inline void exposure_eliminate(const double S[17], int unknowns, double Ac[21], double bc[6], ExposureElim* e) {
  const double sw = S[kExpSw], sl = S[kExpSl], sll = S[kExpSll];
  const double thresh = kExposurePivot * (sw > sll ? sw : sll);
  int rank = 0;
  double l00 = 1.0, l10 = 0.0, l11 = 1.0;
  if (unknowns >= 1 && sw > thresh) { rank = 1; l00 = sqrt(sw); }
  if (unknowns == 2 && rank == 1) {
    const double t10 = sl / l00, p1 = sll - t10 * t10;
    const double floor2 = kExposureVariance * sll;
    if (p1 > (thresh > floor2 ? thresh : floor2)) { rank = 2; l10 = t10; l11 = sqrt(p1); }
  }
  e->rank = rank; e->l00 = l00; e->l10 = l10; e->l11 = l11;
  e->z[0] = rank >= 1 ? S[kExpSr] / l00 : 0.0;
  e->z[1] = rank == 2 ? (S[kExpSlr] - l10 * e->z[0]) / l11 : 0.0;
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) {
    e->Y[0][i] = rank >= 1 ? S[kExpP + i] / l00 : 0.0;
    e->Y[1][i] = rank == 2 ? (S[kExpQ + i] - l10 * e->Y[0][i]) / l11 : 0.0;
  }
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) {
    TF_AL_UNROLL
    for (int j = i; j < 6; ++j) {
      const int u = align_upper(i, j);
      Ac[u] = (Ac[u] - e->Y[0][i] * e->Y[0][j]) - e->Y[1][i] * e->Y[1][j];
    }
    bc[i] = (bc[i] - e->Y[0][i] * e->z[0]) - e->Y[1][i] * e->z[1];
  }
}

// The pair's own step for the twist xi the joined system gave: de = (d offset, d gain).
TF_AL_HD inline void exposure_step(const double S[17], const ExposureElim& e, const double xi[6], double de[2]) {
  double t0 = S[kExpSr], t1 = S[kExpSlr];
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) { t0 = t0 + S[kExpP + i] * xi[i]; t1 = t1 + S[kExpQ + i] * xi[i]; }
  de[0] = 0.0; de[1] = 0.0;
  if (e.rank == 2) {
    const double u0 = t0 / e.l00, u1 = (t1 - e.l10 * u0) / e.l11;
    de[1] = u1 / e.l11;
    de[0] = (u0 - e.l10 * de[1]) / e.l00;
  } else if (e.rank == 1) {
    de[0] = (t0 / e.l00) / e.l00;
  }
}

// pair = (gain, offset).  The gain is clamped after every update; a component beyond the rank stays as it is.
TF_AL_HD inline void exposure_apply(double pair[2], int rank, const double de[2], double min_gain, double max_gain) {
  if (rank >= 1) pair[1] = pair[1] + de[0];
  if (rank == 2) {
    const double g = pair[0] + de[1];
    const double lo = g > min_gain ? g : min_gain;
    pair[0] = lo < max_gain ? lo : max_gain;
  }
}

}  // namespace tf
