// tf_align_group_solve.h -- what tf_align_group's step needs beyond tf_align_solve.h: the pose update of a frame that moves
// with a rigid body whose twist is taken about another frame's camera centre.  One text for the device (k_galign_solve,
// tf_align_group.hip) and for host programs (tests/cpp_align_group/group_solve_print.cpp).  Everything is f64 with
// -ffp-contract=off; the loops have constant trip counts and are unrolled, as tf_align_solve.h's.
//
//   A twist xi = (v, w) about the centre c moves a world point x to c + E (x - c) + v, E = exp([w]x) (align_rodrigues).
//   A frame [R | t] of the body becomes R <- E R, t <- (c + E (t - c)) + v: d = t - c componentwise,
//   (E d)_i = (E[i][0] d_0 + E[i][1] d_1) + E[i][2] d_2, then c_i + (E d)_i, then + v_i.
//   For the body's anchor c is its own t: d = 0, E d = 0, c + 0 = c, and t <- t + v -- the bits of align_update (the
//   product E R is the same text as there).
#pragma once

#include "tf_align_solve.h"

namespace tf {

// pose: row-major 3 x 4 [R | t], camera to world; E = exp([w]x) of the step, c the centre of the twist (the anchor's t before
// the step), v the step's translation
TF_AL_HD inline void align_update_about(double pose[12], const double E[9], const double c[3], const double v[3]) {
  double R[9], d[3];
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i)
    TF_AL_UNROLL
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (E[3 * i] * pose[j] + E[3 * i + 1] * pose[4 + j]) + E[3 * i + 2] * pose[8 + j];
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i) d[i] = pose[4 * i + 3] - c[i];
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i) {
    TF_AL_UNROLL
    for (int j = 0; j < 3; ++j) pose[4 * i + j] = R[3 * i + j];
    const double ed = (E[3 * i] * d[0] + E[3 * i + 1] * d[1]) + E[3 * i + 2] * d[2];
    pose[4 * i + 3] = (c[i] + ed) + v[i];
  }
}

}  // namespace tf
