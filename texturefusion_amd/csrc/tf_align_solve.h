// tf_align_solve.h -- the Gauss-Newton step of tf_align_frame: a damped 6 x 6 Cholesky solve and the pose update, one text
// for the device (k_align_solve, tf_align.hip) and for host programs (tests/cpp_align/align_solve_print.cpp).  Everything
// is f64 with -ffp-contract=off.  Every loop over matrix indices has a constant trip count and is unrolled, so that on the
// device the arrays live in registers (tf_cc_solve.h says why).
//
//   A is symmetric, given by its 21 upper entries row by row: (0,0) (0,1) .. (0,5) (1,1) .. (5,5).
//   M = A + damping * diag(A);  M = L L^T by rows (L[i][j] = (M[i][j] - sum_k<j L[i][k] L[j][k]) / L[j][j], the sum taken
//   in ascending k);  a pivot M[j][j] - sum_k L[j][k]^2 that is not above 1e-12 * max_i M[i][i] ends the solve as singular;
//   L y = b forwards, L^T x = y backwards, xi = -x.
//   Pose update of a twist xi = (v, w) about the camera centre: R <- exp([w]x) R, t <- t + v, with
//   exp([w]x) = I + a K + b K^2, K = [w]x, th = |w|:  a = sin(th) / th, b = 2 sin^2(th / 2) / th^2 (th >= 1e-8),
//   a = 1, b = 1/2 below (the series' first terms: the next ones are below 2e-17).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define TF_AL_HD __host__ __device__
#else
#define TF_AL_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define TF_AL_UNROLL _Pragma("unroll")
#else
#define TF_AL_UNROLL
#endif

namespace tf {

constexpr double kAlignPivot = 1e-12;  // relative to the largest diagonal entry
constexpr double kAlignSeries = 1e-8;  // |w| below which exp([w]x) takes the series form

// position of (i, j), i <= j, among the 21 upper entries
TF_AL_HD constexpr int align_upper(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// xi = -(A + damping diag(A))^-1 b.  Returns false (xi = 0) where a pivot fails the test above.
TF_AL_HD inline bool align_solve6(const double A[21], const double b[6], double damping, double xi[6]) {
  double M[36], L[36];
  double dmax = 0.0;
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i)
    TF_AL_UNROLL
    for (int j = 0; j < 6; ++j) {
      const double a = A[i <= j ? align_upper(i, j) : align_upper(j, i)];
      M[6 * i + j] = i == j ? a + damping * a : a;
      L[6 * i + j] = 0.0;
    }
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) { xi[i] = 0.0; dmax = M[7 * i] > dmax ? M[7 * i] : dmax; }
  const double thresh = kAlignPivot * dmax;
  bool ok = true;
  TF_AL_UNROLL
  for (int j = 0; j < 6; ++j) {
    double piv = M[7 * j];
    TF_AL_UNROLL
    for (int k = 0; k < j; ++k) piv = piv - L[6 * j + k] * L[6 * j + k];
    if (!(piv > thresh)) ok = false;
    const double d = sqrt(ok ? piv : 1.0);
    L[7 * j] = d;
    TF_AL_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      double s = M[6 * i + j];
      TF_AL_UNROLL
      for (int k = 0; k < j; ++k) s = s - L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s / d;
    }
  }
  if (!ok) return false;
  double y[6], x[6];
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    TF_AL_UNROLL
    for (int k = 0; k < i; ++k) s = s - L[6 * i + k] * y[k];
    y[i] = s / L[7 * i];
  }
  TF_AL_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    TF_AL_UNROLL
    for (int k = i + 1; k < 6; ++k) s = s - L[6 * k + i] * x[k];
    x[i] = s / L[7 * i];
  }
  TF_AL_UNROLL
  for (int i = 0; i < 6; ++i) xi[i] = -x[i];
  return true;
}

// E = exp([w]x), row-major
TF_AL_HD inline void align_rodrigues(const double w[3], double E[9]) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double th = sqrt(th2);
  double a = 1.0, b = 0.5;
  if (th >= kAlignSeries) {
    const double sh = sin(0.5 * th);
    a = sin(th) / th;
    b = 2.0 * (sh * sh) / th2;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i)
    TF_AL_UNROLL
    for (int j = 0; j < 3; ++j) {
      const double k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
      E[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * K[3 * i + j]) + b * k2;
    }
}

// pose: row-major 3 x 4 [R | t], camera to world.  R <- exp([w]x) R, t <- t + v with xi = (v, w).
TF_AL_HD inline void align_update(double pose[12], const double xi[6]) {
  double E[9], R[9];
  align_rodrigues(xi + 3, E);
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i)
    TF_AL_UNROLL
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (E[3 * i] * pose[j] + E[3 * i + 1] * pose[4 + j]) + E[3 * i + 2] * pose[8 + j];
  TF_AL_UNROLL
  for (int i = 0; i < 3; ++i) {
    TF_AL_UNROLL
    for (int j = 0; j < 3; ++j) pose[4 * i + j] = R[3 * i + j];
    pose[4 * i + 3] = pose[4 * i + 3] + xi[i];
  }
}

}  // namespace tf
