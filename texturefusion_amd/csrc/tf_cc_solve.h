// tf_cc_solve.h -- the per-cluster solve of Chisel::CompensateColor (Structure/Chisel.cpp:247-266), one text for the host
// path (tf_compensate_color, tf_atlas.hip) and the device path (k_ccd_combine, tf_cc.hip).  Every statement is f64 (or an
// explicit f32 rounding) with -ffp-contract=off; f64 divide and square root are correctly rounded on both sides, so host
// and device compute the same bits.  Every loop over matrix indices has a constant trip count and is unrolled: on the
// device the 3x3 arrays then live in registers (a register file cannot be indexed at run time; an index that stays a
// variable sends the array to private memory).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define TF_CC_HD __host__ __device__
#else
#define TF_CC_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define TF_CC_UNROLL _Pragma("unroll")
#else
#define TF_CC_UNROLL
#endif

namespace tf {

// symmetric 3x3 eigen-decomposition, cyclic Jacobi in double: A = V diag(w) V^T
TF_CC_HD inline void sym3_eig(const float A[9], double w[3], double V[9]) {
  double a[9];
  TF_CC_UNROLL
  for (int i = 0; i < 9; i++) { a[i] = (double)A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 64; sweep++) {
    if (a[1] * a[1] + a[2] * a[2] + a[5] * a[5] < 1e-300) break;
    TF_CC_UNROLL
    for (int p = 0; p < 2; p++)
      TF_CC_UNROLL
      for (int q = p + 1; q < 3; q++) {
        const double apq = a[3 * p + q];
        if (apq == 0.0) continue;
        const double theta = (a[3 * q + q] - a[3 * p + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        TF_CC_UNROLL
        for (int k = 0; k < 3; k++) {
          const double akp = a[3 * k + p], akq = a[3 * k + q];
          a[3 * k + p] = cs * akp - sn * akq;
          a[3 * k + q] = sn * akp + cs * akq;
        }
        TF_CC_UNROLL
        for (int k = 0; k < 3; k++) {
          const double apk = a[3 * p + k], aqk = a[3 * q + k];
          a[3 * p + k] = cs * apk - sn * aqk;
          a[3 * q + k] = sn * apk + cs * aqk;
        }
        TF_CC_UNROLL
        for (int k = 0; k < 3; k++) {
          const double vkp = V[3 * k + p], vkq = V[3 * k + q];
          V[3 * k + p] = cs * vkp - sn * vkq;
          V[3 * k + q] = sn * vkp + cs * vkq;
        }
      }
  }
  TF_CC_UNROLL
  for (int i = 0; i < 3; i++) w[i] = a[4 * i];
}
TF_CC_HD inline void mat3_mul(const double A[9], const double B[9], double C[9]) {
  TF_CC_UNROLL
  for (int i = 0; i < 3; i++)
    TF_CC_UNROLL
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// Chisel.cpp:247-266: T = U Ds' Um Dm Um^T Ds' U^T with media = Ds U^T Ct U Ds
TF_CC_HD inline void color_transfer(const float cov_src[9], const float cov_tar[9], float T[9]) {
  double ws[3], U[9], Ut[9], ct[9], D[9] = {0}, M1[9], M2[9], media[9];
  sym3_eig(cov_src, ws, U);
  TF_CC_UNROLL
  for (int i = 0; i < 3; i++) {
    D[4 * i] = (double)(float)sqrt(ws[i] > 0.0 ? ws[i] : 0.0);
    TF_CC_UNROLL
    for (int j = 0; j < 3; j++) { Ut[3 * i + j] = U[3 * j + i]; ct[3 * i + j] = (double)cov_tar[3 * i + j]; }
  }
  mat3_mul(D, Ut, M1); mat3_mul(M1, ct, M2); mat3_mul(M2, U, M1); mat3_mul(M1, D, media);
  float mediaf[9];
  TF_CC_UNROLL
  for (int i = 0; i < 9; i++) mediaf[i] = (float)media[i];
  TF_CC_UNROLL
  for (int i = 0; i < 3; i++)
    TF_CC_UNROLL
    for (int j = i + 1; j < 3; j++) mediaf[3 * j + i] = mediaf[3 * i + j];
  double wm[3], Um[9], Umt[9], Dm[9] = {0}, Di[9] = {0};
  sym3_eig(mediaf, wm, Um);
  TF_CC_UNROLL
  for (int i = 0; i < 3; i++) {
    Dm[4 * i] = (double)(float)sqrt(wm[i] > 0.0 ? wm[i] : 0.0);
    Di[4 * i] = (double)(float)(1.0 / ((double)(float)D[4 * i] + 1e-2));  // 1 / (diag + 1e-2), double literal (:260-262)
    TF_CC_UNROLL
    for (int j = 0; j < 3; j++) Umt[3 * i + j] = Um[3 * j + i];
  }
  double A1[9], A2[9];
  mat3_mul(U, Di, A1); mat3_mul(A1, Um, A2); mat3_mul(A2, Dm, A1); mat3_mul(A1, Umt, A2);
  mat3_mul(A2, Di, A1); mat3_mul(A1, Ut, A2);
  TF_CC_UNROLL
  for (int i = 0; i < 9; i++) T[i] = (float)A2[i];
}

}  // namespace tf
