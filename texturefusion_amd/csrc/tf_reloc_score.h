// tf_reloc_score.h -- the score of a query descriptor against an indexed one (tf_reloc.hip): the final f64 expressions, one
// text for the device (k_reloc_score) and for host programs (tests/cpp_reloc/reloc_score_print.cpp), restated in
// tests/reloc_ref.py.  Everything that is summed is an integer, so the order of summation does not matter; what is left
// for f64 is a handful of operations in a fixed order (-ffp-contract=off).
//
//   n = tiny_w * tiny_h blocks of bw x bh pixels, a = 256 * bw * bh (a grey level of a block sum)
//   D_i = G_i(q) - G_i(k);  sum_d = sum D_i (i64),  sum_d2 = sum D_i^2 (u64)
//   N = n * sum_d2 - sum_d^2: an exact integer of up to 128 bits, >= 0 (Cauchy-Schwarz), n times the zero-mean SSD.  A
//   uniform brightness offset that saturates nowhere adds the same number to every D_i and leaves N as it is, exactly --
//   which sum_d2 - sum_d^2 / n evaluated in f64 would not: the division rounds, and sum_d^2 can pass 2^53 at 160 x 120.
//   Nf = (double)(N >> 64) * 2^64 + (double)(N & (2^64 - 1))        (two exact conversions or roundings, one addition)
//   s_grey = Nf / (((double)n * (double)n) * (a * a))               (grey levels squared)
//   m = blocks valid in both;  sum_z2 = sum over them of (Z_i(q) - Z_i(k))^2 (u64, millimetres squared)
//   s_depth = ((double)sum_z2 / (double)m) * 1e-6                   (metres squared; 0 where m == 0)
//   score = (double)grey_weight * s_grey + (double)depth_weight * s_depth;  +inf where m < min_overlap
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TF_RL_HD __host__ __device__
#else
#define TF_RL_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tf {

struct RelocU128 { uint64_t hi, lo; };

// a * b in full, through 32-bit halves
TF_RL_HD inline RelocU128 reloc_mul64(uint64_t a, uint64_t b) {
  const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);  // < 3 * 2^32
  RelocU128 r;
  r.lo = (p00 & 0xFFFFFFFFull) | (mid << 32);
  r.hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
  return r;
}

// N = n * sum_d2 - sum_d^2 (the caller's sums are those of n values: N >= 0)
TF_RL_HD inline RelocU128 reloc_grey_n(uint64_t sum_d2, int64_t sum_d, uint32_t n) {
  const uint64_t ad = sum_d < 0 ? (uint64_t)0 - (uint64_t)sum_d : (uint64_t)sum_d;
  const RelocU128 x = reloc_mul64((uint64_t)n, sum_d2), y = reloc_mul64(ad, ad);
  RelocU128 r;
  r.lo = x.lo - y.lo;
  r.hi = x.hi - y.hi - (x.lo < y.lo ? 1u : 0u);
  return r;
}

TF_RL_HD inline double reloc_grey_score(uint64_t sum_d2, int64_t sum_d, uint32_t n, uint32_t bw, uint32_t bh) {
  const RelocU128 N = reloc_grey_n(sum_d2, sum_d, n);
  const double nf = (double)N.hi * 18446744073709551616.0 + (double)N.lo;
  const double a = 256.0 * (double)bw * (double)bh;
  return nf / (((double)n * (double)n) * (a * a));
}

TF_RL_HD inline double reloc_depth_score(uint64_t sum_z2, uint32_t m) {
  return m ? ((double)sum_z2 / (double)m) * 1e-6 : 0.0;
}

TF_RL_HD inline double reloc_score(uint64_t sum_d2, int64_t sum_d, uint64_t sum_z2, uint32_t m, uint32_t n, uint32_t bw,
                                   uint32_t bh, float grey_weight, float depth_weight, int32_t min_overlap) {
  if ((int64_t)m < (int64_t)min_overlap) return (double)INFINITY;
  const double g = (double)grey_weight * reloc_grey_score(sum_d2, sum_d, n, bw, bh);
  const double d = (double)depth_weight * reloc_depth_score(sum_z2, m);
  return g + d;
}

}  // namespace tf
