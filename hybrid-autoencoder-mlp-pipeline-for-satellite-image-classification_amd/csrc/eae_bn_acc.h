// The arithmetic of the folded BatchNorm finalize (eae_common.hip.h has the scheme): per-channel workgroup sums go to 64-bit fixed
// point, are added with integer atomics, and the consumers turn the integer totals back into coefficients.  Everything here is a
// host-and-device inline function of its arguments: the kernels include it for the arithmetic and keep the atomics, loads and
// barriers; tests/bn_acc_check.cpp includes it alone and is compared bit for bit with tests/bn_acc_ref.py on the CPU.  (A host
// build must not contract a * b + c into one rounding if it is to agree with the restatement: -ffp-contract=off.)
//
// Range.  A contribution v is stored as llrint(v * scale); the accumulator is read as a SIGNED 64-bit integer, so the total of all
// contributions of a channel has to stay inside (-2^63, 2^63).  With N = contributions per replica x SyncBN world contributions,
// every one of which passed |v * scale| < 2^62 / N, it does: |total| < 2^62 (1 + 2^-22) whatever the signs are.  A contribution at
// or above the limit (or NaN) is not added; it sets the channel's sticky flag, and the consumers turn a set flag into NaN.
//   forward  (scale 2^24): workgroup sums of y and y^2 below 2^38 / N; quantum 2^-24, i.e. half of it per contribution
//   backward (scale 2^42): workgroup sums of g and g * xhat below 2^20 / N; quantum 2^-42
// (Up to this header the limit was the constant 9.0e18 ~ 2^62.96 per contribution whatever N was: two contributions of 2^62.5
// passed it and wrapped the total without a trace, tests/test_bn_acc_reference.py shows it on the restatement.)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define EAE_BN_HD __host__ __device__ __forceinline__
#else
#define EAE_BN_HD inline
#endif

constexpr float BN_ACC_SCALE_FWD = 16777216.f;        // 2^24
constexpr float BN_ACC_SCALE_BWD = 4398046511104.f;   // 2^42
constexpr double BN_ACC_TOTAL = 4611686018427387904.0;   // 2^62: what the magnitudes of all contributions of a channel may add up to

// the limit on |v * scale| of ONE contribution, for a launch of `contributions` workgroups per channel on each of `world` replicas
EAE_BN_HD float bn_acc_limit(long long contributions, int world) {
  const double n = (double)(contributions > 0 ? contributions : 1) * (double)(world > 0 ? world : 1);
  return (float)(BN_ACC_TOTAL / n);
}
// the same limit on the value itself
EAE_BN_HD float bn_acc_value_limit(float scale, long long contributions, int world) { return bn_acc_limit(contributions, world) / scale; }

// float -> fixed point.  `sv` = v * scale (one fp32 rounding, by the caller).  False: the contribution does not fit (too large, or
// not finite) and has to raise the flag instead.
EAE_BN_HD bool bn_acc_fits(float sv, float limit) { return fabsf(sv) < limit; }
EAE_BN_HD unsigned long long bn_acc_fixed(float sv) { return (unsigned long long)llrintf(sv); }      // round to nearest even; added mod 2^64

// ---- forward: integer sums of y and y^2 -> mean, variance, the coefficients s, t of y -> s * y + t, running statistics
struct BnAccFwd { float s, t, mean, invstd; double var; };
EAE_BN_HD BnAccFwd bn_acc_fwd_finish(long long s1, long long s2, bool poisoned, float inv_scale, float count, float eps, float gamma, float beta) {
  BnAccFwd o;
  const double a = poisoned ? (double)__builtin_nanf("") : (double)s1 * (double)inv_scale, b = (double)s2 * (double)inv_scale;
  const double mean = a / count;
  double var = b / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = 1.0f / sqrtf((float)var + eps);
  const float s = gamma * invstd, t = beta - (float)mean * s;
  o.s = s; o.t = t; o.mean = (float)mean; o.invstd = invstd; o.var = var;
  return o;
}
EAE_BN_HD void bn_acc_running(const BnAccFwd& o, float count, float momentum, float& rm, float& rv) {
  const double unb = count > 1.f ? o.var * (double)count / ((double)count - 1.0) : o.var;
  rm = (1.f - momentum) * rm + momentum * o.mean;
  rv = (1.f - momentum) * rv + momentum * (float)unb;
}

// ---- backward: integer sums of g and g * xhat -> dbeta, dgamma and the coefficients of dy = A * g + B * y + C
// (a flagged channel has NEITHER sum: both gradients are NaN.  dgamma used to be taken from the partial integer total, a finite
// number that meant nothing and reached whoever read .grad of a stand-alone module.)
struct BnAccBwd { float A, Bc, Cc, dgamma, dbeta; };
EAE_BN_HD BnAccBwd bn_acc_bwd_finish(long long s1, long long s2, bool poisoned, float inv_scale, float count, float gamma, float mean, float invstd) {
  BnAccBwd o;
  const float db = poisoned ? __builtin_nanf("") : (float)((double)s1 * (double)inv_scale);
  const float dg = poisoned ? __builtin_nanf("") : (float)((double)s2 * (double)inv_scale);
  const float A = gamma * invstd;
  const float Bc = -A * invstd * dg / count;
  const float Cc = -A * db / count - Bc * mean;
  o.A = A; o.Bc = Bc; o.Cc = Cc; o.dgamma = dg; o.dbeta = db;
  return o;
}
