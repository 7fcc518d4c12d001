// exact_sum.hpp -- float64 sums that do not depend on the order of their terms, behind pmn_icp_accumulate (registration.hip) and
// pmn_plane_inliers (cloud_plane.hip).  A floating-point sum depends on the order of its terms, an integer sum does not: every term (a
// float64) is scaled by a power of two chosen on the host from a bound of the term (exact_scale), cut into EXACT_LIMBS signed 32-bit
// digits held in int64 words (exact_split); digits are added with integer adds -- a lane's own, the 64 lanes of a wave by a butterfly
// (exact_wave_sum), up to 2^31 terms without a carry -- a workgroup stores its digit sums into the caller's scratch, [word][nb], and a
// second launch (exact_finish, one one-wave workgroup per sum) adds the workgroups' digits, propagates the carries once and rounds the
// 160-bit total to float64, once.  No atomics of any kind.  What is lost: the part of a term below 2^-157 of the bound of its sum
// (truncated toward zero), and the one rounding of the total.  SUMS, the number of sums, is the template parameter; word i * EXACT_LIMBS
// + k is digit k of sum i.
#pragma once
#include "pmn_common.hpp"

#include <cmath>

#define EXACT_LIMBS 5
#define EXACT_FINISH_THREADS 64

template <int SUMS>
struct ExactScale {
    double to_digits[SUMS];  // 2^(157 - e_i), |term_i| < 2^e_i: a term times this is an integer below 2^157 in magnitude plus a fraction
};

// to_digits for a sum whose terms are bounded by `bound` (one more bit of margin for the roundings of the bound itself); false when the
// scaling would not stay a normal float64
inline bool exact_scale(double bound, double& to_digits) {
    int e = 0;
    (void)std::frexp(bound, &e);  // bound < 2^e
    e += 1;
    if (!std::isfinite(bound) || e > 800 || e < -800) return false;
    to_digits = std::ldexp(1.0, 32 * (EXACT_LIMBS - 1) + 29 - e);
    return true;
}

// digit K of y, which it removes from y (from the top digit down: K = EXACT_LIMBS - 1 first)
template <int K>
__device__ __forceinline__ long long exact_split(double& y) {
#pragma clang fp contract(off)
    const double w = __builtin_ldexp(1.0, 32 * K);
    const double d = trunc(y * __builtin_ldexp(1.0, -32 * K));  // |d| < 2^32 (the top digit: < 2^29)
    y -= d * w;                                                 // exact: removes the leading bits
    return (long long)d;
}

// the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ long long exact_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sums[i] for i = blockIdx.x, the body of a finishing kernel of SUMS one-wave workgroups: the wave adds the nb workgroups' digits --
// integers, so the order is free; it is fixed anyway -- then lane 0 propagates the carries and rounds.
template <int SUMS>
__device__ __forceinline__ void exact_finish(const long long* __restrict__ partial, int nb, const ExactScale<SUMS>& scale,
                                             double* __restrict__ sums) {
#pragma clang fp contract(off)
    const int i = blockIdx.x, lane = threadIdx.x;
    long long L[EXACT_LIMBS];
#pragma unroll
    for (int k = 0; k < EXACT_LIMBS; ++k) {
        const long long* __restrict__ p = partial + (size_t)(i * EXACT_LIMBS + k) * nb;
        long long v = 0;
        for (int j = lane; j < nb; j += EXACT_FINISH_THREADS) v += p[j];
        L[k] = exact_wave_sum(v);
    }
    if (lane != 0) return;
    // digits into [0, 2^32), the top one keeps the sign (|total| < 2^31 * 2^157: the top word stays below 2^60)
#pragma unroll
    for (int k = 0; k + 1 < EXACT_LIMBS; ++k) {
        const long long c = L[k] >> 32;  // floor
        L[k] -= c * 4294967296LL;
        L[k + 1] += c;
    }
    const bool neg = L[EXACT_LIMBS - 1] < 0;
    if (neg) {  // magnitude: complement every digit, add one
        long long carry = 1;
#pragma unroll
        for (int k = 0; k + 1 < EXACT_LIMBS; ++k) {
            const long long d = 4294967295LL - L[k] + carry;
            carry = d >> 32;
            L[k] = d & 4294967295LL;
        }
        L[EXACT_LIMBS - 1] = -1 - L[EXACT_LIMBS - 1] + carry;
    }
    // The magnitude as six 32-bit digits, rounded to float64 ONCE (to nearest, ties to even): the 64 bits from the leading digit down
    // plus the digit below them, the rest as a sticky bit.  Adding the digits as doubles would round more than once, and where those
    // roundings fall depends on the scale, that is on the caller's bound.
    unsigned long long D[EXACT_LIMBS + 1];
#pragma unroll
    for (int k = 0; k + 1 < EXACT_LIMBS; ++k) D[k] = (unsigned long long)L[k];
    D[EXACT_LIMBS - 1] = (unsigned long long)L[EXACT_LIMBS - 1] & 4294967295ULL;
    D[EXACT_LIMBS] = (unsigned long long)L[EXACT_LIMBS - 1] >> 32;
    int h = -1;
#pragma unroll
    for (int k = 0; k <= EXACT_LIMBS; ++k) h = D[k] ? k : h;
    double x = 0.0;
    if (h >= 0) {
        unsigned long long d0 = 0, d1 = 0, d2 = 0, below = 0;  // digits h, h - 1, h - 2 and the OR of the lower ones
#pragma unroll
        for (int k = 0; k <= EXACT_LIMBS; ++k) {
            d0 = k == h ? D[k] : d0;
            d1 = k == h - 1 ? D[k] : d1;
            d2 = k == h - 2 ? D[k] : d2;
            below |= k < h - 2 ? D[k] : 0ULL;
        }
        const unsigned long long hi = (d0 << 32) | d1;  // >= 2^32
        const int lz = __clzll((long long)hi);         // 0 .. 31
        const unsigned long long m = lz ? (hi << lz) | (d2 >> (32 - lz)) : hi;  // bit 63 set
        const bool sticky = ((d2 << lz) & 4294967295ULL) != 0 || below != 0;
        unsigned long long q = m >> 11;
        const unsigned long long r = m & 2047ULL;
        if (r > 1024ULL || (r == 1024ULL && (sticky || (q & 1ULL)))) q += 1;
        x = __builtin_ldexp((double)q, 11 - lz + 32 * (h - 1));  // exact: q <= 2^53
    }
    x = x / scale.to_digits[i];  // exact: a power of two
    sums[i] = neg ? -x : x;
}
