// Order-independent accumulation of floats for the scatter-add gradients (det_grads.hip).
// A contribution v is rounded to nearest-even to a multiple of the quantum q = 2^-e and added as a two's-complement
// integer with a plain vector atomic on 64 bits: integer addition is associative, so the sum does not depend on the
// order of arrival, and what is added depends on v alone.  The scale is chosen per call, on the device, from a bound B
// on |v| that a pre-pass leaves in the header (below) and from the number of contributions of the call, N_c <= 2^n
// (n <= 32, checked at the C ABI):
//     B = c max|g| [max|f|]  (exact in double: at most 24 x 24 bits times a power of two),   2^(b-1) <= B < 2^b,
//     e = 63 - b - n,   q = 2^(b + n - 63).
// No overflow, even if all N_c contributions land on one element: |v| <= B <= 2^b (1 - 2^-24) for one fp32 factor
// (|v| <= B / 3 for the sweep's two), so |round(v / q)| <= 2^(63-n) - 2^(39-n) + 1/2 and the sum of 2^n of them
// stays below 2^63.  Resolution: B >= 2^(b-1), so q <= 2^(n-32) 2^-30 B <= 2^-30 B for every n <= 32.
// v / q is formed in double: v has 24 bits and q is a power of two, so the product is exact and __double2ll_rn is the
// only rounding (a product below double's normal range is far below q / 2 and rounds to 0 either way).
// -231 <= e <= 354 over everything fp32 inputs can give, inside double's exponent range, so 2^e and 2^-e are built from
// their bit patterns.  tests/det_cases.py states the same rule in Python.
// A non-finite contribution (from finite inputs only where a product overflows) sets the header's poison word instead:
// a vector store of the same value from every lane that meets one.
#pragma once
#include "zest_common.cuh"

struct FixedHeader {                         // the first 64 bytes of the workspace; zeroed with it before the pre-pass
    unsigned max_bits[2];                    // bit patterns of max|g| and max|f| (integer atomic max: order-independent)
    unsigned poison;
    unsigned pad_[13];
};
constexpr size_t kFixedHeaderBytes = sizeof(FixedHeader);

struct FixedScale {
    double scale, inv;                       // 2^e and 2^-e
    bool zero, bad;                          // B = 0: nothing to add;  a NaN or an infinity among the inputs
};

// n_maxima: 1 (B = c max|g|) or 2 (B = c max|g| max|f|);  c: the kernel's own constant factor, a power of two
__device__ __forceinline__ FixedScale fixed_scale(const FixedHeader *h, int n_maxima, double c, int n_log2) {
    const unsigned a = h->max_bits[0], b = n_maxima > 1 ? h->max_bits[1] : 0x3f800000u;
    FixedScale s;
    s.bad = a >= 0x7f800000u || b >= 0x7f800000u;
    const double B = (double)__uint_as_float(a) * (double)__uint_as_float(b) * c;
    s.zero = !s.bad && B == 0.0;
    const int e = (s.bad || s.zero) ? 0 : 63 - ((int)((__double_as_longlong(B) >> 52) & 0x7ff) - 1022) - n_log2;
    s.scale = __longlong_as_double((long long)(1023 + e) << 52);
    s.inv = __longlong_as_double((long long)(1023 - e) << 52);
    return s;
}

struct FixedAdd {
    const float *base;                       // the fp32 result the kernel body indexes; never read or written through here
    unsigned long long *acc;                 // one 64-bit accumulator per element of it
    unsigned *poison;
    double scale;
    __device__ __forceinline__ void add(const float *p, float v) const {
        if (!(fabsf(v) <= 3.402823466e+38f)) {
            *poison = 1u;
            return;
        }
        atomicAdd(acc + (p - base), (unsigned long long)__double2ll_rn((double)v * scale));
    }
};
