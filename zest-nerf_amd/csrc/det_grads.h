// Host doors of det_grads.hip that other translation units use: the ordered bias sums of the fp32 training path.
#pragma once
#include <hip/hip_runtime.h>

namespace zest {

constexpr int kBwdRows = 64;            // rows of M per block of the activation backward (body_act_bwd_colsum.cuh)

// db[n] = sum_m A[m, n] (n < N <= 256): per-block partials into `part` (ceil(M / 256) rows of N floats), then one
// launch that adds them in block order and writes db in full.  The same bits on every call.
void colsum_ordered(const float *A, int M, int N, int lda, float *part, float *db, hipStream_t st);

// act_bwd_colsum_kernel's work with the bias gradient through partials (ceil(M / 64) rows of N floats) in the same way
void act_bwd_colsum_ordered(float *d, const float *pre, const float *m, float *dm, int M, int N, int v2, float *part,
                            float *db, hipStream_t st);

}  // namespace zest
