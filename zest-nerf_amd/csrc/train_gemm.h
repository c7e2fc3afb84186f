// The training GEMMs on three-term bf16 operands (train_gemm.hip), as mlp_train.hip calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace zest {

// rows of M per partial product of the TN operation: 128 chunks at the headline 131 072 rows, which with the four tiles
// of a 256 x 256 gradient is two workgroups on every CU, and one on every CU for the one- and two-tile gradients
constexpr int kTrainGemmChunk = 1024;
constexpr int kTrainGemmMaxDim = 256;       // N and K run from 1 to this
// NT, NN: the weight operand split once per GEMM, three bf16 planes of at most 256 x 256 (+ 16-byte alignment slack)
constexpr size_t kTrainGemmPackFloats = 3 * 256 * 256 / 2 + 4;

// floats of workspace train_gemm_split needs: the TN partials; the packed weight planes for NT and NN
size_t train_gemm_split_workspace(int op, int M, int N, int K);
// op: ZEST_GEMM_OP_*; operands as zest_train_gemm documents them.  Arguments are NOT checked here.
void train_gemm_split(int op, int M, int N, int K, const float *a, int lda, const float *b, int ldb, float *c,
                      int ldc, int beta, float *workspace, hipStream_t st);

}  // namespace zest
