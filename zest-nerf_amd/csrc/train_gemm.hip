// The three GEMMs of the fp32 training path (mlp_train.hip) on bf16 MFMAs, fp32 in and fp32 out:
//   NT  Y[M,N]   = X[M,K] . Wt[N,K]^T (+ Y)          forward
//   NN  dX[M,K]  = dY[M,N] . Wt[N,K]  (+ dX)         data gradient
//   TN  dWt[N,K] = dY[M,N]^T . X[M,K]                weight gradient, contracted over M = rays x samples
// Every fp32 operand value a is split into three bf16 terms with fp32's exponent range,
//   hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid)     (round to nearest even; both residuals are exact
//                                                                   in fp32),
// and a product a.b is the six MFMAs mm, hl, lh, hm, mh, hh (smallest first) into ONE fp32 accumulator; the dropped
// ml, lm, ll terms are <= 2^-24 relative each.  That is sgemm's own error class, at six bf16 MFMAs
// (v_mfma_f32_32x32x16_bf16) per product instead of one fp32 MFMA at 1/16 of the bf16 rate.
// A non-finite input gives non-finite output (inf - inf in the split), not necessarily the library's kind of it.
//
// One kernel body serves the three operations as C[I,J] = sum_k A(i,k) B(j,k).  A workgroup (4 waves) owns a 128 x 128
// tile of C, a wave 64 x 64 of it (2 x 2 accumulators of 32 x 32).  Per step of 32 along k the operands' bf16 terms
// go into LDS plane-major, [operand][plane][row][k] with k padded from 32 to 40 elements, as 16-byte runs of 8
// k-values: such a run IS an MFMA operand fragment (lane l: row l & 31, k = 8 (l >> 5) .. + 7), read back with
// ds_read_b128.  The global loads of a step are issued before the MFMAs of the step before and consumed after them.
//   NT, NN (one instantiation): A = X | dY has k contiguous; each thread loads two runs (float4 pairs where base and
//     leading dimension are multiples of 4 floats, dwords otherwise) and splits them on the way into LDS.  B, the
//     weights, is split ONCE per GEMM by train_gemm_pack_kernel into zero-padded planes in the workspace (the pack
//     kernel absorbs the difference between Wt read as (n, k) and as (k, n)); workgroups copy their tile of it.
//   TN: both operands have the row contiguous; see load_rows4.  M is split into chunks of kTrainGemmChunk rows
//     (blockIdx.z), each writing its partial product into the workspace; a second launch sums the partials in chunk
//     order (in fp64, rounded once).  The MFMA accumulator is added to a running total and cleared every 8 steps
//     (256 k-values), which keeps the rounding chains of a chunk as short as a forward GEMM's.
// Ragged rows and k are zero in LDS; every load is issued from an address inside [rows) x [k range) of its operand.
// No atomics anywhere: results are bit-reproducible.
#include "train_gemm.h"
#include "zest_common.cuh"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int kTile = 128;          // rows of either operand per workgroup
constexpr int kStep = 32;           // k per step
constexpr int kFlush = 8;           // steps between two flushes of the MFMA accumulator into the running total
constexpr int kLdk = 40;            // LDS row pitch in bf16 elements (80 bytes)
constexpr int kPlane = kTile * kLdk;            // elements of one plane of one operand

struct GemmArgs {
    const float *a, *b;
    long long a_sr, a_sk, b_sr, b_sk;       // element (row, k) of an operand: base[row * sr + k * sk]
    float *c;
    int ldc;
    int I, J, Kc;                           // C is I x J, the contraction runs over Kc
    int chunk;                              // k range of one blockIdx.z
    int n_jt;                               // column tiles: blockIdx.x = i-tile * n_jt + j-tile
    int beta, a_vec, b_vec;
    const unsigned short *bp;               // NT, NN: B already split (train_gemm_pack_kernel), [3][jpad][kpad] bf16
    int jpad, kpad;
};

// two fp32 -> their three bf16 terms, packed (first value in the low half)
__device__ __forceinline__ void split2(float x0, float x1, unsigned &hi, unsigned &mid, unsigned &lo) {
    const f32x2 f = {x0, x1};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
    const f32x2 r1 = {x0 - __uint_as_float(hi << 16), x1 - __uint_as_float(hi & 0xffff0000u)};
    mid = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
    const f32x2 r2 = {r1[0] - __uint_as_float(mid << 16), r1[1] - __uint_as_float(mid & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}

// The thread's two runs of 8 k-values of one operand tile: rows row0 .. of [0, rows), k from k0 in [.., kend).
// KC: k is the contiguous index (4 threads per row); otherwise the row is (128 consecutive threads per k-run).
// Every load is issued unconditionally from an address inside the operand (row and k clamped to their last valid
// value); store_runs zeroes what lies outside.  A load under a per-element condition would be a branch and a full
// wait each, and a value consumed here would be waited for here instead of after the MFMAs.
template <bool KC>
__device__ __forceinline__ void load_runs(const float *__restrict__ p, long long sr, long long sk, int row0, int rows,
                                          int k0, int kend, bool vec, float (&v)[2][8]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int u = (int)threadIdx.x + 256 * q;
        const int r = KC ? u >> 2 : u & (kTile - 1), kg = KC ? u & 3 : u >> 7;
        const int k = k0 + 8 * kg;
        const long long row_c = min(row0 + r, rows - 1);
        if (KC && vec && k + 8 <= kend) {
            const float *src = p + row_c * sr + k;
            const float4 x0 = *reinterpret_cast<const float4 *>(src);
            const float4 x1 = *reinterpret_cast<const float4 *>(src + 4);
            v[q][0] = x0.x, v[q][1] = x0.y, v[q][2] = x0.z, v[q][3] = x0.w;
            v[q][4] = x1.x, v[q][5] = x1.y, v[q][6] = x1.z, v[q][7] = x1.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++) v[q][e] = p[row_c * sr + (long long)min(k + e, kend - 1) * sk];
        }
    }
}

// zero what lies outside [rows) x [.., kend), split the two runs and write them into the operand's three planes
template <bool KC>
__device__ __forceinline__ void store_runs(unsigned short *lds, int row0, int rows, int k0, int kend,
                                           const float (&v)[2][8]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int u = (int)threadIdx.x + 256 * q;
        const int r = KC ? u >> 2 : u & (kTile - 1), kg = KC ? u & 3 : u >> 7;
        const int k = k0 + 8 * kg;
        const bool row_ok = row0 + r < rows;
        u32x4 h, m, l;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned a, b, c;
            split2((row_ok && k + 2 * j < kend) ? v[q][2 * j] : 0.f,
                   (row_ok && k + 2 * j + 1 < kend) ? v[q][2 * j + 1] : 0.f, a, b, c);
            h[j] = a, m[j] = b, l[j] = c;
        }
        unsigned short *dst = lds + r * kLdk + 8 * kg;
        *reinterpret_cast<u32x4 *>(dst) = h;
        *reinterpret_cast<u32x4 *>(dst + kPlane) = m;
        *reinterpret_cast<u32x4 *>(dst + 2 * kPlane) = l;
    }
}

// the thread's two runs of the packed B operand, three planes each: zero-padded to whole tiles, so no masks
__device__ __forceinline__ void load_packed(const GemmArgs &g, int j0, int k0, u32x4 (&v)[2][3]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int u = (int)threadIdx.x + 256 * q;
        const unsigned short *src = g.bp + (size_t)(j0 + (u >> 2)) * g.kpad + k0 + 8 * (u & 3);
#pragma unroll
        for (int p = 0; p < 3; p++) v[q][p] = *reinterpret_cast<const u32x4 *>(src + (size_t)p * g.jpad * g.kpad);
    }
}
__device__ __forceinline__ void store_packed(unsigned short *lds, const u32x4 (&v)[2][3]) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int u = (int)threadIdx.x + 256 * q;
#pragma unroll
        for (int p = 0; p < 3; p++)
            *reinterpret_cast<u32x4 *>(lds + p * kPlane + (u >> 2) * kLdk + 8 * (u & 3)) = v[q][p];
    }
}

// TN: both operands have the ROW contiguous (the contraction index m strides by the leading dimension).  Threads
// 0..127 stage A, 128..255 stage B; a thread takes four consecutive rows (one float4 per k where base and leading
// dimension allow, four dwords otherwise) at its eight k-values: four runs.  Row 4 q + s of the tile goes to LDS row
// q + 32 s, so that the 32 lanes of a write and of a fragment read hit consecutive LDS rows; the epilogue undoes the
// permutation (tile row of LDS row p: 4 (p & 31) + (p >> 5)).
__device__ __forceinline__ void load_rows4(const float *__restrict__ p, long long sk, int row0, int rows, int k0,
                                           int kend, bool vec, float (&v)[8][4]) {
    const int t = threadIdx.x & 127, row = row0 + 4 * (t & 31), k = k0 + 8 * (t >> 5);
    if (vec && row + 4 <= rows) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const float4 x = *reinterpret_cast<const float4 *>(p + (long long)min(k + e, kend - 1) * sk + row);
            v[e][0] = x.x, v[e][1] = x.y, v[e][2] = x.z, v[e][3] = x.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++)
#pragma unroll
            for (int s = 0; s < 4; s++) v[e][s] = p[(long long)min(k + e, kend - 1) * sk + min(row + s, rows - 1)];
    }
}
__device__ __forceinline__ void store_rows4(unsigned short *lds, int row0, int rows, int k0, int kend,
                                            const float (&v)[8][4]) {
    const int t = threadIdx.x & 127, q = t & 31, kg = t >> 5, k = k0 + 8 * kg;
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const bool row_ok = row0 + 4 * q + s < rows;
        u32x4 h, m, l;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            unsigned a, b, c;
            split2((row_ok && k + 2 * j < kend) ? v[2 * j][s] : 0.f,
                   (row_ok && k + 2 * j + 1 < kend) ? v[2 * j + 1][s] : 0.f, a, b, c);
            h[j] = a, m[j] = b, l[j] = c;
        }
        unsigned short *dst = lds + (q + 32 * s) * kLdk + 8 * kg;
        *reinterpret_cast<u32x4 *>(dst) = h;
        *reinterpret_cast<u32x4 *>(dst + kPlane) = m;
        *reinterpret_cast<u32x4 *>(dst + 2 * kPlane) = l;
    }
}

// B operand of NT / NN (the weights, <= 256 x 256): split once per GEMM into three zero-padded bf16 planes
// [3][jpad][kpad], so that the GEMM's workgroups - up to a thousand per weight tile - copy it instead of splitting it
// again.  row_fast: consecutive threads take consecutive rows (the contiguous index of NN's weight operand).
__global__ void train_gemm_pack_kernel(const float *__restrict__ b, long long sr, long long sk, int J, int Kc, int jpad,
                                       int kpad, int row_fast, unsigned short *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nkg = kpad / 8;
    if (t >= jpad * nkg) return;
    const int j = row_fast ? t % jpad : t / nkg, k = 8 * (row_fast ? t / jpad : t % nkg);
    u32x4 h, m, l;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const float x0 = (j < J && k + 2 * e < Kc) ? b[j * sr + (k + 2 * e) * sk] : 0.f;
        const float x1 = (j < J && k + 2 * e + 1 < Kc) ? b[j * sr + (k + 2 * e + 1) * sk] : 0.f;
        unsigned a, c, d;
        split2(x0, x1, a, c, d);
        h[e] = a, m[e] = c, l[e] = d;
    }
    unsigned short *dst = out + (size_t)j * kpad + k;
    *reinterpret_cast<u32x4 *>(dst) = h;
    *reinterpret_cast<u32x4 *>(dst + (size_t)jpad * kpad) = m;
    *reinterpret_cast<u32x4 *>(dst + 2 * (size_t)jpad * kpad) = l;
}

// A_KC: k is the contiguous index of A.  B_PACKED: B comes split from train_gemm_pack_kernel (NT and NN: then the
// contraction is at most 256 long, one accumulator does); otherwise B streams like A with the row contiguous and the
// accumulator is flushed every kFlush steps (TN).
template <bool A_KC, bool B_PACKED>
__global__ __launch_bounds__(256, 2) void train_gemm_kernel(const GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * 3 * kPlane];        // 61 440 bytes
    unsigned short *lds_a = lds, *lds_b = lds + 3 * kPlane;
    const int it = blockIdx.x / g.n_jt, jt = blockIdx.x % g.n_jt;
    const int i0 = it * kTile, j0 = jt * kTile;
    const int kbeg = blockIdx.z * g.chunk, kend = min(g.Kc, kbeg + g.chunk);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wi = (wid >> 1) * 64, wj = (wid & 1) * 64;        // the wave's corner inside the tile
    const int fr = lane & 31, fh = lane >> 5;
    // 32 x 32 tiles of the wave that reach into C (wave-uniform)
    bool on_i[2], on_j[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if constexpr (B_PACKED) on_i[t] = i0 + wi + 32 * t < g.I, on_j[t] = j0 + wj + 32 * t < g.J;
        else on_i[t] = i0 + wi / 32 + t < g.I, on_j[t] = j0 + wj / 32 + t < g.J;      // LDS rows p of 4 q + p / 32
    }

    // acc takes the MFMAs; in TN it is added to tot and cleared every kFlush steps, so that no rounding chain is
    // longer than 12 * kFlush = 96 accumulations (2 substeps x 6 products per step) however long the contraction
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[ti][tj][e] = tot[ti][tj][e] = 0.f;
    int step = 0;
    float *cz = g.c + (size_t)blockIdx.z * g.I * g.J;       // blockIdx.z > 0 only for the TN partials (ldc = J)
    f32x16 cin[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int e = 0; e < 16; e++) cin[ti][tj][e] = 0.f;
    if (B_PACKED && g.beta) {
        // beta = 1: C is read here, so that the loads fly under the staging of the first steps, and added at the
        // end (an accumulator that started from C would round every one of its 96 additions at C's magnitude) -
        // unconditionally, from clamped addresses: a lane outside C never stores its sum
#pragma unroll
        for (int ti = 0; ti < 2; ti++)
#pragma unroll
            for (int tj = 0; tj < 2; tj++) {
                if (!(on_i[ti] && on_j[tj])) continue;
                const int col = min(j0 + wj + 32 * tj + fr, g.J - 1);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int row = min(i0 + wi + 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * fh, g.I - 1);
                    cin[ti][tj][e] = cz[(size_t)row * g.ldc + col];
                }
            }
    }

    float va[2][8], vr[8][4];
    u32x4 pb[2][3];
    // TN: the operand this half of the workgroup stages (wave-uniform)
    const bool second = threadIdx.x >= 128;
    const float *rp = second ? g.b : g.a;
    const long long rsk = second ? g.b_sk : g.a_sk;
    const int r0 = second ? j0 : i0, rrows = second ? g.J : g.I;
    const bool rvec = second ? g.b_vec : g.a_vec;
    unsigned short *rlds = second ? lds_b : lds_a;
    if constexpr (B_PACKED) {
        load_runs<A_KC>(g.a, g.a_sr, g.a_sk, i0, g.I, kbeg, kend, g.a_vec, va);
        load_packed(g, j0, kbeg, pb);
    } else {
        load_rows4(rp, rsk, r0, rrows, kbeg, kend, rvec, vr);
    }
    for (int k0 = kbeg; k0 < kend; k0 += kStep) {
        __syncthreads();                // the MFMAs of the step before have read their fragments
        if constexpr (B_PACKED) {
            store_runs<A_KC>(lds_a, i0, g.I, k0, kend, va);
            store_packed(lds_b, pb);
        } else {
            store_rows4(rlds, r0, rrows, k0, kend, vr);
        }
        __syncthreads();
        if (k0 + kStep < kend) {        // next step's loads fly under this step's MFMAs
            if constexpr (B_PACKED) {
                load_runs<A_KC>(g.a, g.a_sr, g.a_sk, i0, g.I, k0 + kStep, kend, g.a_vec, va);
                load_packed(g, j0, k0 + kStep, pb);
            } else {
                load_rows4(rp, rsk, r0, rrows, k0 + kStep, kend, rvec, vr);
            }
        }
#pragma unroll
        for (int s = 0; s < kStep / 16; s++) {
            bf16x8 fa[2][3], fb[2][3];
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const int off = p * kPlane + (32 * t + fr) * kLdk + 16 * s + 8 * fh;
                    fa[t][p] = *reinterpret_cast<const bf16x8 *>(lds_a + wi * kLdk + off);
                    fb[t][p] = *reinterpret_cast<const bf16x8 *>(lds_b + wj * kLdk + off);
                }
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) {
                    if (!(on_i[ti] && on_j[tj])) continue;
                    f32x16 c = acc[ti][tj];
                    // planes 0 1 2 = hi mid lo; small products first
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][1], fb[tj][1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][0], fb[tj][2], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][2], fb[tj][0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][0], fb[tj][1], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][1], fb[tj][0], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ti][0], fb[tj][0], c, 0, 0, 0);
                    acc[ti][tj] = c;
                }
        }
        if (!B_PACKED && (++step % kFlush == 0 || k0 + kStep >= kend)) {
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) {
                    tot[ti][tj] += acc[ti][tj];
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[ti][tj][e] = 0.f;
                }
        }
    }
    // C tile: column on the lane, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5) in register e
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            if (!(on_i[ti] && on_j[tj])) continue;
            const int col = B_PACKED ? j0 + wj + 32 * tj + fr : j0 + 4 * fr + wj / 32 + tj;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int rin = (e & 3) + 8 * (e >> 2) + 4 * fh;
                const int row = B_PACKED ? i0 + wi + 32 * ti + rin : i0 + 4 * rin + wi / 32 + ti;
                if (row < g.I && col < g.J) {
                    float *dst = cz + (size_t)row * g.ldc + col;
                    *dst = B_PACKED ? acc[ti][tj][e] + cin[ti][tj][e] : tot[ti][tj][e];
                }
            }
        }
}

// dWt[n, k] (ldw) = sum over the chunks, in chunk order, of part[chunk][n][k]
__global__ void train_gemm_reduce_kernel(const float *__restrict__ part, int n_chunks, int N, int K,
                                         float *__restrict__ dW, int ldw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * K) return;
    double acc = 0.0;       // one rounding for the whole sum; the order is fixed all the same
    for (int z = 0; z < n_chunks; z++) acc += (double)part[(size_t)z * N * K + i];
    dW[(size_t)(i / K) * ldw + (i % K)] = (float)acc;
}

inline bool vec_ok(const float *p, int ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace

namespace zest {

size_t train_gemm_split_workspace(int op, int M, int N, int K) {
    if (M <= 0) return 0;
    if (op != ZEST_GEMM_OP_TN) return kTrainGemmPackFloats;
    return (size_t)zest_div_up(M, kTrainGemmChunk) * N * K;
}

void train_gemm_split(int op, int M, int N, int K, const float *a, int lda, const float *b, int ldb, float *c, int ldc,
                      int beta, float *workspace, hipStream_t st) {
    GemmArgs g;
    g.beta = beta, g.c = c, g.ldc = ldc, g.a = a, g.b = b, g.bp = nullptr, g.jpad = g.kpad = 0, g.b_vec = 0;
    unsigned nz = 1;
    if (op == ZEST_GEMM_OP_TN) {        // A = dY read as (n, m), B = X read as (k, m); partials [chunk][N][K]
        g.a_sr = 1, g.a_sk = lda, g.b_sr = 1, g.b_sk = ldb;
        g.I = N, g.J = K, g.Kc = M, g.chunk = kTrainGemmChunk;
        g.a_vec = vec_ok(a, lda), g.b_vec = vec_ok(b, ldb), g.beta = 0, g.c = workspace, g.ldc = K;
        nz = (unsigned)zest_div_up(M, kTrainGemmChunk);
    } else {                            // A = X (m, k) | dY (m, n);  B = Wt as (n, k) | as (k, n), packed first
        const bool nt = op == ZEST_GEMM_OP_NT;
        g.a_sr = lda, g.a_sk = 1, g.b_sr = nt ? ldb : 1, g.b_sk = nt ? 1 : ldb;
        g.I = M, g.J = nt ? N : K, g.Kc = nt ? K : N, g.chunk = g.Kc;
        g.a_vec = vec_ok(a, lda);
        g.jpad = zest_div_up(g.J, kTile) * kTile, g.kpad = zest_div_up(g.Kc, kStep) * kStep;
        unsigned short *planes = reinterpret_cast<unsigned short *>(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
        g.bp = planes;
        hipLaunchKernelGGL(train_gemm_pack_kernel, dim3(zest_div_up(g.jpad * g.kpad / 8, 256)), dim3(256), 0, st, b,
                           g.b_sr, g.b_sk, g.J, g.Kc, g.jpad, g.kpad, nt ? 0 : 1, planes);
    }
    g.n_jt = zest_div_up(g.J, kTile);
    const dim3 grid((unsigned)zest_div_up(g.I, kTile) * g.n_jt, 1, nz);
    if (op != ZEST_GEMM_OP_TN)
        hipLaunchKernelGGL((train_gemm_kernel<true, true>), grid, dim3(256), 0, st, g);
    else {
        hipLaunchKernelGGL((train_gemm_kernel<false, false>), grid, dim3(256), 0, st, g);
        hipLaunchKernelGGL(train_gemm_reduce_kernel, dim3(zest_div_up(N * K, 256)), dim3(256), 0, st, workspace,
                           (int)nz, N, K, c, ldc);
    }
}

}  // namespace zest
