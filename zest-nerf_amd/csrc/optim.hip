// Multi-tensor Adam with the global-norm gradient clip applied in the update (reference train.py:265-301: torch.optim.Adam
// over a few hundred fp32 tensors; train.py:1324-1335: Trainer(gradient_clip_val=1) clips the global 2-norm before every
// step).  Per element, torch's arithmetic for amsgrad=False, weight_decay=0, maximize=False:
//   g' = g coef,  m = m + (g' - m)(1 - b1),  v = b2 v + (1 - b2) g'^2
//   p = p - step_size m / (sqrt(v) rbc2 + eps),  step_size = lr / (1 - b1^t),  rbc2 = 1 / sqrt(1 - b2^t)
//   coef = min(1, max_norm / (norm + 1e-6)), norm the 2-norm of every gradient of the step; 1 with the clip off
// A few million elements over tens of MB: as a torch composition the cost is launches, so the launch count here does not
// depend on the number of elements or, up to kMaxTensors tensors, of tensors: the update alone with the clip off; with it
// a first launch that leaves one fp32 sum of squares per chunk, and the update, whose workgroups each add those sums in
// double in one fixed order.  No float atomics: two calls on equal inputs are bit-identical.  Gradients are only read.
//
// The flat element space is cut into chunks of kChunk elements that never span two tensors (zest_adam_plan, host only).
// A workgroup of 256 threads strides over the chunks.  What does not change from step to step lives in device tables:
// per tensor the addresses of p, m, v, the element count and the index of its scalars; per chunk its tensor and its
// offset in it.  What does change, the gradient addresses (zero_grad(set_to_none=True) frees them every step) and the
// per-group, per-t scalars, travels in the launch's argument block: no copy, nothing to synchronise.  The block holds
// kMaxTensors addresses and kMaxSlots rows of scalars; a step with more of either is cut into more launches.
//
// The update kernel is a template on the mode.  AMP = false is the step above.  AMP = true (zest_adam_step_amp) speaks a
// GradScaler's protocol without a host read: the gradients are applied as g / scale, the step is skipped when found_inf
// is non-zero or (skip_nonfinite) the norm is not finite, and, since the host cannot know which steps were skipped, the
// step count lives on the device: the scalars travel raw (lr, b1, b2, eps, 1 - b1, 1 - b2 and the host's count of
// ATTEMPTED steps, as doubles), and one thread per row computes step_size and rbc2 in double from
// t = t_host - skipped into LDS.  `skipped` is two ints: the step of parity k reads skipped[k] in every workgroup and
// thread 0 of workgroup 0 of the first update launch alone writes skipped[k ^ 1]; nothing reads what the step writes.
#include "zest_common.cuh"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 4096;                                // elements; a multiple of 4: chunk starts keep the base's alignment
constexpr int kMaxTensors = 384;                            // 3 KB of gradient addresses in the argument block
constexpr int kMaxSlots = 8;
constexpr long long kMaxGrid = 1024;                        // workgroups of a launch; they stride over the chunks

enum { T_P, T_M, T_V, T_N, T_SLOT };
static_assert(T_SLOT + 1 == ZEST_ADAM_TENSOR_COLS, "ZEST_ADAM_TENSOR_COLS");
enum { S_STEP, S_RBC2, S_EPS, S_OMB1, S_B2, S_OMB2 };
static_assert(S_OMB2 + 1 == ZEST_ADAM_SCALARS, "ZEST_ADAM_SCALARS");
enum { R_LR, R_B1, R_B2, R_EPS, R_OMB1, R_OMB2, R_T };
static_assert(R_T + 1 == ZEST_ADAM_RAW_SCALARS, "ZEST_ADAM_RAW_SCALARS");
static_assert(kChunk % 4 == 0, "a chunk is whole quads");

struct Grads {
    const float *g[kMaxTensors];
};

struct Slots {
    float s[kMaxSlots][ZEST_ADAM_SCALARS];
};

// the second argument of the update kernel: the finished scalars, or what the device makes them from
struct Amp {
    double raw[kMaxSlots][ZEST_ADAM_RAW_SCALARS];
    const float *grad_scale, *found_inf;                    // one value each, or NULL
    const int *skipped_in;                                  // skipped[parity]
    int *skipped_out;                                       // skipped[parity ^ 1] in the first update launch, else NULL
    int n_slots, clip, skip_nonfinite;
};

template <bool AMP>
struct SlotArg {
    typedef Slots type;
};
template <>
struct SlotArg<true> {
    typedef Amp type;
};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// four consecutive floats: one 16-byte access where the address allows it.  Both forms visit the elements in the same
// order, so a result does not depend on where a tensor starts.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *p) {
    if (VEC) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool VEC>
__device__ __forceinline__ void store4(float *p, float4 x) {
    if (VEC) {
        *reinterpret_cast<float4 *>(p) = x;
    } else {
        p[0] = x.x, p[1] = x.y, p[2] = x.z, p[3] = x.w;
    }
}

// the tensor and the extent of chunk c
struct Chunk {
    int tensor, n;
    long long offset;
};

__device__ __forceinline__ Chunk chunk_of(const long long *__restrict__ tens, const int *__restrict__ chunk_tensor,
                                          const long long *__restrict__ chunk_offset, long long c) {
    Chunk k;
    k.tensor = uniform(chunk_tensor[c]);
    k.offset = chunk_offset[c];
    const long long left = tens[(long long)k.tensor * ZEST_ADAM_TENSOR_COLS + T_N] - k.offset;
    k.n = uniform((int)(left < kChunk ? left : kChunk));
    return k;
}

template <bool VEC>
__device__ __forceinline__ float chunk_sumsq(const float *g, int n) {
    const int tid = threadIdx.x, n4 = n >> 2;
    float acc = 0.0f;
    for (int q = tid; q < n4; q += kThreads) {
        const float4 x = load4<VEC>(g + 4 * q);
        acc = fmaf(x.x, x.x, acc), acc = fmaf(x.y, x.y, acc), acc = fmaf(x.z, x.z, acc), acc = fmaf(x.w, x.w, acc);
    }
    if (tid < (n & 3)) {
        const float x = g[4 * n4 + tid];
        acc = fmaf(x, x, acc);
    }
    return acc;
}

// one fp32 sum of squares per chunk of [c0, c1) -> partial[c]
__global__ __launch_bounds__(kThreads) void adam_sumsq_kernel(Grads grads, const long long *__restrict__ tens,
                                                               const int *__restrict__ chunk_tensor,
                                                               const long long *__restrict__ chunk_offset, int t0, long long c0,
                                                               long long c1, float *__restrict__ partial) {
    __shared__ float red[kWaves][1];
    __shared__ float sums[1];
    for (long long c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
        const Chunk k = chunk_of(tens, chunk_tensor, chunk_offset, c);
        const float *g = grads.g[k.tensor - t0] + k.offset;
        float acc[1];
        acc[0] = ((uintptr_t)g & 15) == 0 ? chunk_sumsq<true>(g, k.n) : chunk_sumsq<false>(g, k.n);
        block_sums<1, kWaves>(acc, red, sums);
        if (threadIdx.x == 0) partial[c] = sums[0];
    }
}

__device__ __forceinline__ void adam_element(float g, float &p, float &m, float &v, float coef, const float *s) {
    g *= coef;
    m = m + (g - m) * s[S_OMB1];
    v = s[S_B2] * v + s[S_OMB2] * g * g;
    p = p - s[S_STEP] * (m / (sqrtf(v) * s[S_RBC2] + s[S_EPS]));
}

template <bool VEC>
__device__ __forceinline__ void chunk_update(const float *g, float *p, float *m, float *v, int n, float coef, const float *s) {
    const int tid = threadIdx.x, n4 = n >> 2;
    for (int q = tid; q < n4; q += kThreads) {
        const float4 g4 = load4<VEC>(g + 4 * q);
        float4 p4 = load4<VEC>(p + 4 * q), m4 = load4<VEC>(m + 4 * q), v4 = load4<VEC>(v + 4 * q);
        adam_element(g4.x, p4.x, m4.x, v4.x, coef, s);
        adam_element(g4.y, p4.y, m4.y, v4.y, coef, s);
        adam_element(g4.z, p4.z, m4.z, v4.z, coef, s);
        adam_element(g4.w, p4.w, m4.w, v4.w, coef, s);
        store4<VEC>(p + 4 * q, p4), store4<VEC>(m + 4 * q, m4), store4<VEC>(v + 4 * q, v4);
    }
    if (tid < (n & 3)) {
        const int i = 4 * n4 + tid;
        float pi = p[i], mi = m[i], vi = v[i];
        adam_element(g[i], pi, mi, vi, coef, s);
        p[i] = pi, m[i] = mi, v[i] = vi;
    }
}

// b^t for an integer t >= 1 by repeated squaring, in double (at most 31 squarings)
__device__ __forceinline__ double ipow(double b, int t) {
    double r = 1.0;
    for (; t > 0; t >>= 1, b *= b)
        if (t & 1) r *= b;
    return r;
}

// the sum of the n_partial sums of squares, in double, in one fixed order whatever the workgroup: a thread its strided
// share in index order, the lanes of a wave by butterfly, the waves in turn
__device__ __forceinline__ double total_sumsq(const float *__restrict__ partial, long long n_partial, double *wave_total) {
    const int tid = threadIdx.x;
    double a = 0.0;
    for (long long i = tid; i < n_partial; i += kThreads) a += (double)partial[i];
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) a += __shfl_xor(a, w, 64);
    if ((tid & 63) == 0) wave_total[tid >> 6] = a;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < kWaves; w++) total += wave_total[w];
    return total;
}

// the update of the chunks [c0, c1).  partial: NULL with the clip off; else the n_partial sums of squares of EVERY chunk
// of the step, which each workgroup adds in double in the same order (a thread its strided share in index order, the
// lanes of a wave by butterfly, the waves in turn), so that every workgroup of every launch holds the same coefficient.
// AMP: see the head of the file.  Every workgroup of every launch of a step reads the same scale, found_inf, sums and
// counter, so all of them take the same decision; a skipped step stores nothing but the norm and the counter.
template <bool AMP>
__global__ __launch_bounds__(kThreads) void adam_update_kernel(Grads grads, typename SlotArg<AMP>::type slots,
                                                                const long long *__restrict__ tens,
                                                                const int *__restrict__ chunk_tensor,
                                                                const long long *__restrict__ chunk_offset, int t0, long long c0,
                                                                long long c1, const float *__restrict__ partial,
                                                                long long n_partial, float max_norm, float *__restrict__ norm_out) {
    __shared__ double wave_total[kWaves];
    __shared__ float made[AMP ? kMaxSlots : 1][ZEST_ADAM_SCALARS];
    const int tid = threadIdx.x;
    float coef = 1.0f;
    if constexpr (AMP) {
        const float inv = slots.grad_scale ? (float)(1.0 / (double)slots.grad_scale[0]) : 1.0f;
        bool skip = slots.found_inf && slots.found_inf[0] != 0.0f;
        const int skipped = slots.skipped_in[0];
        double mult = (double)inv;
        if (partial) {
            const double norm = (double)inv * sqrt(total_sumsq(partial, n_partial, wave_total));    // of the unscaled gradients
            if (slots.clip) {
                const double c = (double)max_norm / (norm + 1e-6);
                if (!(c > 1.0)) mult = (double)inv * c;      // a NaN norm gives a NaN multiplier, as torch's clamp does
            }
            if (slots.skip_nonfinite && !(fabs(norm) <= 1.7976931348623157e308)) skip = true;
            if (norm_out && blockIdx.x == 0 && tid == 0) *norm_out = (float)norm;
        }
        coef = (float)mult;
        if (slots.skipped_out && blockIdx.x == 0 && tid == 0) *slots.skipped_out = skipped + (skip ? 1 : 0);
        if (skip) return;                                   // the same in every thread of every workgroup of the step
        if (tid < slots.n_slots) {
            const double *r = slots.raw[tid];
            int t = (int)r[R_T] - skipped;
            t = t < 1 ? 1 : t;
            made[tid][S_STEP] = (float)(r[R_LR] / (1.0 - ipow(r[R_B1], t)));
            made[tid][S_RBC2] = (float)(1.0 / sqrt(1.0 - ipow(r[R_B2], t)));
            made[tid][S_EPS] = (float)r[R_EPS];
            made[tid][S_OMB1] = (float)r[R_OMB1];
            made[tid][S_B2] = (float)r[R_B2];
            made[tid][S_OMB2] = (float)r[R_OMB2];
        }
        __syncthreads();
    } else if (partial) {
        const double norm = sqrt(total_sumsq(partial, n_partial, wave_total)), c = (double)max_norm / (norm + 1e-6);
        coef = c > 1.0 ? 1.0f : (float)c;                   // a NaN norm gives a NaN coefficient, as torch's clamp does
        if (norm_out && blockIdx.x == 0 && tid == 0) *norm_out = (float)norm;
    }
    for (long long c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
        const Chunk k = chunk_of(tens, chunk_tensor, chunk_offset, c);
        const long long *row = tens + (long long)k.tensor * ZEST_ADAM_TENSOR_COLS;
        const float *g = grads.g[k.tensor - t0] + k.offset;
        float *p = (float *)row[T_P] + k.offset, *m = (float *)row[T_M] + k.offset, *v = (float *)row[T_V] + k.offset;
        const float *s;
        if constexpr (AMP)
            s = made[uniform((int)row[T_SLOT])];
        else
            s = slots.s[uniform((int)row[T_SLOT])];
        if ((((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0)
            chunk_update<true>(g, p, m, v, k.n, coef, s);
        else
            chunk_update<false>(g, p, m, v, k.n, coef, s);
    }
}

}  // namespace

extern "C" int zest_adam_chunk(void) { return kChunk; }
extern "C" int zest_adam_max_tensors(void) { return kMaxTensors; }
extern "C" int zest_adam_max_slots(void) { return kMaxSlots; }

extern "C" long long zest_adam_plan(const long long *sizes, int n_tensors, int *chunk_tensor, long long *chunk_offset,
                                    long long capacity) {
    const char *who = "zest_adam_plan";
    if (n_tensors < 0 || (n_tensors > 0 && !sizes) || (!chunk_tensor) != (!chunk_offset) || capacity < 0) {
        zest_set_error("%s: n_tensors=%d, capacity=%lld, or one chunk array without the other", who, n_tensors, capacity);
        return -1;
    }
    long long n = 0;
    for (int t = 0; t < n_tensors; t++) {
        if (sizes[t] < 0) {
            zest_set_error("%s: tensor %d has %lld elements", who, t, sizes[t]);
            return -1;
        }
        for (long long off = 0; off < sizes[t]; off += kChunk, n++) {
            if (!chunk_tensor) continue;
            if (n >= capacity) {
                zest_set_error("%s: more chunks than the capacity %lld", who, capacity);
                return -1;
            }
            chunk_tensor[n] = t, chunk_offset[n] = off;
        }
    }
    return n;
}

extern "C" size_t zest_adam_work_bytes(long long n_chunks) {
    if (n_chunks < 0) {
        zest_set_error("zest_adam_work_bytes: n_chunks=%lld", n_chunks);
        return 0;
    }
    return (size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(float);
}

// the checks and launches of both entries; amp: NULL for zest_adam_step
struct AmpHost {
    const double *raw;
    const int *launch_slots;
    const float *grad_scale, *found_inf;
    int skip_nonfinite;
    int *skipped;
    int parity;
};

static int adam_step_launch(const char *who, const long long *tensors, const int *chunk_tensor, const long long *chunk_offset,
                            int n_launches, const int *launch_tensor, const long long *launch_chunk, const void *const *grads,
                            const float *scalars, int clip, float max_norm, void *work, size_t work_bytes, float *norm_out,
                            const AmpHost *amp, void *stream) {
    ZEST_CHECK_ARG(n_launches >= 0, "%s: n_launches=%d", who, n_launches);
    if (n_launches == 0) return 0;
    ZEST_CHECK_ARG(tensors && chunk_tensor && chunk_offset, "%s: null tensor or chunk table", who);
    ZEST_CHECK_ARG(launch_tensor && launch_chunk && grads && (amp ? (const void *)amp->raw : (const void *)scalars),
                   "%s: null launch bounds, gradient table or scalars", who);
    ZEST_CHECK_ARG(launch_tensor[0] == 0 && launch_chunk[0] == 0, "%s: the launch bounds do not start at 0", who);
    for (int l = 0; l < n_launches; l++) {
        const int nt = launch_tensor[l + 1] - launch_tensor[l];
        ZEST_CHECK_ARG(nt >= 1 && nt <= kMaxTensors, "%s: launch %d holds %d tensors, 1..%d fit", who, l, nt, kMaxTensors);
        ZEST_CHECK_ARG(launch_chunk[l + 1] > launch_chunk[l], "%s: launch %d holds no chunk", who, l);
    }
    const int n_tensors = launch_tensor[n_launches];
    const long long n_chunks = launch_chunk[n_launches];
    for (int t = 0; t < n_tensors; t++) ZEST_CHECK_ARG(grads[t], "%s: gradient %d is null", who, t);
    if (clip)
        ZEST_CHECK_ARG(max_norm >= 0.0f && max_norm <= 3.0e38f, "%s: max_norm %g is not a finite value >= 0", who, (double)max_norm);
    const bool sums = clip || (amp && amp->skip_nonfinite);  // the first launch: for the clip, or to see a norm that is not finite
    if (sums) {
        ZEST_CHECK_ARG(work && norm_out, "%s: null work buffer or norm with the clip%s on", who, amp ? " or skip_nonfinite" : "");
        ZEST_CHECK_ARG(work_bytes >= (size_t)n_chunks * sizeof(float), "%s: work buffer of %zu bytes, %zu needed", who, work_bytes,
                       (size_t)n_chunks * sizeof(float));
    }
    if (amp) {
        ZEST_CHECK_ARG(amp->skipped, "%s: null skipped counter", who);
        ZEST_CHECK_ARG(amp->parity == 0 || amp->parity == 1, "%s: parity %d is not 0 or 1", who, amp->parity);
        ZEST_CHECK_ARG(amp->launch_slots, "%s: null launch_slots", who);
        for (int l = 0; l < n_launches; l++) {
            const int ns = amp->launch_slots[l];
            ZEST_CHECK_ARG(ns >= 1 && ns <= kMaxSlots, "%s: launch %d uses %d rows of scalars, 1..%d fit", who, l, ns, kMaxSlots);
            for (int k = 0; k < ns; k++) {
                const double th = amp->raw[((size_t)l * kMaxSlots + k) * ZEST_ADAM_RAW_SCALARS + R_T];
                ZEST_CHECK_ARG(th >= 1.0 && th <= 2147483647.0 && th == (double)(int)th,
                               "%s: t_host %g of launch %d, row %d is not a whole number >= 1", who, th, l, k);
            }
        }
    }
    float *partial = sums ? (float *)work : nullptr;
    Grads g;
    for (int pass = sums ? 0 : 1; pass < 2; pass++) {
        for (int l = 0; l < n_launches; l++) {
            const int t0 = launch_tensor[l], nt = launch_tensor[l + 1] - t0;
            const long long c0 = launch_chunk[l], c1 = launch_chunk[l + 1];
            for (int t = 0; t < kMaxTensors; t++) g.g[t] = t < nt ? (const float *)grads[t0 + t] : nullptr;
            const unsigned grid = (unsigned)(c1 - c0 < kMaxGrid ? c1 - c0 : kMaxGrid);
            if (pass == 0) {
                hipLaunchKernelGGL(adam_sumsq_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, tensors, chunk_tensor,
                                   chunk_offset, t0, c0, c1, partial);
            } else if (amp) {
                Amp a;
                for (int k = 0; k < kMaxSlots; k++)
                    for (int j = 0; j < ZEST_ADAM_RAW_SCALARS; j++)
                        a.raw[k][j] = amp->raw[((size_t)l * kMaxSlots + k) * ZEST_ADAM_RAW_SCALARS + j];
                a.grad_scale = amp->grad_scale, a.found_inf = amp->found_inf;
                a.skipped_in = amp->skipped + amp->parity;
                a.skipped_out = l == 0 ? amp->skipped + (amp->parity ^ 1) : nullptr;    // once per step, not per launch
                a.n_slots = amp->launch_slots[l], a.clip = clip != 0, a.skip_nonfinite = amp->skip_nonfinite != 0;
                hipLaunchKernelGGL(adam_update_kernel<true>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, a, tensors,
                                   chunk_tensor, chunk_offset, t0, c0, c1, (const float *)partial, n_chunks, max_norm,
                                   l == 0 ? norm_out : nullptr);
            } else {
                Slots s;
                for (int k = 0; k < kMaxSlots; k++)
                    for (int j = 0; j < ZEST_ADAM_SCALARS; j++) s.s[k][j] = scalars[((size_t)l * kMaxSlots + k) * ZEST_ADAM_SCALARS + j];
                hipLaunchKernelGGL(adam_update_kernel<false>, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g, s, tensors,
                                   chunk_tensor, chunk_offset, t0, c0, c1, (const float *)partial, n_chunks, max_norm,
                                   l == 0 ? norm_out : nullptr);
            }
        }
    }
    ZEST_RETURN_LAUNCH(who);
}

extern "C" int zest_adam_step(const long long *tensors, const int *chunk_tensor, const long long *chunk_offset, int n_launches,
                              const int *launch_tensor, const long long *launch_chunk, const void *const *grads,
                              const float *scalars, int clip, float max_norm, void *work, size_t work_bytes,
                              float *norm_out, void *stream) {
    return adam_step_launch("zest_adam_step", tensors, chunk_tensor, chunk_offset, n_launches, launch_tensor, launch_chunk, grads,
                            scalars, clip, max_norm, work, work_bytes, norm_out, nullptr, stream);
}

extern "C" int zest_adam_step_amp(const long long *tensors, const int *chunk_tensor, const long long *chunk_offset, int n_launches,
                                  const int *launch_tensor, const long long *launch_chunk, const int *launch_slots,
                                  const void *const *grads, const double *raw_scalars, int clip, float max_norm, void *work,
                                  size_t work_bytes, float *norm_out, const float *grad_scale, const float *found_inf,
                                  int skip_nonfinite, int *skipped, int parity, void *stream) {
    const AmpHost amp = {raw_scalars, launch_slots, grad_scale, found_inf, skip_nonfinite, skipped, parity};
    return adam_step_launch("zest_adam_step_amp", tensors, chunk_tensor, chunk_offset, n_launches, launch_tensor, launch_chunk,
                            grads, nullptr, clip, max_norm, work, work_bytes, norm_out, &amp, stream);
}
