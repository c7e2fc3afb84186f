// MFMA engine for the width-256 NeRF MLP (bf16 / fp16 / split-fp16 operands): activations stay in registers.
//
// Orientation: Y^T = W X^T with v_mfma_f32_16x16x32_bf16 (under random data the chip holds a higher clock
// on this shape: at identical operand traffic it delivered 5-15 % more FLOP/s here than 32x32x16, cf.
// MI355X_MICROARCH.md "Shape"; its price is issue room - two plain VALU slots per MFMA - so the
// epilogues count their instructions).  A wave owns NB blocks of 32 samples =
// 2 NB column blocks of 16: lane l serves sample column l & 15 of every column block, as group
// g = l >> 4 of four.  The A operand is a pre-packed 1 KiB weight tile (16 output rows x 32
// k-positions, mlp_plan.h) and feeds one MFMA per column block; the B operand is one k-tile of
// a column block's activations, 8 bf16 per lane (positions 8g .. 8g+7).  Two finished 16x16
// accumulator tiles of a row block (4 fp32 per lane each: rows 4g .. 4g+3), biased via their
// initial value, modulated, rectified and rounded to bf16 pairs, ARE one k-tile of the next
// op's B operand: no LDS round trip and no cross-lane traffic between layers
// (cdna_hip_programming.md section 3, "an accumulator tile as the next MFMA's operand"; the k
// permutation that implies is folded into the packed weights).  Row blocks are the outer loop,
// so only four small accumulators (plus four for the modulation) per 32 samples are live next
// to the 64-register input and output operands.
//
// The weight stream (units of 1 KiB in consumption order, mlp_plan.h) comes from a `Tiles`
// source: RingTiles (fused renderer and standalone MLP kernel) reads them from an LDS ring that
// the workgroup's waves keep filled with LDS-DMA (`global_load_lds`), several chunks ahead of
// the MFMAs.  (Reading every unit from global memory in every wave, the first version of the
// standalone kernel, is 2.3x slower.)
#pragma once
#include <hip/hip_bf16.h>
#include "mlp_plan.h"
#include "zest_common.cuh"

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float v4f;
typedef __attribute__((ext_vector_type(4))) unsigned v4u;
typedef const __attribute__((address_space(1))) v4u *gptr_u4;        // global memory, 16-byte units

namespace zest {

// units in the stream of one net (mirror of build_plan for ORDER_ACC, checked on the host)
// (parts: stream units per weight tile, 2 for the split fp16 pair; fold: the inference stream, whose view layer
// carries feature_linear - mlp_plan.h - so the 8 row blocks of op D+1 are absent)
constexpr int stream_units_raw(int nt_pts, int nt_feat, int parts = 1, bool fold = false) {
    const int mod = nt_feat * parts, P = nt_pts * parts, H = 16 * parts;   // mod: modulation units per row block (0 = off)
    return 8 * (1 + mod + P) + 6 * 8 * (1 + mod + H) + 8 * (1 + mod + P + H)   // trunk
           + (1 + H) + (fold ? 0 : 8 * (1 + H)) + 4 * (1 + H + 2 * parts) + (1 + H / 2);     // heads
}
constexpr int stream_units(int nt_pts, int nt_feat, int parts = 1, bool fold = false) {
    return (stream_units_raw(nt_pts, nt_feat, parts, fold) + kStreamAlign - 1) / kStreamAlign * kStreamAlign;
}
static_assert(stream_units_raw(4, 0) == 1262 && stream_units_raw(4, 0, 1, true) == 1126 &&
              stream_units(4, 0, 1, true) == 9 * kStreamAlign, "unit counts of the headline net (DESIGN.md 3.1)");

// ---- weight source: LDS ring fed by LDS-DMA -----------------------------------------------
// The ring holds kRingUnits KiB = kSlots chunks of kChunk units.  All NW waves of the
// workgroup walk the stream in step.  On entering chunk c every wave waits until its own DMA
// pieces of chunk c have landed (counted vmcnt: the younger kAhead-1 chunks stay in flight),
// meets the others at a barrier - after which chunk c is complete and chunk c-1 is no longer
// read by anyone - and issues its share of chunk c+kAhead into the slot that frees.  The
// stream length is a multiple of the ring size, so unit u always sits at ring offset
// u % kRingUnits and passes follow each other without draining the ring.
#ifndef ZEST_CHUNK
#define ZEST_CHUNK 16      // units per chunk (one rendezvous per chunk)
#define ZEST_SLOTS 8       // chunks in the ring
#define ZEST_AHEAD 4       // chunks of DMA kept in flight
#endif
constexpr int kChunk = ZEST_CHUNK, kSlots = ZEST_SLOTS, kRingUnits = kChunk * kSlots, kAhead = ZEST_AHEAD;
static_assert(kStreamAlign % kRingUnits == 0, "stream padding must be a multiple of the ring size");
static_assert(kSlots >= kAhead + 1, "a slot is refilled while the previous chunk may still be read");

#ifndef ZEST_ISSUERS
#define ZEST_ISSUERS 8     // waves of the workgroup that issue the weight DMA (8: every wave its share; 4: waves 0-3,
#endif                     // one per SIMD, take all of it and their SIMD partners 4-7 none - measured in DESIGN.md section 4)
template <int NW, int UNITS_A, int UNITS_B>
struct RingTiles {
    static constexpr int kIssuers = ZEST_ISSUERS < NW ? ZEST_ISSUERS : NW;
    static constexpr int kPieces = kChunk / kIssuers;       // DMA pieces per issuing wave per chunk
    static constexpr int kChunksA = UNITS_A / kChunk, kChunks = (UNITS_A + UNITS_B) / kChunk;
    static_assert(kChunk % kIssuers == 0 && UNITS_A % kRingUnits == 0 && UNITS_B % kRingUnits == 0, "");
    char *ring;            // LDS, kRingUnits KiB, 16-byte aligned
    gptr_u4 src_a, src_b;  // the two nets' streams (src_b unused when UNITS_B == 0)
    int lane, grp, wave;   // grp = lane >> 4; wave: provably uniform (readfirstlane)
    unsigned voff;         // (wave * kPieces * 64 + lane) * 16: this lane's byte offset in a chunk
    unsigned lds_wave_base; // LDS byte address of the ring + wave * kPieces * 1024
#ifdef ZEST_STAMPS         // diagnostic build: cycles spent in enter_chunk (DMA wait + barrier + issue)
    mutable unsigned long long t_wait = 0, t_issue = 0, t_vm = 0;   // t_vm: the vmcnt part of t_wait
#endif

    // LDS-DMA of this wave's pieces of a chunk.  Issued through inline asm so that only the
    // counted waits in enter_chunk govern it: hipcc would otherwise drain vmcnt(0) in front of
    // every ds_read it cannot prove disjoint from the DMA destination
    // (cdna_hip_programming.md 5.7).  M0 = this wave's LDS destination; the instruction offset
    // advances both the global source and the LDS destination, so one M0 write serves all of
    // the wave's pieces.  M0 is not restored: hipcc keeps nothing live in it across an asm
    // statement that declares it clobbered.  Addressing is scalar base + 32-bit lane offset,
    // and the chunk's byte offset is made opaque so the 64-bit adds stay here instead of being
    // hoisted out of the pass loop for all chunks at once (which spills SGPRs to VGPR lanes).
    __device__ __forceinline__ void issue(int chunk) const {      // chunk: compile-time after unrolling
        if (kIssuers < NW && wave >= kIssuers) return;             // wave-uniform: a scalar branch
        const int c = chunk % kChunks;
        unsigned off = (unsigned)((c < kChunksA ? c : c - kChunksA) * kChunk * 1024);
        asm volatile("" : "+s"(off));
        const __attribute__((address_space(1))) char *sb =
            (const __attribute__((address_space(1))) char *)(c < kChunksA ? src_a : src_b) + off;
        const unsigned dst = lds_wave_base + (c % kSlots) * kChunk * 1024;
        static_assert(kPieces == 1 || kPieces == 2 || kPieces == 4, "pieces per wave");
        if (kPieces == 1)
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                         :: "v"(voff), "s"(sb), "s"(dst) : "memory", "m0");
        else if (kPieces == 2)
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\t"
                         "global_load_lds_dwordx4 %0, %1 offset:1024"
                         :: "v"(voff), "s"(sb), "s"(dst) : "memory", "m0");
        else
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\t"
                         "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
                         "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
                         "global_load_lds_dwordx4 %0, %1 offset:3072"
                         :: "v"(voff), "s"(sb), "s"(dst) : "memory", "m0");
    }
    __device__ __forceinline__ void prologue() const {
#pragma unroll
        for (int c = 0; c < kAhead; c++) issue(c);
    }
    __device__ __forceinline__ void enter_chunk(int chunk) const {
#ifdef ZEST_STAMPS
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
        // all but the youngest (kAhead-1)*kPieces of this wave's DMA pieces have landed
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"((kAhead - 1) * kPieces) : "memory");
#ifdef ZEST_STAMPS
        t_vm += __builtin_amdgcn_s_memtime() - t0;
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef ZEST_STAMPS
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
#endif
        issue(chunk + kAhead);
#ifdef ZEST_STAMPS
        t_wait += t1 - t0, t_issue += __builtin_amdgcn_s_memtime() - t1;
#endif
    }
    __device__ __forceinline__ void touch(int unit) const {
        if (unit % kChunk == 0) enter_chunk(unit / kChunk);
    }
    // LDS read addresses: exactly two base registers per access pattern (lower / upper 64 KiB of
    // the ring, the reach of the 16-bit DS offset field), made opaque once.  Left to itself hipcc
    // materialises every `const + lane * 16` beyond the first 64 KiB as a loop-invariant VGPR of
    // its own: ~60 registers of addresses that crowd out operands and end in scratch.
    mutable unsigned rd_lo = 0, rd_hi = 0, rb_lo = 0, rb_hi = 0;
    __device__ __forceinline__ void init_addr() const {
        const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)ring;
        rd_lo = base + lane * 16, rd_hi = rd_lo + 65536, rb_lo = base + grp * 16, rb_hi = rb_lo + 65536;
        asm volatile("" : "+v"(rd_lo), "+v"(rd_hi), "+v"(rb_lo), "+v"(rb_hi));
    }
    static_assert(kRingUnits <= 128, "two 64 KiB windows");
    template <class T>
    static __device__ __forceinline__ const __attribute__((address_space(3))) T *lds_at(unsigned addr) {
        return (const __attribute__((address_space(3))) T *)(uintptr_t)addr;
    }
    __device__ __forceinline__ bf16x8 load(int unit) const {
        touch(unit);
        const int r = unit % kRingUnits;
        const v4u v = *lds_at<v4u>((r < 64 ? rd_lo : rd_hi) + (r % 64) * 1024);
        return *reinterpret_cast<const bf16x8 *>(&v);
    }
    __device__ __forceinline__ f32x4 load_bias(int unit, int which, int rt) const {
        if (which == 0 && rt == 0) touch(unit);     // the other blocks of the header are read right after
        const int r = unit % kRingUnits;
        return *lds_at<v4f>((r < 64 ? rb_lo : rb_hi) + (r % 64) * 1024 + which * 128 + rt * 64);
    }
    // walk the padding [unit, end) of a net's stream so every chunk is entered exactly once
    __device__ __forceinline__ void finish(int unit, int end) const {
#pragma unroll
        for (int u = (unit + kChunk - 1) / kChunk * kChunk; u < end; u += kChunk) enter_chunk(u / kChunk);
    }
    __device__ __forceinline__ void drain() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// ---- operand types ------------------------------------------------------------------------
// EP (engine precision) is one of ZEST_PREC_BF16 / _F16 / _F16X3 (include/zest_render.h).  A tile
// of 8 operand values per lane is 4 VGPRs of 2-byte elements (`bf16x8` is used as the raw
// container for both element types).  ZEST_PREC_F16X3 carries every operand as the pair
// hi = fp16(v), lo = fp16((v - hi) * 2^11): together 22 significant bits.  The lo part is scaled
// so that it stays a normal fp16 number wherever hi is one, and the products that contain it
// are summed in an accumulator of their own that enters the result scaled by 2^-11:
//     sum_k w_k x_k  ~=  sum hi_w hi_x  +  2^-11 (sum hi_w lo_x + sum lo_w hi_x)
// (the dropped lo*lo term is 2^-22 relative).  Three MFMAs per product at the fp16 rate instead
// of one fp32 MFMA at 1/16 of that rate.
constexpr int ep_parts(int EP) { return EP == ZEST_PREC_F16X3 ? 2 : 1; }
constexpr float kLoScale = 2048.0f, kLoUnscale = 1.0f / 2048.0f;

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;

// two fp32 -> one register of two 2-byte elements, round to nearest even: one v_cvt_pk_bf16_f32 /
// v_cvt_pk_f16_f32.  Written as a vector conversion the compiler understands - an inline-asm form
// would read MFMA results without the wait states hipcc inserts for its own instructions (cdna
// guide 5.7 item 2) - and not as __float22bfloat162_rn, which costs 2 cvt + shift + or.
template <int EP>
__device__ __forceinline__ unsigned pack_pair(float lo, float hi) {
    const f32x2_t f = {lo, hi};
    if constexpr (EP == ZEST_PREC_BF16) {
        const bf16x2_t r = __builtin_convertvector(f, bf16x2_t);
        return __builtin_bit_cast(unsigned, r);
    } else {
        const f16x2_t r = __builtin_convertvector(f, f16x2_t);
        return __builtin_bit_cast(unsigned, r);
    }
}
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) { return pack_pair<ZEST_PREC_BF16>(lo, hi); }
__device__ __forceinline__ unsigned short bf16_bits(float v) { return (unsigned short)(pack_bf16(v, 0.f) & 0xFFFFu); }

// the (hi, lo) registers of two values (ZEST_PREC_F16X3)
__device__ __forceinline__ void split_pair(float a, float b, unsigned &hi, unsigned &lo) {
    const f32x2_t f = {a, b};
    const f16x2_t h = __builtin_convertvector(f, f16x2_t);
    const f32x2_t back = __builtin_convertvector(h, f32x2_t);
    const f32x2_t rem = {(a - back[0]) * kLoScale, (b - back[1]) * kLoScale};     // a - hi is exact in fp32
    const f16x2_t l = __builtin_convertvector(rem, f16x2_t);
    hi = __builtin_bit_cast(unsigned, h), lo = __builtin_bit_cast(unsigned, l);
}

template <int EP>
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (EP == ZEST_PREC_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b),
                                                      c, 0, 0, 0);
}

// relu as one v_med3_f32: max(v, 0) for every finite activation (fmaxf costs a second,
// canonicalising v_max in front; med3 against a finite bound is not folded back into it).
// The fp16 modes take the largest fp16 number as the bound: an activation beyond it saturates
// instead of turning into infinity (and NaN one layer later).
template <int EP>
__device__ __forceinline__ float relu1(float v) {
    return __builtin_amdgcn_fmed3f(v, 0.0f, EP == ZEST_PREC_BF16 ? 3.0e38f : 65504.0f);
}

template <int N, int NP = 1>
struct OpArr {              // N k-tiles of one column block's operand in NP parts (hi [, lo]); N = 0 allowed
    bf16x8 t[NP][N > 0 ? N : 1];
};

// eight fp32 values of one lane -> k-tile `k` of an operand
template <int EP, int N>
__device__ __forceinline__ void store_tile(const float (&v)[8], OpArr<N, ep_parts(EP)> &op, int k) {
    if constexpr (EP == ZEST_PREC_F16X3) {
        uint4 h, l;
        split_pair(v[0], v[1], h.x, l.x), split_pair(v[2], v[3], h.y, l.y);
        split_pair(v[4], v[5], h.z, l.z), split_pair(v[6], v[7], h.w, l.w);
        op.t[0][k] = __builtin_bit_cast(bf16x8, h), op.t[1][k] = __builtin_bit_cast(bf16x8, l);
    } else {
        const uint4 q = make_uint4(pack_pair<EP>(v[0], v[1]), pack_pair<EP>(v[2], v[3]), pack_pair<EP>(v[4], v[5]),
                                   pack_pair<EP>(v[6], v[7]));
        op.t[0][k] = __builtin_bit_cast(bf16x8, q);
    }
}

// ReLU of a 16-bit operand tile AFTER rounding, on the packed pairs: a negative bf16 is a negative int16, so
// max(x, 0) per 16-bit half is one v_pk_max_i16 for two values where relu in fp32 costs one v_med3_f32 each.
// Same bits as relu-then-round (rounding keeps the sign; -0 becomes +0 either way).  The engine's issue port
// is the contended resource (MI355X_MICROARCH.md, row 'vector-instruction ISSUE cost': a 16x16x32 MFMA leaves
// room for two plain VALU instructions): this takes 8 of the ~33 VALU instructions of a 256-wide row block away.
typedef __attribute__((ext_vector_type(2))) short s16x2_t;
__device__ __forceinline__ unsigned relu_bf16x2(unsigned u) {
    const s16x2_t r = __builtin_elementwise_max(__builtin_bit_cast(s16x2_t, u), s16x2_t{0, 0});
    return __builtin_bit_cast(unsigned, r);
}
template <int EP, int N>
__device__ __forceinline__ void store_tile_relu16(const float (&v)[8], OpArr<N, 1> &op, int k) {
    const uint4 q = make_uint4(relu_bf16x2(pack_pair<EP>(v[0], v[1])), relu_bf16x2(pack_pair<EP>(v[2], v[3])),
                               relu_bf16x2(pack_pair<EP>(v[4], v[5])), relu_bf16x2(pack_pair<EP>(v[6], v[7])));
    op.t[0][k] = __builtin_bit_cast(bf16x8, q);
}
// fp16 operands take the same packed ReLU (a negative fp16 is a negative int16 as well).  What the fp32 ReLU did on
// top for them - saturate an activation beyond 65504 instead of letting it round to infinity (and NaN one layer
// later) - is done by the hardware: with MODE.FP16_OVFL set an fp16 result that overflows is clamped to +-65504.
// The kernels that run the engine on fp16 operands set the bit once at their start (engine_fp16_overflow_clamp).
__device__ __forceinline__ void engine_fp16_overflow_clamp() {
    __builtin_amdgcn_s_setreg((0 << 11) | (23 << 6) | 1, 1);        // hwreg(HW_REG_MODE, offset 23 = FP16_OVFL, 1 bit) = 1
}

// Weight tiles kept in flight ahead of the MFMAs that consume them: the read-ahead depth PF of engine_layer, a template
// argument per kernel family.  kPrefetch is what the kernels at 229-256 VGPRs can afford.  kPrefetchLone is for the
// kernels with registers to spare (16-bit operands, no features; +12 VGPRs): when its SIMD partner waits at a
// rendezvous or has no block, a wave has the matrix pipe to itself, and 3 tiles = 6 MFMAs (~96 cycles) of cover are
// less than an LDS round trip with eight waves reading.  Depths 3 / 4 / 6 / 8 on the headline kernel (continuous
// window, below): -1.0 / -0.9 / -1.8 / -1.3 % of the step (profiles/ring_protocol_parent_vs_child.txt).
// -DZEST_PREFETCH=n (A/B builds) sets one depth for every kernel.
#ifdef ZEST_PREFETCH
constexpr int kPrefetch = ZEST_PREFETCH, kPrefetchLone = ZEST_PREFETCH;
#else
constexpr int kPrefetch = 3, kPrefetchLone = 6;
#endif

// What is fetched ahead for one row block: its bias initialisers and its first tiles.
template <int NP, int PF>
struct RowBlockPre {
    f32x4 bias[2], mbias[2];      // per row tile
    bf16x8 win[PF][NP];
};

// One Linear: NJB row blocks (32 outputs = row tiles 0, 1) over the operand
// [A (NKA k-tiles) | B (NKB k-tiles)] of each of the CB column blocks.
//   MOD:  the row block is modulated by the feature operand (NKF k-tiles) with the op's
//         modulation tiles
//   MODE: 0 = produce k-tile jb of `out`, 1 = keep row tile 0 of row block 0 in `keep`
//         (head / rgb: lane group g holds rows 4g .. 4g+3)
// Unit order inside a row block: header, then per k-tile the row tiles 0, 1 (modulation k-tiles
// first; a split tile is the unit pair hi, lo): independent accumulators take turns.  The LDS
// reads are software-pipelined by hand, in source order: every tile is requested P = min(PF, tiles of a row block)
// tiles before the MFMAs that use it.
//   CONT = false: the NEXT row block's header and first tiles are requested behind the current row block's last
//         MFMA, before its epilogue, whose VALU instructions cover part of their latency.  The window runs empty at
//         the end of every row block (the listing counts lgkmcnt down to 0 there).
//   CONT = true: the window runs on across the row blocks of a layer: the next row block's header and first tiles
//         are requested inside the current k loop, each P tiles ahead of its MFMAs as every other tile is.  With a
//         partner on the matrix pipe the refill hides behind the partner's MFMAs; a wave alone on its SIMD waits an
//         LDS round trip per row block without it.  Units are still requested in stream order, so every chunk is
//         entered exactly once and in order; no value changes.  The split-fp16 feature kernels and the standalone
//         / training kernels answer with scratch and keep CONT = false.
// A sink sees every finished operand tile of the layers that have one (training: the activation stash):
//   sink(id, jb, cb, v)   id: 0-7 trunk layers, 8 feature_linear, 9 view layer; v: the 8 fp32 values
struct NoSink {
    __device__ __forceinline__ void operator()(int, int, int, const float (&)[8]) const {}
};

// V2: additive modulation (Renderer_linear, networks.py:294) instead of the multiplicative one.  A template
// parameter on purpose: as a launch-time flag, `v2 ? v + m : v * m` per element makes hipcc compute both and select -
// three vector instructions per value where one is needed, 2 048 of the ~5 500 a feature pass issued beside its
// 2 880 MFMAs, on the port the engine is short of (MI355X_MICROARCH.md, 'vector-instruction ISSUE cost') - and a
// scalar branch per row block cuts the unrolled network into basic blocks the register allocator answers with
// ~200 spills.
template <int EP, int CB, int NJB, int NKA, int NKB, bool MOD, int NKF, bool RELU, int MODE, bool V2, int PF, bool CONT,
          class Tiles, class Sink = NoSink>
__device__ __forceinline__ void engine_layer(const Tiles &tiles, int &unit,
                                             const OpArr<NKA, ep_parts(EP)> (&opa)[CB],
                                             const OpArr<NKB, ep_parts(EP)> (&opb)[CB],
                                             const OpArr<NKF, ep_parts(EP)> (&opf)[CB],
                                             OpArr<8, ep_parts(EP)> (&out)[CB], f32x4 (&keep)[CB],
                                             int sink_id = 0, const Sink &sink = Sink()) {
    constexpr int NP = ep_parts(EP);
    constexpr bool X3 = EP == ZEST_PREC_F16X3;
    constexpr int NM = MOD ? 2 * NKF : 0, T = NM + 2 * (NKA + NKB);     // tiles per row block
    static_assert(T >= 1, "empty layer");
    // a sink wants the activated fp32 values: only the plain inference layer rounds first
    constexpr bool kPackedRelu = RELU && MODE == 0 && EP != ZEST_PREC_F16X3 && __is_same(Sink, NoSink);
    constexpr int P = PF < T ? PF : T;                          // tiles in flight in this layer
    auto preload_header = [&](RowBlockPre<NP, PF> &p, int u0) {   // u0: the row block's header unit
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
            p.bias[rt] = tiles.load_bias(u0, 0, rt);
            if (MOD) p.mbias[rt] = tiles.load_bias(u0, 1, rt);
        }
    };
    auto preload_tile = [&](RowBlockPre<NP, PF> &p, int u0, int k) {
#pragma unroll
        for (int pt = 0; pt < NP; pt++) p.win[k][pt] = tiles.load(u0 + 1 + NP * k + pt);
    };
    auto preload = [&](RowBlockPre<NP, PF> &p, int u0) {
        preload_header(p, u0);
#pragma unroll
        for (int k = 0; k < P; k++) preload_tile(p, u0, k);
    };
    RowBlockPre<NP, PF> pre;
    preload(pre, unit);
#pragma unroll
    for (int jb = 0; jb < NJB; jb++) {
        const int u0 = unit;
        // acc: the hi*hi products (all products of the one-part types); corr: hi*lo + lo*hi, scaled 2^11
        f32x4 acc[2][CB], macc[2][CB], corr[2][CB], mcorr[2][CB];
        bf16x8 win[P][NP];
#pragma unroll
        for (int k = 0; k < P; k++)
#pragma unroll
            for (int pt = 0; pt < NP; pt++) win[k][pt] = pre.win[k][pt];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int cb = 0; cb < CB; cb++) {
                acc[rt][cb] = pre.bias[rt];
                if (MOD) macc[rt][cb] = pre.mbias[rt];
                if (X3) corr[rt][cb] = f32x4{0.f, 0.f, 0.f, 0.f}, mcorr[rt][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
        for (int k = 0; k < T; k++) {
            bf16x8 a[NP];
#pragma unroll
            for (int pt = 0; pt < NP; pt++) a[pt] = win[k % P][pt];
            const int rt = k % 2, kt = (k < NM ? k : k - NM) / 2;          // compile-time after unrolling
#pragma unroll
            for (int cb = 0; cb < CB; cb++) {
                // the operand k-tile this weight tile multiplies, part pt (every index is a
                // compile-time constant after unrolling; the clamps keep dead branches in range)
                auto opnd = [&](int pt) -> bf16x8 {
                    if (k < NM) return opf[cb].t[pt][k < NM ? kt : 0];
                    if (kt < NKA) return opa[cb].t[pt][(k >= NM && kt < NKA) ? kt : 0];
                    return opb[cb].t[pt][(k >= NM && kt >= NKA) ? kt - NKA : 0];
                };
                if (k < NM) {
                    macc[rt][cb] = mfma16<EP>(a[0], opnd(0), macc[rt][cb]);
                    if constexpr (X3) {
                        mcorr[rt][cb] = mfma16<EP>(a[0], opnd(NP - 1), mcorr[rt][cb]);
                        mcorr[rt][cb] = mfma16<EP>(a[NP - 1], opnd(0), mcorr[rt][cb]);
                    }
                } else {
                    acc[rt][cb] = mfma16<EP>(a[0], opnd(0), acc[rt][cb]);
                    if constexpr (X3) {
                        corr[rt][cb] = mfma16<EP>(a[0], opnd(NP - 1), corr[rt][cb]);
                        corr[rt][cb] = mfma16<EP>(a[NP - 1], opnd(0), corr[rt][cb]);
                    }
                }
            }
            if (k + P < T) {
#pragma unroll
                for (int pt = 0; pt < NP; pt++) win[k % P][pt] = tiles.load(u0 + 1 + NP * (k + P) + pt);
            } else if (CONT && jb + 1 < NJB) {                  // tile k + P - T of the next row block
                if (k + P == T) preload_header(pre, u0 + 1 + NP * T);
                preload_tile(pre, u0 + 1 + NP * T, k + P - T);
            }
        }
        unit = u0 + 1 + NP * T;
        if (!CONT && jb + 1 < NJB) preload(pre, unit);          // in flight during the epilogue
#pragma unroll
        for (int cb = 0; cb < CB; cb++) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                v[i] = acc[i >> 2][cb][i & 3];
                if (X3) v[i] = fmaf(corr[i >> 2][cb][i & 3], kLoUnscale, v[i]);
            }
            if (MOD) {
                float mv[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    mv[i] = macc[i >> 2][cb][i & 3];
                    if (X3) mv[i] = fmaf(mcorr[i >> 2][cb][i & 3], kLoUnscale, mv[i]);
                }
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = V2 ? v[i] + mv[i] : v[i] * mv[i];
            }
            if (RELU && !kPackedRelu) {
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = relu1<EP>(v[i]);
            }
            if (MODE == 0) {
                if constexpr (kPackedRelu) store_tile_relu16<EP>(v, out[cb], jb);
                else store_tile<EP>(v, out[cb], jb);
                sink(sink_id, jb, cb, v);
            } else if (jb == 0) {
                keep[cb] = f32x4{v[0], v[1], v[2], v[3]};
            }
        }
    }
}

// The whole network for CB column blocks of 16 samples, reading the stream from unit `unit` on
// (advanced to the end of the net's padded stream).  pts/feat: encoder operands in plan position
// order, NU_* = their logical stream tiles per row block = 2 x k-tiles.  `pts_fn(pts)` builds the
// point operand.  It is called twice, for layer 0 and for the skip layer 5, each time into an operand that
// lives for that layer only, so the engine holds no point operand of its own through layers 1-4.  Keep the
// two calls: the standalone kernel (mlp_engine.hip) relies on them to have those registers free in between,
// and the callers (all of which build the operand once and hand out copies) are tuned to this shape.
// `views_fn(views)` builds the direction operand when it is first needed (op 10).
// Results per column block: head (lane group g: rows 4g .. 4g+3 of the head
// tile; row 0 alpha, rows 1.. extra heads) and rgb (group 0: rows 0-2), raw.
// PF, CONT: read-ahead depth and window shape of every layer (engine_layer), chosen per kernel family.
// FOLD: the stream is the inference stream (mlp_plan.h): no feature_linear layer (sink id 8 is never seen), the
// view layer multiplies the trunk output itself.  The training forward, whose backward needs the feature_linear
// output in the stash, runs FOLD = false on the plain stream.
template <int EP, int CB, int NU_PTS, bool MOD, int NU_FEAT, bool V2, bool FOLD = false, int PF = kPrefetch,
          bool CONT = false, class Tiles, class PtsFn, class ViewsFn, class Sink = NoSink>
__device__ __forceinline__ void engine_forward(const Tiles &tiles, int &unit, PtsFn pts_fn,
                                               const OpArr<NU_FEAT / 2, ep_parts(EP)> (&feat)[CB], ViewsFn views_fn,
                                               f32x4 (&head)[CB], f32x4 (&rgb)[CB], const Sink &sink = Sink()) {
    constexpr int KP = NU_PTS / 2, KF = NU_FEAT / 2, NP = ep_parts(EP);
    static_assert(NU_PTS % 2 == 0 && NU_FEAT % 2 == 0, "units per row block come in row-tile pairs");
    OpArr<8, NP> hA[CB], hB[CB];
    OpArr<0, NP> none[CB];
    f32x4 unused[CB];
    const int unit0 = unit;
    {
        OpArr<KP, NP> pts[CB];
        pts_fn(pts);
        engine_layer<EP, CB, 8, KP, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, pts, none, feat, hA, unused, 0, sink);
    }
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hA, none, feat, hB, unused, 1, sink);
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hB, none, feat, hA, unused, 2, sink);
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hA, none, feat, hB, unused, 3, sink);
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hB, none, feat, hA, unused, 4, sink);
    {
        OpArr<KP, NP> pts[CB];
        pts_fn(pts);
        engine_layer<EP, CB, 8, KP, 8, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, pts, hA, feat, hB, unused, 5, sink);
    }
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hB, none, feat, hA, unused, 6, sink);
    engine_layer<EP, CB, 8, 8, 0, MOD, KF, true, 0, V2, PF, CONT>(tiles, unit, hA, none, feat, hB, unused, 7, sink);
    // trunk output in hB
    engine_layer<EP, CB, 1, 8, 0, false, KF, false, 1, V2, PF, CONT>(tiles, unit, hB, none, feat, hA, head);
    if constexpr (!FOLD)
        engine_layer<EP, CB, 8, 8, 0, false, KF, false, 0, V2, PF, CONT>(tiles, unit, hB, none, feat, hA, unused, 8, sink);
    // view layer: on the feature_linear output (hA -> hB), or folded on the trunk output itself (hB -> hA)
    OpArr<8, NP> (&vin)[CB] = FOLD ? hB : hA, (&vout)[CB] = FOLD ? hA : hB;
    OpArr<1, NP> views[CB];
    views_fn(views);
    engine_layer<EP, CB, 4, 8, 1, false, KF, true, 0, V2, PF, CONT>(tiles, unit, vin, views, feat, vout, unused, 9, sink);
    // rgb: 128 hidden features = first 4 k-tiles of the view layer's output
    OpArr<4, NP> h128[CB];
#pragma unroll
    for (int cb = 0; cb < CB; cb++)
#pragma unroll
        for (int pt = 0; pt < NP; pt++)
#pragma unroll
            for (int k = 0; k < 4; k++) h128[cb].t[pt][k] = vout[cb].t[pt][k];
    engine_layer<EP, CB, 1, 4, 0, false, KF, false, 1, V2, PF, CONT>(tiles, unit, h128, none, feat, vin, rgb);
    tiles.finish(unit, unit0 + stream_units(NU_PTS, MOD ? NU_FEAT : 0, NP, FOLD));
    unit = unit0 + stream_units(NU_PTS, MOD ? NU_FEAT : 0, NP, FOLD);
}

// standalone launcher (mlp.hip -> zest_mlp_fwd)
int mlp_engine_launch(const MlpPlan &p, const void *tiles, const float *x, int M, float *out,
                    hipStream_t stream);

}  // namespace zest
