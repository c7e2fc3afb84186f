// The plane sweep's projection and bilinear taps, shared by its kernels (volume_cost.hip) and the order-independent
// forms of their backward (det_grads.hip).
#pragma once
#include "zest_common.cuh"

constexpr int kC = 32;               // feature channels of FeatureNet's top level
constexpr int kMaxViews = 8;
constexpr int kRowStride = 66;      // row stride (floats) of the backward kernel's LDS transpose tile

struct Tap4 {                        // bilinear taps, zero padding, align_corners (grid_sample)
    int off[4];                      // pixel offsets y * W + x (clamped when the weight is 0)
    float w[4];
};

// Source-view sampling position of reference pixel (xr, yr) on the plane at `depth`, following
// homo_warp's arithmetic: p = R [xr, yr, 1]^T + T / depth; (sx, sy) = p.xy / p.z; normalised to
// [-1, 1] (the in-frame mask is taken on the normalised value, strictly inside) and mapped
// back to pixels as grid_sample(align_corners=True) does.
__device__ __forceinline__ void project(const float *__restrict__ P, float xr, float yr, float depth,
                                        int H, int W, float &gx, float &gy) {
    const float X = fmaf(P[0], xr, fmaf(P[1], yr, P[2])) + P[3] / depth;
    const float Y = fmaf(P[4], xr, fmaf(P[5], yr, P[6])) + P[7] / depth;
    const float Z = fmaf(P[8], xr, fmaf(P[9], yr, P[10])) + P[11] / depth;
    gx = (X / Z) / ((float)(W - 1) / 2.0f) - 1.0f;
    gy = (Y / Z) / ((float)(H - 1) / 2.0f) - 1.0f;
}

__device__ __forceinline__ Tap4 taps(float gx, float gy, int H, int W) {
    Tap4 t;
    float px = (gx + 1.0f) * 0.5f * (float)(W - 1), py = (gy + 1.0f) * 0.5f * (float)(H - 1);
    // NaN / far-away positions (a plane behind the source camera): no contribution
    const bool finite = fabsf(px) < 1e8f && fabsf(py) < 1e8f;
    px = finite ? px : -4.0f, py = finite ? py : -4.0f;
    const float x0f = floorf(px), y0f = floorf(py);
    const float tx = px - x0f, ty = py - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int dx = c & 1, dy = c >> 1, xi = x0 + dx, yi = y0 + dy;
        const bool ok = (unsigned)xi < (unsigned)W && (unsigned)yi < (unsigned)H;
        t.w[c] = ok ? (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty) : 0.0f;
        t.off[c] = min(max(yi, 0), H - 1) * W + min(max(xi, 0), W - 1);
    }
    return t;
}
