// Backward of homo_warp.
// A kernel BODY, included as text between the braces of a __global__ function whose parameters carry the names used
// here (proj, depth, grid_in, C, D, H, W, Hp, Wp, pad, g_warped, g_src), after
//     #define ZEST_GRAD_ADD(p, v)   how the float v is added into *p
// The default kernel (volume_cost.hip) defines it as atomicAdd(p, v) - its device code is what it was when this text stood in the
// kernel itself (profiles/device_code_identity_deterministic.txt); the order-independent kernel of det_grads.hip adds v
// in 64-bit fixed point (fixed_accum.cuh).  Both compute v with the same fp32 expression.
//
// backward of homo_warp with respect to the source map: g_warped [C,D,Hp,Wp] -> g_src [C,H,W]
// (accumulated: zero it first).  The sampling positions (grid or homography + depths) are data.
// A contribution is w g with a bilinear weight w in [0, 1]: c = 1, as for the lookup.
    const long long nvox = (long long)D * Hp * Wp;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nvox) return;
    float gx, gy;
    if (grid_in) {
        gx = grid_in[2 * idx], gy = grid_in[2 * idx + 1];
    } else {
        const unsigned row = (unsigned)idx / (unsigned)Wp;
        const int x = (int)((unsigned)idx - row * (unsigned)Wp), d = (int)(row / (unsigned)Hp), y = (int)(row - (unsigned)d * (unsigned)Hp);
        project(proj, (float)(x - pad), (float)(y - pad), depth[d], H, W, gx, gy);
    }
    const Tap4 t = taps(gx, gy, H, W);
    for (int c = 0; c < C; c++) {
        const float g = g_warped[(size_t)c * nvox + idx];
        float *s = g_src + (size_t)c * H * W;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (t.w[k] != 0.0f) ZEST_GRAD_ADD(s + t.off[k], t.w[k] * g);
    }
