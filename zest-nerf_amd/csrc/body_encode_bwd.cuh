// Backward of the encoding-volume lookup and the positional encoding (encode_kernel).
// A kernel BODY, included as text between the braces of a __global__ function whose parameters carry the names used
// here (g_x, ndc, R, S, has_time, vol, D, Hv, Wv, V, g_ndc, g_vol), after
//     #define ZEST_GRAD_ADD(p, v)   how the float v is added into *p
// The default kernel (encode.hip) defines it as atomicAdd(p, v) - its device code is what it was when this text stood in the
// kernel itself (profiles/device_code_identity_deterministic.txt); the order-independent kernel of det_grads.hip adds v
// in 64-bit fixed point (fixed_accum.cuh).  Both compute v with the same fp32 expression.
//
// Backward of encode_kernel for the inputs that carry gradients in the reference's training
// graph: the volume coordinates (through the positional encoding and through the trilinear
// lookup's dependence on them - needed for the scene-flow displaced points, renderer.py:461,488)
// and the encoding volume itself (scatter-add; MVSNet trains through it).  World points, source
// images, cameras and ray directions are data and receive no gradient.
// Eight lanes per sample (lane & 7 = volume channel): a corner's scatter-add is then 8 adjacent floats = one
// 32-byte segment per sample and 8 segments per wave instruction, instead of 64 single floats in 64 different
// rows (the shape at which memory-side float atomics run at 1/17 of their rate: the first version of this
// kernel spent 0.45 ms per 1024 x 128 batch on them).  The octet's lanes 0-2 also take one coordinate each of
// the positional-encoding part; the per-corner dot products are reduced over the octet with shuffles.
// A contribution to the volume is w g with w = wx wy wz and every factor in [0, 1] (t = f - floor(f) and 1 - t): |w g| <= |g|
// after every rounding, so the constant factor of the fixed-point bound is c = 1.
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long m_raw = tid >> 3;
    const int ch = (int)(tid & 7);
    const bool live = m_raw < (long long)R * S;
    const long long m = live ? m_raw : 0;                     // idle octets compute on sample 0 and store nothing
    const int C = 3 + has_time;
    const int P = C * 21, F = vol ? 8 + 4 * V : 0;
    const float *row = g_x + (size_t)m * (P + F + 27);
    const float p[3] = {ndc[3 * m], ndc[3 * m + 1], ndc[3 * m + 2]};
    float gpe = 0.0f;                                          // lanes 0-2: d / d coordinate ch through the encoding
    if (ch < 3) {
        float acc = row[ch], f = 1.0f;
        for (int k = 0; k < 10; k++) {
            float sn, cs;
            zest_sincos(p[ch] * f, &sn, &cs);
            acc += f * (cs * row[C * (1 + 2 * k) + ch] - sn * row[C * (2 + 2 * k) + ch]);
            f *= 2.0f;
        }
        gpe = acc;
    }
    float dxs = 0.f, dys = 0.f, dzs = 0.f;
    if (vol) {
        const float gf = row[P + ch];
        const float fx = zest_unnorm(p[0], Wv), fy = zest_unnorm(p[1], Hv), fz = zest_unnorm(p[2], D);
        const bool inside = fx > -2.0f && fx < (float)Wv + 1.0f && fy > -2.0f && fy < (float)Hv + 1.0f &&
                            fz > -2.0f && fz < (float)D + 1.0f;
        const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
        const float tx = fx - x0f, ty = fy - y0f, tz = fz - z0f;
        const int x0 = inside ? (int)x0f : -8, y0 = inside ? (int)y0f : -8, z0 = inside ? (int)z0f : -8;
        const float *volf = reinterpret_cast<const float *>(vol);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
            const int xi = x0 + dx, yi = y0 + dy, zi = z0 + dz;
            const bool ok = (unsigned)xi < (unsigned)Wv && (unsigned)yi < (unsigned)Hv && (unsigned)zi < (unsigned)D;
            const size_t vox = ok ? zest_vox(zi, yi, xi, D, Wv) : 0;
            const float wx = dx ? tx : 1.0f - tx, wy = dy ? ty : 1.0f - ty, wz = dz ? tz : 1.0f - tz;
            float dot = ok ? volf[8 * vox + ch] * gf : 0.0f;                    // octet-uniform `ok`
            dot += __shfl_xor(dot, 1, 64), dot += __shfl_xor(dot, 2, 64), dot += __shfl_xor(dot, 4, 64);
            dxs += (dx ? 1.0f : -1.0f) * wy * wz * dot;
            dys += (dy ? 1.0f : -1.0f) * wx * wz * dot;
            dzs += (dz ? 1.0f : -1.0f) * wx * wy * dot;
            if (g_vol && ok && live) ZEST_GRAD_ADD(g_vol + 8 * vox + ch, wx * wy * wz * gf);
        }
    }
    if (live && ch < 3) {
        const float scale = ch == 0 ? (float)(Wv - 1) : (ch == 1 ? (float)(Hv - 1) : (float)(D - 1));
        const float dv = ch == 0 ? dxs : (ch == 1 ? dys : dzs);
        g_ndc[3 * m + ch] = gpe + (vol ? dv * scale : 0.0f);
    }
