// Backward through relu(mod(pre, m)) with the bias gradient folded in.
// A kernel BODY, included as text between the braces of a __global__ function with the parameters d, pre, m, dm, M, N,
// v2, after
//     #define ZEST_BIAS_SUM(n, acc)   where the block's sum `acc` of column n goes
// mlp_train.hip adds it into db[n] with a float atomic - its device code is what it was when this text stood in the
// kernel itself (profiles/device_code_identity_deterministic.txt); det_grads.hip stores it as the block's own partial
// for a second launch to add in block order.
//
// d (in: dL/dact, out: dL/dpre) and dm += dL/dm, through relu(mod(pre, m)), with the bias gradient
// folded in: db[n] += sum over the block's rows of dL/dpre.
// One thread per column (N = 128 or 256 columns = blockDim.x), kBwdRows rows per block: the
// separate column-sum pass over dL/dpre (11 % of a training step) disappears.
    const int n = threadIdx.x;
    const int m0 = blockIdx.x * kBwdRows, m1 = min(m0 + kBwdRows, M);
    float acc = 0.f;
    for (int r = m0; r < m1; r++) {
        const size_t i = (size_t)r * N + n;
        const float p = pre[i], g = d[i];
        float out;
        if (!m) {
            out = p > 0.f ? g : 0.f;
        } else {
            const float mv = m[i];
            const bool on = (v2 ? p + mv : p * mv) > 0.f;
            const float go = on ? g : 0.f;
            out = v2 ? go : go * mv;
            dm[i] += v2 ? go : go * p;
        }
        d[i] = out;
        acc += out;
    }
    ZEST_BIAS_SUM(n, acc);
