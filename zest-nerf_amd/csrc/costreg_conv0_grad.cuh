// What the two gradient kernels of CostRegNet.conv0 share (costreg_wgrad.hip, costreg_dgrad.hip): the layer's shape
// and the refusals both entry points make before a launch.
#pragma once
#include "mlp_engine.cuh"

namespace zest {

constexpr int kCO = 8, kCI = 48, kTaps = 27;     // output channels, padded input channels, 3 x 3 x 3 taps

// The refusals of zest_costreg_wgrad / zest_costreg_dgrad, in the order both make them; `who` is the entry point's
// name, `operands` names the pointers that must be 16-byte aligned.  extents_ok: the file's own check of D, H, W.
inline int conv0_grad_refusal(const char *who, int cin, int cout, bool extents_ok, int D, int H, int W, bool no_null,
                              bool all_aligned, const char *operands) {
    ZEST_CHECK_ARG(cout == kCO, "%s: %d output channels, the kernel is built for %d", who, cout, kCO);
    ZEST_CHECK_ARG(cin >= 1 && cin <= kCI, "%s: %d input channels, expected 1 .. %d", who, cin, kCI);
    ZEST_CHECK_ARG(extents_ok, "%s: bad shape %d x %d x %d", who, D, H, W);
    ZEST_CHECK_ARG(no_null, "%s: null pointer", who);
    ZEST_CHECK_ARG(all_aligned, "%s: %s must be 16-byte aligned", who, operands);
    return 0;
}

}  // namespace zest
