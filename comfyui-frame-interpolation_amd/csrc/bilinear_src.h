// The source taps of torch's bilinear F.interpolate(scale_factor=s, align_corners=False) along one axis, shared by resize_ratio_kernel
// (ifrnet_ops.hip) and amt_upsample_lrelu_kernel (amt_net.hip) so that the arithmetic exists once.
#pragma once
#include <hip/hip_runtime.h>

namespace vfi {

// torch area_pixel_compute_source_index(ratio, dst, align_corners=False) + guard_index_and_lambda, with the ratio the
// caller derived from the user's scale_factor (F.interpolate(scale_factor=s) passes 1/s, not in/out)
struct BilS {
    int i0, i1;
    float w0, w1;
};
__device__ static inline BilS bil_src(int d, float ratio, int in_size) {
    float src = __fsub_rn(__fmul_rn(ratio, __fadd_rn((float)d, 0.5f)), 0.5f);
    if (src < 0.f) src = 0.f;
    int i0 = (int)floorf(src);
    if (i0 > in_size - 1) i0 = in_size - 1;
    const float l = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
    BilS b;
    b.i0 = i0;
    b.i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    b.w1 = l;
    b.w0 = __fsub_rn(1.0f, l);
    return b;
}
}  // namespace vfi
