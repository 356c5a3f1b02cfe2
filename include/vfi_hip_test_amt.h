/*
 * vfi_hip_test_amt.h — test taps of the two AMT kernels that have no entry point of their own (csrc/amt_net.hip): amt_add_kernel (channel-window
 * copies, stride-2 sub-sampling, residual sums) and amt_warp_kernel.  Like the taps of vfi_hip_test.h they are compiled under VFI_TEST_TAPS
 * only, i.e. into libvfi_hip_test.so and never into the product library.  They have a header of their own for the reason vfi_hip_test_wino.h
 * has one: tests/test_capi_symbols.py::test_header_and_binding_agree spells out the complete list of functions vfi_hip_test.h declares;
 * cfi_amd._lib binds them in a test build beside that list (AMT_TEST_PROTOTYPES).  Each is the launch the forward itself issues (the net's
 * Run::add / Run::warp): same kernel, same grid.
 */
#ifndef VFI_HIP_TEST_AMT_H
#define VFI_HIP_TEST_AMT_H

#include "vfi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[y, x, r * C + c] = a[y * step, x * step, r * C + c] (+ b[y, x, c] when b is not null) for r < reps, c < C: a [., a_w, a_cs] is read at
 * every step-th row and column, b [h, w, b_cs], out [h, w, out_cs].  b null: a copy.  out may be a (the forward's in-place sums). */
int vfi_test_amt_add(const float* a_dev, int a_cs, int a_w, int step, const float* b_dev, int b_cs, float* out_dev, int out_cs, int h, int w, int C,
                     int reps, void* stream);
/* amt_arch.warp (:26-34) of the C-channel window in [H, W, in_cs] by the 2-channel flow window [H, W, flow_cs] into out [H, W, out_cs]:
 * bilinear, border padding, align_corners = True. */
int vfi_test_amt_warp(const float* in_dev, int in_cs, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_AMT_H */
