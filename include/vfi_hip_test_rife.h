/*
 * vfi_hip_test_rife.h — test tap of RIFE's fused block 1->2 transition (csrc/rife_ops.hip: trans2_conv0a_kernel), the sibling of
 * vfi_test_rife_trans1_conv0a.  Like the taps of vfi_hip_test.h it is compiled under VFI_TEST_TAPS only, i.e. into libvfi_hip_test.so and
 * never into the product library.  It has a header of its own because tests/test_capi_symbols.py::test_header_and_binding_agree spells
 * out the complete list of functions vfi_hip_test.h declares; cfi_amd._lib binds it in a test build beside that list (RIFE_TEST_PROTOTYPES).
 */
#ifndef VFI_HIP_TEST_RIFE_H
#define VFI_HIP_TEST_RIFE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The block transition 4 -> 2 fused into block 2's conv0.0, on caller buffers (device pointers except the weights):
 *   Fout = Fin + up(T, 4) * 4 over [B][Hp][Wp][4] (Fin is only read, Fout != Fin);
 *   A0   = LeakyReLU(conv0.0(X) + bias, slope) as NHWC [B][Hp/4][Wp/4][48], X being the 20-channel input of the scale-2 block.
 * T is the planar4 output of the scale-4 block, [B][2][Hp/4][Wp/4][4].  w_oihw_host [48][20][3][3] and bias_host [48] are HOST arrays,
 * packed here as vfi_rife_create packs them.  B in 1..32, Hp and Wp multiples of 64, slope in [0,1]; anything else returns an error
 * before any launch.  Synchronises `stream`. */
int vfi_test_rife_trans2_conv0a(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* T,
                                const float* Fin, float* Fout, const float* w_oihw_host, const float* bias_host, float* A0, int Hp, int Wp, float slope,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_RIFE_H */
