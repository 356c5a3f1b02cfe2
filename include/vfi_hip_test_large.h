/*
 * vfi_hip_test_large.h — test tap of the layer objects' LARGE kernel forms (csrc/conv_mfma2.hip, conv_wino.hip).  Like the taps of
 * vfi_hip_test.h it is compiled under VFI_TEST_TAPS only, i.e. into libvfi_hip_test.so and never into the product library.  It has a header
 * of its own because tests/test_capi_symbols.py::test_header_and_binding_agree spells out the complete list of functions vfi_hip_test.h
 * declares; cfi_amd._lib binds it in a test build beside that list (LARGE_TEST_PROTOTYPES).
 */
#ifndef VFI_HIP_TEST_LARGE_H
#define VFI_HIP_TEST_LARGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every launch of a LARGE kernel form this thread has made since the last call of this function, oldest first: 6 ints per launch
 * (family 2 = second-generation direct kernel, 3 = Winograd; Hin, Win, in_cs, Cin_p, Cout), at most cap_entries of them written to `out`;
 * the log (256 launches at most) is emptied.  vfi_test_last_conv_launch keeps the last launch only: this is a whole network's worth.
 * Returns the number of launches logged.  Host only. */
int vfi_test_large_launches(int32_t* out, int cap_entries);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_LARGE_H */
