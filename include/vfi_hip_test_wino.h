/*
 * vfi_hip_test_wino.h — test taps of the Winograd kernel's dead-plane table (csrc/conv_wino.hip).  Like the taps of vfi_hip_test.h they are
 * compiled under VFI_TEST_TAPS only, i.e. into libvfi_hip_test.so and never into the product library.  They have a header of their own
 * because tests/test_capi_symbols.py::test_header_and_binding_agree spells out the complete list of functions vfi_hip_test.h declares;
 * cfi_amd._lib binds them in a test build beside that list (WINO_TEST_PROTOTYPES).
 */
#ifndef VFI_HIP_TEST_WINO_H
#define VFI_HIP_TEST_WINO_H

#ifdef __cplusplus
extern "C" {
#endif

/* The dead-plane table of the Winograd kernel's transposed-convolution forms (csrc/conv_wino.hip: wino_dead_forms), host only.  A 3x3
 * layer w3_host OIHW [Cout][Cin][3][3] is packed with pack_wino3x3 (Cout padded to 32s, Cin to Cin_p) and the packed image scanned: per
 * 32-channel N block one form — 0 none, 1 / 2 plane row 0 / 3 of U = G g G^T is zero for the whole block, 3 / 4 plane column 0 / 3 is
 * (a row before a column; only exact == 0.0f counts).  Returns the number of blocks written to forms_out or < 0. */
int vfi_test_wino_dead_forms(const float* w3_host, int Cout, int Cin, int Cin_p, int* forms_out, int cap);
/* ... and what a ConvTranspose2d(Cin, LO, 4, 2, 1) layer [Cin][LO][4][4] is launched with (pack_deconv_wino): the forms as the kernel
 * decodes them from its argument words, *gray_out = 1 where the parity groups were packed in the order p00 p01 p11 p10 (chosen only
 * where it skips more planes), and order_out[co] (4 * LO ints, may be NULL) = the row of vfi_test_pack_deconv3x3's w3 that sits at N
 * position co.  Returns the number of blocks or < 0. */
int vfi_test_deconv_wino_plan(const float* weight_host, int Cin, int LO, int* forms_out, int cap, int* gray_out, int* order_out);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_WINO_H */
