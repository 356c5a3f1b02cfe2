/*
 * vfi_hip_test_atm.h — the test tap of ATM's multi-scale global-motion ensemble (csrc/atm_net.hip).  Like the taps of vfi_hip_test.h it is
 * compiled under VFI_TEST_TAPS only, i.e. into libvfi_hip_test.so and never into the product library.  It has a header of its own for the
 * reason vfi_hip_test_wino.h has one: tests/test_capi_symbols.py::test_header_and_binding_agree spells out the complete list of functions
 * vfi_hip_test.h declares; cfi_amd._lib binds it in a test build beside that list (ATM_TEST_PROTOTYPES).
 */
#ifndef VFI_HIP_TEST_ATM_H
#define VFI_HIP_TEST_ATM_H

#include "vfi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The record of the last vfi_atm_forward_ensemble on this object to the host: the three alignment losses (levels 0, 1, 2) and the chosen
 * level, as vfi_atm_select_flow wrote them on the device.  Synchronises the stream that forward ran on.  An error before the object's first
 * ensemble forward. */
int vfi_atm_ensemble_record(vfi_atm_t* net, float* losses, int* level);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_ATM_H */
