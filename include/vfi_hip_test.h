/*
 * vfi_hip_test.h — TEST TAPS: entry points that exist for the parity tests and A/B tools only (a naive cross-check convolution,
 * read-back of internal tensors, switches between two correct kernel forms).  They are NOT in the product library: csrc/build.py
 * compiles them (`#ifdef VFI_TEST_TAPS`) into a second library, libvfi_hip_test.so — the product objects + these — which
 * tests/conftest.py and tools/ select with cfi_amd._lib.use_test_build().  libvfi_hip.so exports exactly include/vfi_hip.h
 * (tests/test_capi_symbols.py::test_product_library_has_no_test_taps): nothing loaded beside a node can flip a model's kernel choice.
 * (Per-kernel tracing, vfi_trace_*, the clock probe and vfi_rife_work stay in vfi_hip.h: bench.py's roofline figures are part of
 * the deliverable, and none of them changes a result.)
 */
#ifndef VFI_HIP_TEST_H
#define VFI_HIP_TEST_H

#include "vfi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Same contract as vfi_conv3x3, straightforward one-thread-per-output FMA kernel (cross-check of the MFMA path). */
int vfi_conv3x3_naive(const float* in_dev, const float* weight_host, const float* bias_host,
                      const float* beta_host, float* out_dev, int N, int H, int W, int Cin,
                      int Cout, int stride, int act, float slope, void* stream);


/* Algorithm choice of the 3x3 stride-1 layers (layer objects and the RIFE network): 0 automatic (Winograd where the launch has
 * enough work items), 1 direct implicit-GEMM kernel only, 2 Winograd wherever the shape allows, 3 as 2 with 32x4 regions wherever the
 * launcher picks the region shape itself (the region shape changes no bit); mode < 0 queries.  Returns the
 * mode in force.  Lets a test run BOTH forms of one layer / network on one input. */
int vfi_test_conv_algo(int mode);

/* The Winograd F(2x2,3x3) weight pack of a 3x3 layer (csrc/conv_wino.hip: U = G g G^T, layout
 * [Cout_p/32][Cin_p/8][j][xi/4][half][co%32][xi%4], physical input channel = c8*8 + half*4 + j), written to a HOST buffer: lets the
 * CPU suite check the pack and emulate the kernel's addressing (tests/test_wino_emulation.py).  Returns floats written or < 0. */
int64_t vfi_test_pack_wino3x3(const float* weight_host, int Cout, int Cin, const int* chan_map, int Cin_p, float* out_host, int64_t cap);
/* ConvTranspose2d(Cin, LO, 4, 2, 1) rewritten as ONE 3x3 stride-1 pad-1 convolution with 4 * LO output channels (channel g * LO + co =
 * output parity g = 2 py + px of channel co; csrc/conv_wino.hip: pack_deconv_as_conv3x3 — how the RIFE lastconv runs on the Winograd
 * kernel): w3_host OIHW [4 * LO][Cin][3][3], b3_host [4 * LO].  Host only.  Returns floats written to w3_host or < 0. */
int64_t vfi_test_pack_deconv3x3(const float* weight_host, const float* bias_host, int Cin, int LO, float* w3_host, float* b3_host, int64_t cap);

/* A/B options of tools/ and tests/: each selects between two CORRECT forms of a kernel or launch (csrc/vfi_common.h, enum Option):
 *   stage_quad (bit mask, default 14), fuse_encode (1), fuse0a (1; 2 = the fused kernel in its earlier form, which multiplies all 24 padded input channels: same bits), stage0 (1; 0 = block 0's input gathered from the frame packs per pair instead of assembled from the per-frame staging images), m2n2_px (-1), grouped_variant (-1), splitk (1), splat_atomic (0; 1 = LDS-atomic tile kernel, 3 = staged list gather with compaction for C == 4),
 *   splat_spill_cap (-1), wino_xcd (1), deconv_wino (1), encode_batched (1), wino_quant (1), m2m_fused (1: M2M render as one kernel), m2m_side (0; 1: M2M prepare forks its image-pyramid convolutions onto a side stream — measured neutral / slower under pair lanes), film_side (1: FILM forward on two streams — image 1's feature extraction and the backward flow pyramid beside image 0's / the forward one), xcd_bands (0), wino_dead (1; 0 = the Winograd kernel multiplies all 16 transform planes of a transposed-convolution layer instead of skipping the zero ones: same bits), att_ksplit (0 = the key split of the attention kernel chosen from the CU count; 1..8 = that many key ranges, fewer where one would be empty), wino_probe (0; 1..4 = the cycle-ledger forms of the hot
 *   Winograd instantiation: same results, s_memtime stamps summed per wave of workgroup 0), large_image_bytes (2^31 - 1; the bytes of one
 *   image from which a layer object's launch takes the large-image form of its kernel, csrc/conv_mfma2.hip / conv_wino.hip LARGE: a lower
 *   value puts small images on that path, same bits).
 * The product library reads NO experiment switch from the environment and does not contain this call: the defaults are all it can run.
 * Returns 0, or -2 for an unknown name. */
int vfi_test_set_option(const char* name, int64_t value);
/* The stamp sums of the last launch made under wino_probe != 0 on the current device: [4 waves][8] uint32 = q0, q1, q2, q3 (sums mod
 * 2^32 of the stamps the probe form takes, csrc/conv_wino.hip), stamps per sum, s_memtime at the wave's end, chunks, probe id.
 * Synchronises the device.  tools/wino_ledger.py turns them into the cycle ledger of docs/design/winograd.md. */
int vfi_test_wino_probe_read(uint32_t* out32);
/* Force direct-conv tile variants by trace name: "conv0a_b3=42,resconv_c128=36"; NULL / "" clears (tools/variant_sweep.sh). */
int vfi_test_variant_override(const char* spec);
/* What the calling thread's most recent convolution launch was (any launch made through the direct kernels' or the Winograd kernel's
 * launcher: layer objects, vfi_conv3x3, the networks): up to 8 int32 to `out` —
 *   [0] kernel family: 1 first-generation direct (csrc/conv_mfma.hip), 2 second-generation direct (conv_mfma2.hip), 3 Winograd; 0 = none yet
 *   [1] direct: tile variant id in the common numbering (0.. / 32..); Winograd: region shape 8 (16x8 pixels) / 16 (32x4)
 *   [2] direct: 0 plain, 1 EXT, 2 MASKED, 3 LARGE instantiation; Winograd: the epilogue MODE (0, 1, 10 .. 15)
 *   [3] the store form: out_mode (direct) / SHUF (Winograd; 3 = the LARGE instantiation, an NHWC store as SHUF 0)
 *   [4] split-K slices (1 = unsplit; > 1: the epilogue ran in the reduce kernel)
 *   [5] grid.x   [6] tiles (direct) / work items (Winograd): grid.x < [6] is a persistent launch
 *   [7] launches this thread has made so far.
 * Host only, touches no kernel.  Returns the number of ints written or < 0. */
int vfi_test_last_conv_launch(int32_t* out, int cap);

/* Debug taps for parity tests: copy internal tensors of the LAST interpolate call to host.
 * what: 0 = flow after stage `stage` [B,Hp,Wp,4];  1 = stage input X of `stage`, planar4 [B,Cx/4,Hs,Ws,4];
 *       2 = frame slot pack, planar4 [2,Hp,Wp,4] = (rgb0 | encode features) (stage = slot).
 * Returns number of floats written or <0. */
int64_t vfi_rife_debug_read(vfi_rife_t* net, int what, int stage, float* host_buf, int64_t cap);
int vfi_rife_debug_keep(vfi_rife_t* net, int on);

/* The RIFE stage kernels (csrc/rife_ops.hip), ONE launcher of csrc/rife_ops.h per call, unchanged, on the caller's device buffers:
 * tests/test_gpu_rife_stage.py compares each with a float64 restatement of its own operation.  Layouts as in rife_ops.hip (frame pack
 * planar4 [1 + NF][Hp][Wp][4] at Ppool + slot * pack_stride floats; F [B][Hp][Wp][4]; M [B][Hp][Wp]; X planar4 [B][CX/4][Hs][Ws][4];
 * T planar4 [B][tp][Hs][Ws][4]).  The task table is three host arrays of B <= 32 entries.  Every call validates its arguments
 * (B, Hp and Wp multiples of 64, scales, CX against NF, pack_stride against the pack) and returns -2 without a launch if one is bad;
 * the launches are asynchronous on `stream` except vfi_test_rife_trans1_conv0a, which synchronises it. */
int vfi_test_rife_stage_in(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* F,
                           const float* M, const float* FEAT, float* X, int Hp, int Wp, int s, int CX, int NF, int has_flow, void* stream);
/* Spool: per slot a staging image planar4 [2][Hp/8][Wp/8][4] at Spool + slot * stage_stride floats; X [B][4][Hp/8][Wp/8][4] */
int vfi_test_rife_stage_in0_staged(const float* Spool, int64_t stage_stride, const int* slot0, const int* slot1, const float* t, int B, float* X, int Hp,
                                   int Wp, void* stream);
int vfi_test_rife_flow_up(const float* T, float* F, float* M, int B, int Hp, int Wp, int s, int tp, int has_prev, void* stream);
/* T with 4 planes -> FEAT [B][2][Hp][Wp][4] */
int vfi_test_rife_feat_up(const float* T, float* FEAT, int B, int Hp, int Wp, int s, void* stream);
/* F is updated in place; CX = round_up(12 + 8 NF, 8) */
int vfi_test_rife_stage_trans(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* T, float* F,
                              float* X, int Hp, int Wp, int s_prev, int s_next, int NF, int CX, int has_prev, void* stream);
/* arch 4.26: T with 4 planes, CX = 32 */
int vfi_test_rife_stage_trans_x(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* T, float* F,
                                float* X, int Hp, int Wp, int s_prev, int s_next, int CX, int has_prev, void* stream);
/* The last transition fused into conv0.0 of the last block.  w_oihw_host [32][20][3][3] and bias_host [32] are plain HOST tensors: the
 * call packs them with the routine vfi_rife_create uses for that layer.  Fout must differ from Fin; A0 [B][Hp/2][Wp/2][32]. */
int vfi_test_rife_trans1_conv0a(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* T,
                                const float* Fin, float* Fout, const float* w_oihw_host, const float* bias_host, float* A0, int Hp, int Wp, float slope,
                                void* stream);
/* out [B][H][W][3]; Fdbg (nullable) [B][Hp][Wp][4] receives the final flow inside H x W */
int vfi_test_rife_final_blend(const float* Ppool, int64_t pack_stride, const int* slot0, const int* slot1, const float* t, int B, const float* T,
                              const float* F, float* out, float* Fdbg, int H, int W, int Hp, int Wp, int s, int tp, void* stream);
/* X1 [B][CX/4][Hp][Wp][4] -> X [B][CX/4][u Hp][u Wp][4], plane flow_plane (or none: -1) times u */
int vfi_test_rife_planar4_up(const float* X1, float* X, int B, int Hp, int Wp, int u, int CX, int flow_plane, void* stream);
/* T [B][tp][u Hp][u Wp][4] -> T1 [B][tp][Hp][Wp][4], plane 0 divided by u */
int vfi_test_rife_t_down(const float* T, float* T1, int B, int Hp, int Wp, int u, int tp, void* stream);


/* The call order of FILM's greedy bisection for `inter_frames` new frames (film/__init__.py:17-40) as the C side computes it:
 * (left, right, new) grid positions, 3 ints per call; returns the number of calls or < 0.  Host only. */
int vfi_test_film_schedule(int inter_frames, int* triples, int cap);
/* ... and the float32 grid it is computed on: torch.linspace(0, 1, n) restated (n floats to `out`). */
int vfi_test_linspace01(int n, float* out);

/* FILM: the synthesised flow pyramid of the last vfi_film_forward — direction d (0 forward, 1 backward), pyramid level l,
 * [h_l, w_l, 2] floats to host.  Returns the number of floats or < 0. */
int64_t vfi_film_debug_read_flow(vfi_film_t* net, int d, int level, float* host_buf, int64_t cap);

/* M2M: internal tensors of the last vfi_m2m_prepare to host.  what 0: the PWC flows [2,Hp/4,Wp/4,2] (image 0 forward,
 * 1 backward); 1: d0 [2,Hp,Wp,8] = (refined-flow base 2 | normalised image 3 | warped partner 3); 2: r [2,Hp,Wp,12] = (8 flow
 * residuals | mask logit | pad).  Returns the number of floats or < 0. */
int64_t vfi_m2m_debug_read(vfi_m2m_t* net, int what, float* host_buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_TEST_H */
