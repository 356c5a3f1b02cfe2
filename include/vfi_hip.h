/*
 * vfi_hip.h — C ABI of libvfi_hip.so, the MI355X (gfx950) frame-interpolation hot path.
 *
 * Drop-in boundary: this is what the reference's Python node layer would bind (ctypes) in
 * place of its torch.nn / cupy / taichi calls.  Plain pointers and sizes only — no torch
 * types.  All tensors are fp32.  "dev" pointers are device (HBM) addresses, e.g.
 * torch.Tensor.data_ptr() of a CUDA/HIP tensor; `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Every function returns 0 on success, non-zero on error with
 * a message available from vfi_last_error().  Launches are asynchronous on `stream`.
 *
 * Layout convention: images and activations are NHWC ("channels last"), which is also the
 * layout of ComfyUI's IMAGE type ([N,H,W,C], reference vfi_utils.py:139-143) — the
 * reference's NHWC->NCHW einops views disappear on this path.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference
 * checkout, /root/reference in the build container).
 */
#ifndef VFI_HIP_H
#define VFI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------- */

/* Select the HIP device for the calling thread/process (one process per GPU).
 * Replaces comfy.model_management.get_torch_device() use at vfi_models/rife/__init__.py:121. */
int vfi_init(int device);
const char* vfi_last_error(void);
/* "gfx950" etc. of the active device, plus CU count. */
int vfi_device_info(char* arch_buf, int arch_buf_len, int* n_cus);

/* Per-kernel event tracing (bench.py roofline leg).  When enabled, every kernel launch made
 * by the library is bracketed by hipEventRecord on its stream.  vfi_trace_report() waits for
 * the recorded events and writes one line per kernel name: "<name> <calls> <total_ms>\n". */
int vfi_trace_enable(int on);
int vfi_trace_reset(void);
int vfi_trace_report(char* buf, int buf_len);

/* Shader-clock probe (bench.py `clock`, `roofline.frac_at_clock`).  The chip clocks to its power budget, so a launch duration alone
 * cannot tell a slower kernel from a slower box.  While a buffer is installed, every launch of the dominant (Winograd 3x3) kernel is
 * given one record of 8 x uint64 in it — { t0 = s_memtime at start, r0 = s_memrealtime at start, t1, r1 at end, tag, 0, 0, 0 } of
 * workgroup 0 (persistent: it lives as long as the launch) — until `capacity` records are used.  s_memtime ticks at the shader clock,
 * s_memrealtime at a constant rate (100 MHz; bench.py checks it against the HIP-event duration of the same launches):
 *   sustained MHz of launch i = (t1 - t0) / (r1 - r0) x 100.
 * dev_records: buffer of capacity * 8 uint64 on the CURRENT device, zeroed by the caller; NULL / 0 uninstalls (the names stay
 * readable).  Installing / uninstalling SYNCHRONISES the device first (a probed launch in flight re-reads the installed buffer for its
 * closing stamp), so the buffer may be freed as soon as the uninstalling call has returned.  At most `capacity` launches take a record
 * and a name.  vfi_clock_probe_names writes the trace names of the probed launches, one per line; line `tag` names record `tag`;
 * returns their count (< 0 on error). */
int vfi_clock_probe(void* dev_records, int capacity);
int vfi_clock_probe_names(char* buf, int buf_len);

/* ---- single-op entry points (parity tests, reuse by other nodes) ----------------------- */

/* RIFE backward warp: bilinear, padding_mode="border", align_corners=True, in the reference's
 * fp32 expression order (normalise -> grid_sample un-normalise round trip).
 * Replaces warp() at vfi_models/rife/rife_arch.py:31-70.
 *   in   [N,H,W,C]   flow [N,H,W,2] (x,y displacement in pixels)   out [N,H,W,C] */
int vfi_warp_border(const float* in_dev, const float* flow_dev, float* out_dev,
                    int N, int H, int W, int C, void* stream);

/* Generic NHWC convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 * Replaces torch.nn.Conv2d(k=3,pad=1,stride=1|2) (+ LeakyReLU / ResConv epilogue):
 *   vfi_models/rife/rife_arch.py:73-107 (conv), :20-28 (ResConv).
 *   weight: reference layout [Cout,Cin,3,3] (host pointer, repacked internally per call —
 *           test/utility entry; the model handles pre-pack at vfi_rife_create).
 *   in  [N,H,W,Cin]  out [N,Ho,Wo,Cout]   Ho = (H+2-3)/stride+1
 *   beta (host, [Cout]) may be NULL; if given: y = lrelu(conv*beta + in) (requires Cin==Cout, stride 1)
 *   act: 0 none, 1 LeakyReLU(slope)
 *   variant: -1 = heuristic, >=0 selects a tile configuration (see csrc/conv_mfma.hip); 100 / 101 = the Winograd F(2x2,3x3)
 *            form (stride 1; csrc/conv_wino.hip) with 16x8 / 32x4 output pixels per wave. */
int vfi_conv3x3(const float* in_dev, const float* weight_host, const float* bias_host,
                const float* beta_host, float* out_dev, int N, int H, int W, int Cin, int Cout,
                int stride, int act, float slope, int variant, void* stream);

/* ConvTranspose2d(Cin, Cout, 4, stride 2, pad 1) followed by PixelShuffle(2), output NHWC
 * [N,4H,4W,Cout/4].  Replaces IFBlock.lastconv, vfi_models/rife/rife_arch.py:215-218.
 *   weight: reference layout [Cin,Cout,4,4] (host). */
int vfi_deconv4x4_ps2(const float* in_dev, const float* weight_host, const float* bias_host,
                      float* out_dev, int N, int H, int W, int Cin, int Cout, void* stream);

/* ---- generic NHWC building blocks (FILM path; vfi_models/film/film_arch.py) -------------------------
 * Every tensor pointer addresses the first channel of a channel WINDOW inside a (possibly wider) NHWC tensor
 * whose pixel stride is `*_cs` floats, so the reference's torch.cat along channels is a matter of offsets. */

typedef struct vfi_conv vfi_conv_t;

/* nn.Conv2d(Cin, Cout, k, padding='same') with k in {1,2,3} (k=2 pads bottom/right like torch), weights
 * [Cout,Cin,k,k] in the reference layout (host).  `chan_map[ci]` (nullable) = position of reference input
 * channel ci inside the physical input window of `Cin_phys` channels (multiple of 8; unmapped positions get
 * zero weights — they must hold finite values).  Replaces film_arch.conv(), film_arch.py:784-798. */
vfi_conv_t* vfi_conv_create(const float* w_oihw_host, const float* bias_host, int Cout, int Cin, int kh, int kw,
                            const int* chan_map, int Cin_phys);
void vfi_conv_destroy(vfi_conv_t* conv);
/* out[..., :Cout] = act(conv(in[..., :Cin_phys]) + bias);  act: 0 none, 1 LeakyReLU(slope), 2 clamp to [0,1]
 * (the FILM node's prediction.clamp(0, 1), vfi_models/film/__init__.py:39). */
int vfi_conv_forward(const vfi_conv_t* conv, const float* in_dev, int in_cs, float* out_dev, int out_cs,
                     int N, int H, int W, int act, float slope, void* stream);
/* F.interpolate(x, scale_factor 2, 'nearest') + Conv2d(Cin, Cout, 2, padding 'same') — the first convolution of every FILM Fusion level
 * (film_arch.py:282-292) — as ONE layer that reads the LOW-resolution tensor (round 6): vfi_conv_forward(c, in [N,H,W,*], out [N,2H,2W,out_cs],
 * N, H, W, act 0 | 1, slope).  The four output parities are 4 * Cout channels of a 2x2 convolution whose weights are the original taps summed
 * per input pixel; parity (0,0) keeps 1 tap, (0,1) / (1,0) two, (1,1) four: 9 tap blocks instead of 16 and no up-sampled tensor.  Cout % 64 == 0.
 * Only for an exact x2 (the caller falls back to vfi_upsample_nearest + vfi_conv_forward otherwise). */
vfi_conv_t* vfi_conv_create_up2x2(const float* weight_oihw_host, const float* bias_host, int Cout, int Cin, const int* chan_map, int Cin_phys);

/* F.avg_pool2d(x, 2, 2) (odd sizes floor), film_arch.py:655-674, :112-113.  C % 4 == 0, both strides % 4 == 0 and >= C, both windows
 * 16-byte aligned (float4 accesses), N > 0, H, W >= 2: anything else is refused before the launch. */
int vfi_avgpool2(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, void* stream);
/* F.interpolate(x, size=(Hout,Wout), mode='nearest'), film_arch.py:286.  C % 4 == 0, both strides % 4 == 0 and >= C, both windows
 * 16-byte aligned, N and every size > 0. */
int vfi_upsample_nearest(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int Hin, int Win,
                         int Hout, int Wout, int C, void* stream);
/* F.interpolate(mul * x, size=(Hout,Wout), mode='bilinear') (align_corners=False), film_arch.py:597,610,752.  Any C > 0; strides >= C,
 * N and every size > 0. */
int vfi_resize_bilinear(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int Hin, int Win,
                        int Hout, int Wout, int C, float mul, void* stream);
/* film_arch.warp(image, flow_mul * flow): backward bilinear warp sampling at (x + fx, y + fy), border padding,
 * align_corners=False, reference fp32 expression order; flow = [dx, dy] per pixel.  film_arch.py:677-724.  C % 4 == 0, in_cs and out_cs
 * % 4 == 0, the image and output windows 16-byte aligned, H, W > 1. */
int vfi_warp_film(const float* in_dev, int in_cs, const float* flow_dev, int flow_cs, float flow_mul,
                  float* out_dev, int out_cs, int N, int H, int W, int C, void* stream);
/* out = alpha * a + beta * b over a C-channel window (b may be NULL): flow accumulation v = v_res + v,
 * multiply_pyramid, and channel-window copies.  film_arch.py:600-602,727-742. */
int vfi_axpby(const float* a_dev, int a_cs, const float* b_dev, int b_cs, float* out_dev, int out_cs,
              int64_t pixels, int C, float alpha, float beta, void* stream);

/* ---- FILM as one object ("same triplet for FILM") ------------------------------------------
 * The interpolator of the FILM node, weights resident, workspace owned, the launch sequence of one frame pair issued by
 * one call.  `tensors[i]` = host pointers to the 82 state_dict tensors in film_spec.film_shapes() order (== the state_dict
 * order of film_arch.Interpolator / of the TorchScript artifact film_net_fp32.pt), reference layouts; numels checked.
 * Replaces torch.jit.load(...) + model(frame0, frame1, dt) of vfi_models/film/__init__.py:73-76,30-39 and
 * Interpolator.debug_forward, film_arch.py:401-455 (the model ignores dt: always the midpoint, :427-429). */
typedef struct vfi_film vfi_film_t;
vfi_film_t* vfi_film_create(const float* const* tensors, const int64_t* numels, int n_tensors);
void vfi_film_destroy(vfi_film_t* net);
/* out_dev [H,W,3] = Interpolator(x0, x1) for x0_dev, x1_dev [H,W,C] fp32 (C >= 3, alpha ignored); clamp != 0 applies the
 * node's prediction.clamp(0, 1) (film/__init__.py:39).  H, W >= 64, H * W <= vfi_film_max_pixels().  The workspace (15 GB at 1080p) is sized on first use.
 * All work is ordered on `stream` as seen by the caller; inside, half of the network up to the fusion runs on a side stream of the
 * object's own (forked from and joined to `stream` by events within the call: round 6, docs/design/film.md). */
int vfi_film_forward(vfi_film_t* net, const float* x0_dev, const float* x1_dev, int C, int H, int W, float* out_dev, int clamp,
                     void* stream);
int vfi_film_release_workspace(vfi_film_t* net);
/* The largest frame vfi_film_forward takes, in pixels H * W: vfi_conv_huge_max_floats() / 208 = 10 324 440, where 208 = 144 + 64 floats per
 * pixel is the object's widest tensor, the aligned pyramid's level 0 with the fusion's slot (2160x3840 and 2160x4096 fit; 2176x4800 does
 * not).  A larger frame is refused before any allocation or launch.  The object's layers carry vfi_conv_allow_huge: at 2160x3840 three of
 * them read an operand of more than 4 GiB (docs/design/film.md).  Frames of up to 5 162 220 pixels, the limit before the large layer forms
 * existed, run the launches they always ran. */
int64_t vfi_film_max_pixels(void);
/* Device bytes of the object's workspace as it stands (0 before the first forward and after a release; it grows during the first forward of
 * a frame size, whose scratch tensors are allocated at first use).  For tools and documentation: 69 GB at 2160x3840. */
int64_t vfi_film_workspace_bytes(vfi_film_t* net);
/* on != 0 (the default): vfi_film_forward forks half of the network onto the object's side stream; 0: everything on the caller's stream —
 * what a host that already keeps several pairs in flight on streams of its own (the nodes' pair lanes) wants: four busy streams on the
 * runtime's four hardware queues left the lanes 2 % slower than two.  Frames are bit-identical either way.  Returns the previous setting. */
int vfi_film_two_streams(vfi_film_t* net, int on);

/* The whole FILM node call for a HOST clip, replacing FILM_VFI.vfi's body, vfi_models/film/__init__.py:63-113:
 * frames_host [N,H,W,C] fp32 (C >= 3; alpha dropped) -> out_host [*n_out,H,W,3].  Per kept pair: frame_i, then the m-1 new frames
 * of the greedy bisection (:12-42; every model call returns the midpoint of two known frames, clamped to [0,1], and later calls
 * consume earlier outputs); a skipped pair is DROPPED, frame included (:89-90); the clip's last frame is appended.
 * multipliers == NULL: `multiplier` for every pair; else the list (n_multipliers entries) padded with 2 (:84-87).  skip: [N-1]
 * flags or NULL.  out_host == NULL only computes *n_out.  Synchronous, own stream. */
int vfi_film_run(vfi_film_t* net, const float* frames_host, int N, int H, int W, int C, int multiplier, const int* multipliers,
                 int n_multipliers, const uint8_t* skip, float* out_host, int64_t* n_out);

/* ---- M2M custom ops ---------------------------------------------------------------------- */

/* Summation splat (forward warp): out[n, y', x', c] += in[n,y,x,c] * bilinear weight at the 4 integer
 * neighbours of (x + flow_x, y + flow_y); out-of-image targets dropped, non-finite targets skipped.
 * `out` is zeroed by the call.  Replaces softsplat_func.forward / the softsplat_out CUDA kernel,
 * vfi_models/ops/cupy_ops/softsplat.py:140-233.   in/out [N,H,W,C], flow [N,H,W,2] (NHWC). */
int vfi_softsplat_sum(const float* in_dev, const float* flow_dev, float* out_dev, int N, int H, int W, int C,
                      void* stream);

/* 9x9 mean-L1 cost volume: out[n,y,x, out_coff + 9*(dy+4)+(dx+4)] = mean_c |one[n,y,x,c] - two[n,y+dy,x+dx,c]|,
 * out-of-image (y+dy,x+dx) -> mean_c |one|.  Replaces costvol_func.forward / costvol_out,
 * vfi_models/ops/cupy_ops/costvol.py:4-43,135-183.   one/two [N,H,W,C] (C % 4 == 0); out [N,H,W,out_cs]:
 * the 81 channels are written at channel offset out_coff of a wider NHWC tensor (the reference's
 * torch.cat of the volume with features, vfi_models/m2m/M2M_arch.py:484-490, then costs nothing). */
int vfi_costvol9x9(const float* one_dev, int one_cs, const float* two_dev, int two_cs, int two_swap, float* out_dev,
                   int N, int H, int W, int C, int out_cs, int out_coff, void* stream);
/* one/two are channel windows (pixel strides one_cs/two_cs); two_swap != 0 reads `two` from the partner image
 * n^1 of a batch of direction pairs (the reference runs the decoder on (a,b) and on (b,a), M2M_arch.py:521-546). */

/* ---- the reference's remaining custom ops, NCHW (the drop-in ops backend cfi_amd.ops) ------------------- */
/* Every `*_strides` argument is a host array of 4 element strides (n, c, y, x) of that NCHW operand, so channel slices are
 * read in place.  fp32 only; nothing is allocated and nothing synchronises. */

/* Separable adaptive convolution: out[n,c,y,x] = sum_fy sum_fx in[n,c,y+fy,x+fx] * ver[n,fy,y,x] * hor[n,fx,y,x], K taps
 * each way; `in` is pre-padded (Hin >= Ho + K - 1, Win >= Wo + K - 1).  Replaces sepconv_func.forward / sepconv_out,
 * vfi_models/ops/cupy_ops/sepconv.py:86-117,155-199 (plain fp32 sums of row sums instead of the Kahan-compensated sum). */
int vfi_sepconv(const float* in_dev, const long long* in_strides, const float* ver_dev, const long long* ver_strides,
                const float* hor_dev, const long long* hor_strides, float* out_dev, const long long* out_strides, int N, int C,
                int Hin, int Win, int Ho, int Wo, int K, void* stream);

/* AdaCoF forward: out[n,c,i,j] = sum_{k,l < F} weight[n,kF+l,i,j] * bilinear(input[n,c], i + k*dilation + alpha,
 * j + l*dilation + beta) with alpha/beta = offset_i/offset_j[n,kF+l,i,j], corners clamped to the image, the integer part
 * (int)alpha truncated toward zero.  Contiguous NCHW operands; Ho/Wo must satisfy the reference's asserts.  Replaces
 * FunctionAdaCoF.forward / kernel_AdaCoF_updateOutput, vfi_models/ops/cupy_ops/adacof.py:5-65,259-333. */
int vfi_adacof(const float* input_dev, const float* weight_dev, const float* offset_i_dev, const float* offset_j_dev,
               float* out_dev, int N, int C, int H, int W, int F, int dilation, int Ho, int Wo, void* stream);

/* PWC correlation: out[n, 9*(dy+4)+(dx+4), y, x] = (1/C) sum_c a[n,c,y,x] * b[n,c,y+dy,x+dx], |dy|,|dx| <= 4, b outside the
 * image = 0; out is a contiguous [N,81,H,W] tensor.  Replaces _FunctionCorrelation.forward / kernel_Correlation_rearrange +
 * kernel_Correlation_updateOutput, vfi_models/ops/cupy_ops/correlation.py:4-102,232-296 (one kernel, no padded copies). */
int vfi_correlation81(const float* a_dev, const long long* a_strides, const float* b_dev, const long long* b_strides,
                      float* out_dev, int N, int C, int H, int W, void* stream);

/* Distance transform of contiguous [N,H,W] data: tmp = min(diam2, min_j data[row][j] + (x-j)^2) along rows, then
 * out = sqrt(min(diam2, min_i tmp[i][col] + (y-i)^2)) along columns.  H, W <= 16384; tmp must not alias data or out.
 * Replaces the two kernel_dt launches + the final sqrt of batch_edt, vfi_models/ops/cupy_ops/batch_edt.py:10-100. */
int vfi_edt(const float* data_dev, float* tmp_dev, float* out_dev, int N, int H, int W, float diam2, void* stream);

/* ---- M2M network building blocks (vfi_models/m2m/M2M_arch.py) -------------------------------- */

/* Generalised layer object: kind 0 = nn.Conv2d(Cin, Cout, k, stride, padding) with (k,stride) in
 * {(3,1),(3,2),(2,2),(1,1)}: k=3 pads 1 — pad_mode 0 zeros (M2M_arch.py:589-602), 1 replicate (the "conv(3,replpad)"
 * of Basic, :228-260), 2 reflect (ReflectionPad2d(1) + Conv2d, CAIN's ConvNorm, cain/common.py:26-45; inputs >= 2x2); k=2/s=2 pads 0 ("sconv(2)" after evenize, :205-226 — sizes must be even).
 * kind 1 = nn.ConvTranspose2d(Cin, Cout, 4, 2, 1) (deconv(), :605-618), weights [Cin,Cout,4,4].
 * prelu_host (nullable): Cout per-channel PReLU slopes, applied by act 3. */
vfi_conv_t* vfi_conv_create_ex(int kind, const float* w_host, const float* bias_host, int Cout, int Cin, int k, int stride,
                               int pad_mode, const int* chan_map, int Cin_phys, const float* prelu_host);
/* out = post_scale * act(layer(in) + bias + res) + post_shift.  act: 0 none, 1 LeakyReLU / single-parameter PReLU
 * (slope), 2 clamp01, 3 per-channel PReLU, 4 sigmoid, 5 GELU (erf form, nn.GELU()).  post_scale == 0 disables the affine.  res (nullable):
 * [N,Hout,Wout,res_cs] added before the activation (the decoder's `flow + netMain(...)`, :503).
 * Output is [N, ceil(Hin/stride), ceil(Win/stride), out_cs] (kind 0; stride-2 layers need even sizes unless vfi_conv_accept_odd) or [N, 2*Hin, 2*Win, out_cs] (kind 1). */
/* Let a 3x3 stride-2 layer (kind 0) take odd input sizes, as nn.Conv2d(k=3, s=2, p=1) does: output ceil(Hin/2) x ceil(Win/2), the
 * missing row / column read as padding.  Off by default (such a layer rejects odd sizes); even sizes compute the same bits either way.
 * Fails for any other layer. */
int vfi_conv_accept_odd(vfi_conv_t* conv, int on);
/* Operand images (input, output, residual of ONE image) and the kernels' index arithmetic.  Every layer object serves images below 2 GiB.
 * The plain forms — kind 0, zero padding, act 0 / 1 / 2, no post affine; 3x3 stride 1 / 2, 2x2, 1x1 and the 4x4 stride-2 polyphase form —
 * also serve 2 GiB up to 4 GiB - 1 through kernel forms that rebase their buffer descriptors per tile / per region.  From 4 GiB on a call
 * is refused ("image larger than 2 GiB") unless the object was given this permission: then the same forms serve operand images of up to
 * vfi_conv_huge_max_floats() = 2^31 - 1 floats (8 GiB - 4 bytes) each, the bound of the audited arithmetic (an image's float count is kept
 * in an int; every address is a 64-bit per-tile base plus an offset of a few rows).  Off by default, a property of the object; no launch
 * that was legal without it changes its kernel, its geometry or a bit of its output.  Of the extended feature set one layer form is served
 * in the same way and to the same bounds: per-channel PReLU (act 3) with zero padding, no residual and no post affine, by the Winograd kernel
 * (3x3 stride 1) and the direct kernel (3x3 stride 1 / 2, 1x1) — ATM's full-resolution layers, operands of 2.67 to 4.28 GB at 2160 x 3840.
 * The other extended forms (replicate / reflect padding, sigmoid, GELU, post affine, transposed convolutions, residual + PReLU) keep their
 * 2 GiB refusal. */
int vfi_conv_allow_huge(vfi_conv_t* conv, int on);
int64_t vfi_conv_huge_max_floats(void);
/* One more layer form may be served above 2 GiB, and only by an object that was given this permission: Conv2d 3x3 stride 1 + residual +
 * per-channel PReLU (act 3, zero padding, no post affine) — the last layer of AMT-G's ResBlock, prelu(conv5(x3) + r0), whose input is 2.92 GB
 * at 2160 x 3840.  With it the Winograd kernel (both region shapes) and the direct kernel's 3x3 stride-1 tiles take their large-image forms
 * under the conditions that hold for act 3 without a residual (operand images below 4 GiB, or vfi_conv_allow_huge's bound with that
 * permission too); input, output and residual are each addressed from a per-region / per-tile 64-bit base.  Same arithmetic and summation
 * order as the plain form: the same bits wherever both are legal.  Off by default, a property of the object: without it every call decides,
 * launches and refuses ("image larger than 2 GiB") exactly as before. */
int vfi_conv_allow_large_res_prelu(vfi_conv_t* conv, int on);
int vfi_conv_forward_ex(const vfi_conv_t* conv, const float* in_dev, int in_cs, int Hin, int Win, float* out_dev, int out_cs,
                        int N, int act, float slope, float post_scale, float post_shift, const float* res_dev, int res_cs,
                        void* stream);

/* Replicate-pad both frames to Hp x Wp (M2M_arch.py:903-913), joint mean/std over the padded pair (:915-931),
 * and write (frame_n - mean) / (std + 1e-7) to out[n, y, x, out_coff + 0..2] (n = 0,1; out [2,Hp,Wp,out_cs]).
 * stats_dev[0] = mean, stats_dev[1] = std + 1e-7.  frames: [H,W,C] fp32, C >= 3.  workspace: >= 16 KiB device. */
int vfi_m2m_normalize(const float* frame0_dev, const float* frame1_dev, int C, int H, int W, int Hp, int Wp, float* out_dev,
                      int out_cs, int out_coff, float* stats_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);
/* backwarp(): grid_sample(in, grid + flow*2/(size-1), bilinear, zeros, align_corners=True), M2M_arch.py:24-92.
 * in_swap != 0 samples the partner image n^1.  flow = [dx, dy] per pixel. */
int vfi_warp_m2m(const float* in_dev, int in_cs, int in_swap, const float* flow_dev, int flow_cs, float* out_dev, int out_cs,
                 int N, int H, int W, int C, void* stream);
/* adaptive_avg_pool2d to 1x1 (mode 0 -> out [N,1,C]), Hx1 (mode 1 -> [N,H,C]) or 1xW (mode 2 -> [N,W,C]), :689-703 */
int vfi_pool_mean(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, int mode, void* stream);
/* out = s3 * mean_k(cC[n,k*C+c] * cH[n,y,k] * cW[n,x,k]), k < 16 — the EncDec "cube" attention, :786-795 */
int vfi_m2m_cube_apply(const float* s3_dev, int s3_cs, const float* cC_dev, const float* cH_dev, int cH_cs, const float* cW_dev,
                       int cW_cs, float* out_dev, int out_cs, int N, int H, int W, int C, void* stream);
/* Timestep-independent splat preparation for the 8 splats s = 2*branch + direction of one pair (:945-1010, :559-561):
 * tf_dev [8,H,W,2] = flow + residual, e_dev [8,H,W] = exp(clip(alpha * photometric, -20, 20)).
 * d0 [2,H,W,d0_cs] = (flow 0..1 | normalised image 2..4 | ..), r [2,H,W,r_cs] = (8 residuals | mask logit). */
int vfi_m2m_photo(const float* d0_dev, int d0_cs, const float* r_dev, int r_cs, float alpha, float* tf_dev, float* e_dev, int H,
                  int W, void* stream);
/* img4_dev [2,H,W,4] = (d0's channels 2..4 = the normalised image, 1): the compact plane the kernels below read with one 16-byte load
 * per tap / source (round 6, csrc/m2m_render.hip). */
int vfi_m2m_image4(const float* d0_dev, int d0_cs, float* img4_dev, int H, int W, void* stream);
/* = vfi_warp_m2m(image, in_swap = 1, C = 3) with the partner image taken from img4 (bit-identical): out[n,y,x,0..2] =
 * backwarp(img4[n ^ 1], flow[n]) (M2M_arch.py:24-92, :866-890). */
int vfi_m2m_warp_image4(const float* img4_dev, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int H, int W, void* stream);
/* vfi_m2m_photo's results computed per 32x32 tile, plus what the one-kernel render below needs: img4_dev from vfi_m2m_image4
 * (input); tile_ranges_dev [8][ceil(H/32)*ceil(W/32)][4] =
 * (fx_min, fx_max, fy_min, fy_max) of every refined flow field tf_s over the tile's finite values (min > max: none);
 * smax_dev [8] = max |tf_s|.  tf_dev / e_dev as vfi_m2m_photo (bit-identical). */
int vfi_m2m_photo_tiles(const float* d0_dev, int d0_cs, const float* r_dev, int r_cs, float alpha, const float* img4_dev, float* tf_dev,
                        float* e_dev, float* tile_ranges_dev, float* smax_dev, int H, int W, void* stream);
/* forwarp_mframe_mask for one timestep 0 <= t <= 1 as ONE kernel (M2M_arch.py:551-581, :1012-1037 with softsplat_out of
 * cupy_ops/softsplat.py:140-192 inside): = vfi_m2m_splat_inputs + vfi_softsplat_sum (8 splats) + vfi_m2m_combine, bit-identical to
 * that sequence wherever a tile's source window fits one LDS stage (1824 sources), same sums in another strip order beyond; no limit
 * on the displacement, no fallback launches.  Inputs from vfi_m2m_photo_tiles (Hp x Wp = the padded size), stats from
 * vfi_m2m_normalize; out_dev [H,W,3]. */
int vfi_m2m_render_fused(const float* img4_dev, const float* tf_dev, const float* e_dev, const float* tile_ranges_dev, const float* smax_dev,
                         const float* stats_dev, float t, float* out_dev, int Hp, int Wp, int H, int W, void* stream);
/* Per timestep t: in_dev [8,H,W,4] = (image*td*e, td*e), flow_dev [8,H,W,2] = tf * tm (:1012-1024, :563-567) */
int vfi_m2m_splat_inputs(const float* d0_dev, int d0_cs, const float* tf_dev, const float* e_dev, float t, float* in_dev,
                         float* flow_dev, int H, int W, void* stream);
/* splat_dev [8,Hp,Wp,4] (vfi_softsplat_sum of the above) -> out [H,W,3]: normalise by the splatted weights, fill holes
 * with the t-blend, undo the input normalisation, crop (:569-581, :1026-1037) */
int vfi_m2m_combine(const float* splat_dev, const float* d0_dev, int d0_cs, const float* stats_dev, float t, float* out_dev,
                    int Hp, int Wp, int H, int W, void* stream);

/* ---- M2M as one object ("same triplet for M2M") ---------------------------------------------
 * `tensors[i]` = host pointers to the 188 state_dict tensors of M2M_PWC in m2m_spec.m2m_shapes() order (== torch state_dict
 * order), reference layouts; numels checked.  Replaces M2M_PWC() + load_state_dict (vfi_models/m2m/__init__.py:43-46) and
 * M2M_PWC.forward (M2M_arch.py:894-1037), split where the reference's timestep loop starts (:948):
 *   vfi_m2m_prepare — padding, normalisation, flow network, motion refinement, photometric metric: once per frame pair;
 *   vfi_m2m_render  — the 8 splats + blend of ONE timestep t -> out_dev [H,W,3] (not clamped, like the reference). */
typedef struct vfi_m2m vfi_m2m_t;
vfi_m2m_t* vfi_m2m_create(const float* const* tensors, const int64_t* numels, int n_tensors);
void vfi_m2m_destroy(vfi_m2m_t* net);
int vfi_m2m_prepare(vfi_m2m_t* net, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, void* stream);
int vfi_m2m_render(vfi_m2m_t* net, float t, float* out_dev, void* stream);
int vfi_m2m_release_workspace(vfi_m2m_t* net);
/* device bytes of the object's workspace at the moment — the activation tensors and a few KB of control words (0 after
 * vfi_m2m_release_workspace): what a host that keeps the object between clips weighs against re-allocating per clip (the nodes:
 * ckpt.end_call) */
int64_t vfi_m2m_workspace_bytes(vfi_m2m_t* net);

/* The whole M2M node call for a HOST clip, replacing M2M_VFI.vfi + generic_frame_loop in timestep mode
 * (vfi_models/m2m/__init__.py:33-60, vfi_utils.py:149-389): frames_host [N,H,W,C] fp32, N >= 2 -> out_host [*n_out,H,W,3].
 * multipliers == NULL ("int multiplier"): frame_i, its multiplier-1 new frames at t = k/m (none when skip[i]), ..., last frame.
 * multipliers != NULL ("list multiplier", n_multipliers entries padded with 2): every pair runs as its own 2-frame loop — m == 0
 * drops the pair INCLUDING its first frame (and the clip's last frame when it is the last pair), m == 1 keeps the frame, and the
 * skip list is consulted with the pair's LOCAL index, i.e. skip[0], for every pair (vfi_utils.py:364-386): reproduced as is.
 * New frames are not clamped (like the reference).  out_host == NULL only computes *n_out.  Synchronous, own stream. */
int vfi_m2m_run(vfi_m2m_t* net, const float* frames_host, int N, int H, int W, int C, int multiplier, const int* multipliers,
                int n_multipliers, const uint8_t* skip, float* out_host, int64_t* n_out);

/* ---- RIFE arch 4.0 building blocks (sudo_rife4 checkpoint; rife40.py drives them with the layer objects above) -- */

/* Block-0 input of one task: out [Hp,Wp,8] = (clamp(frame0.rgb), clamp(frame1.rgb), timestep, 0), images zero in the
 * padding, timestep everywhere (torch.clamp + F.pad + timestep.repeat, rife_arch.py:476-499).  frames [H,W,C>=3]. */
int vfi_rife40_prep(const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float timestep, float* out_dev,
                    int Hp, int Wp, void* stream);
/* warp() (rife_arch.py:31-70: bilinear, border, align_corners=True, reference expression order) over NHWC channel
 * windows; flow = [dx, dy] at flow_dev[pixel * flow_cs]. */
int vfi_warp_rife(const float* in_dev, int in_cs, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int N,
                  int H, int W, int C, void* stream);
/* *out_dev = max |x| over a C-channel window of `pixels` pixels — the `f0[:, :2].abs().max() > 32` test that doubles
 * the block scales (rife_arch.py:598-607). */
int vfi_absmax(const float* x_dev, int cs, int C, int64_t pixels, float* out_dev, void* stream);
/* merged = w0 * sigmoid(mask) + w1 * (1 - sigmoid(mask)); with res (the Unet output): clamp(merged + (res*2 - 1), 0, 1);
 * crop to H x W and the node's clamp(0,1) (rife_arch.py:712-732, rife/__init__.py:207).  w01 [B,Hp,Wp,>=6] = (w0 | w1). */
int vfi_rife40_output(const float* w01_dev, int w_cs, const float* mask_dev, int m_cs, const float* res_dev, int r_cs,
                      float* out_dev, int B, int Hp, int Wp, int H, int W, void* stream);

/* ---- IFRNet building blocks (IFRNet_L / IFRNet_S checkpoints; ifrnet.py drives them with the layer objects above) -- */

/* img{0,1} [Hp,Wp,4] = (frame{0,1}.rgb, 0), zero in the padding: F.pad of both frames, no clamp
 * (vfi_models/ifrnet/IFRNet_L_arch.py:230-235).  frames [H,W,C>=3]. */
int vfi_ifrnet_prep(const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float* img0_dev, float* img1_dev,
                    int Hp, int Wp, void* stream);
/* mean_[n] = mean over both padded images of pair n (IFRNet_L_arch.py:242-247), from the per-image channel means
 * chan_means [2N,4] (vfi_pool_mean mode 0 over img [2N,Hp,Wp,4]; images 0..N-1 = img0, N..2N-1 = img1);
 * writes mean_out[n] and subtracts it from the colour channels of both images in place (:248-249). */
int vfi_ifrnet_center(float* img_dev, const float* chan_means_dev, float* mean_out_dev, int N, int64_t pixels, void* stream);
/* convrelu(3, 64, 7, 2, 3): Conv2d 7x7 stride 2 pad 3 + PReLU(64), the head of IFRNet_L's encoder (:128-130).
 * w_dev [7][7][3][Cout] (device), out [N,(Hin-1)/2+1,(Win-1)/2+1,out_cs].  Cout is 64, or 84 (AMT-G's pyramid stem); out_cs % 4 == 0. */
int vfi_conv7x7s2_prelu(const float* in_dev, int in_cs, const float* w_dev, const float* bias_dev, const float* slope_dev, int Cout,
                        float* out_dev, int out_cs, int N, int Hin, int Win, void* stream);
/* torch.sigmoid in place over a C-channel window (:278) */
int vfi_sigmoid(float* x_dev, int cs, int C, int64_t pixels, void* stream);
/* out[n, p, 0..C) = values_host[n] for N <= 64 items of pixels_per_item pixels: embt.repeat(1, 1, h, w) (:160-163) */
int vfi_fill_items(float* out_dev, int cs, int C, int N, int64_t pixels_per_item, const float* values_host, void* stream);
/* F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False) * post_mul with the source step the CALLER
 * derived from s (torch uses (float)(1/s), not Hin/Hout, when a scale_factor is given) and the output size floor(in*s)
 * (:38-41,250-251,281-288). */
int vfi_resize_bilinear_ratio(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int Hin, int Win, int Hout, int Wout,
                              int C, float ratio_h, float ratio_w, float post_mul, void* stream);
/* imgt = clamp(mask * warp(img0, flow0) + (1 - mask) * warp(img1, flow1) + mean_ + res, 0, 1)[:H, :W] (:290-294).
 * fin [N,Hf,Wf,8] = (flow0 xy, flow1 xy, mask, res rgb) at the size of the reference's last resize (the warp grid has
 * that size, the images Hp x Wp); img{0,1} [N,Hp,Wp,4] mean-removed; out [N,H,W,3].  0 < H <= min(Hp, Hf), 0 < W <= min(Wp, Wf). */
int vfi_ifrnet_output(const float* img0_dev, const float* img1_dev, const float* fin_dev, const float* mean_dev, float* out_dev, int N,
                      int Hp, int Wp, int Hf, int Wf, int H, int W, void* stream);

/* ---- GMFSS Fortuna (union) building blocks (vfi_models/gmfss_fortuna/GMFSS_Fortuna_union_arch.py; gmfss.py drives them
 * together with the layer objects above).  First-correct versions: one thread per output element. ------------------------ */

/* F.pad of an RGB frame into channels 0..2 of an NHWC tensor, zeros in the padding (gmfss_fortuna/__init__.py:43-48) */
int vfi_pad_rgb(const float* frame_dev, int C, int H, int W, float* out_dev, int out_cs, int Hp, int Wp, void* stream);
/* (x - mean[c]) / std[c], C <= 8: normalize_img (:1123-1131) */
int vfi_normalize_channels(const float* in_dev, int in_cs, float* out_dev, int out_cs, int C, int64_t pixels, const float* mean_host,
                           const float* std_host, void* stream);
/* nn.PReLU() (one shared slope) over a channel window: the pre-activations of MetricNet / FeatureNet / GridNet (:1420-1561) */
int vfi_prelu_scalar(const float* in_dev, int in_cs, float* out_dev, int out_cs, int C, int64_t pixels, float slope, void* stream);
/* nn.InstanceNorm2d (no affine, eps 1e-5): stats [N][C][2] = (mean, 1/sqrt(var+eps)); workspace >= N*64*C*2 doubles
 * (:165-215); a larger one is used for more, shorter strips of the first pass (up to 1024: more workgroups in flight) */
int vfi_instnorm_stats(const float* x_dev, int cs, int C, int N, int64_t HW, float* stats_dev, double* workspace_dev,
                       int64_t workspace_bytes, void* stream);
/* out = act2(act1((x - mean) * rstd) + add): norm(+relu) and the residual sum + relu of ResidualBlock_class (:207-215) */
int vfi_instnorm_apply(const float* x_dev, int cs, const float* stats_dev, int C, int N, int64_t HW, int relu1, const float* add_dev,
                       int add_cs, int relu2, float* out_dev, int out_cs, void* stream);
/* nn.LayerNorm(C) over the channel axis (eps 1e-5), TransformerLayer.norm1 / norm2 (:479-523) */
int vfi_layernorm(const float* x_dev, int cs, int C, int64_t tokens, const float* gamma_dev, const float* beta_dev, float* out_dev,
                  int out_cs, void* stream);
/* out = add + LayerNorm(x) (`source + message`, TransformerLayer.forward :517-523), out2 (nullable) = a second copy of the result in
 * another channel window (the FFN's concat slot).  out may be add itself (in place); neither output may alias x. */
int vfi_layernorm_add(const float* x_dev, int cs, int C, int64_t tokens, const float* gamma_dev, const float* beta_dev, const float* add_dev,
                      int add_cs, float* out_dev, int out_cs, float* out2_dev, int out2_cs, void* stream);
/* nn.GELU() (erf form) in place over a channel window (:467-471) */
int vfi_gelu(float* x_dev, int cs, int C, int64_t pixels, void* stream);
/* torch.roll by (-shift_h, -shift_w) + split_feature into splits x splits windows: [B,h,w,C] -> [B*K*K, (h/K)*(w/K), C];
 * inverse != 0: merge_splits + roll back (:367-436,1059-1120) */
int vfi_window_partition(const float* in_dev, int in_cs, float* out_dev, int out_cs, int B, int h, int w, int C, int splits, int shift_h,
                         int shift_w, int inverse, void* stream);
/* out[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k]: q k^T / sqrt(c) of the attention and matching steps (:319,417,810) */
int vfi_bmm_nt(const float* a_dev, int a_cs, const float* b_dev, int b_cs, float* out_dev, int nb, int M, int N, int K, float alpha,
               void* stream);
/* out[b][m][c] = sum_n P[b][m][n] * V[b][n][c]: attn v, prob grid, prob flow (:321,425,833,741) */
int vfi_bmm_nn(const float* p_dev, const float* v_dev, int v_cs, float* out_dev, int out_cs, int nb, int M, int N, int C, void* stream);
/* softmax over the rows of x [nb][rows][cols] in place; mask [period][rows][cols] (nullable) is added first, batch b taking
 * mask[b % period] (scores += attn_mask.repeat(b, 1, 1), :422-425) */
int vfi_softmax_rows(float* x_dev, int nb, int rows, int cols, const float* mask_dev, int mask_period, void* stream);
/* The three calls above as ONE flash-style kernel on the fp32 matrix cores, the score matrix never touching HBM:
 *   out[b][m][0:DV] = sum_n softmax_n(alpha * q[b][m] . k[b][n] + mask) * v[b][n][0:DV],   q, k: [nb][L][C = 128]
 * mask = -100 where labels[b % period][m] != labels[b % period][n] (labels nullable, int32 [period][Lk]: the shifted-window
 * attention mask of generate_shift_window_attn_mask, :326-364, as region labels).  DV = 128 (attention) or 1..32 (global
 * matching / flow propagation: v = pixel grid / flow).  Replaces single_head_split_window_attention (:367-436),
 * global_correlation_softmax (:806-843), FeatureFlowAttention.forward's global branch (:708-745). */
int vfi_attention(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, float* out_dev,
                  int out_cs, int nb, int Lq, int Lk, int C, int DV, float alpha, const int* labels_dev, int label_period,
                  void* stream);
/* single_head_split_window_attention (:367-436) on [B,h,w,.] token MAPS, with the roll + split into splits x splits windows
 * (split_feature / merge_splits, :1059-1120) and the roll back folded into the kernel's addressing — no partitioned copies
 * of q / k / v / out in HBM.  shift = (0,0) or (wh/2, ww/2) with labels_dev = int32 [splits^2][wh*ww] region labels (nullable).
 * out must not alias q / k / v. */
int vfi_window_attention(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, float* out_dev,
                         int out_cs, int B, int h, int w, int splits, int shift_h, int shift_w, int C, float alpha,
                         const int* labels_dev, void* stream);
/* flow_warp / bilinear_sample: grid_sample(zeros, align_corners=True) at pixel + flow (:955-991) */
int vfi_flow_sample(const float* in_dev, int in_cs, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int N, int H, int W,
                    int C, void* stream);
/* F.interpolate(x, size=(Hout,Wout), mode="bilinear", align_corners=True) * post_mul: the x2 flow up-sampling between GMFlow's
 * scales (:1302-1307) */
int vfi_resize_bilinear_ac(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int Hin, int Win, int Hout, int Wout,
                           int C, float post_mul, void* stream);
/* flow[:, 0:2] += local_correlation_softmax(f0, f1, radius) (:846-913,1335) */
int vfi_local_match(const float* f0_dev, int f0_cs, const float* f1_dev, int f1_cs, float* flow_dev, int flow_cs, int N, int H, int W,
                    int C, int radius, void* stream);
/* FeatureFlowAttention.forward_local_window_attn: q / k already projected, (2r+1)^2 window, zero padding (:745-803) */
int vfi_local_propagate(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* flow_dev, int flow_cs, float* out_dev,
                        int out_cs, int N, int H, int W, int C, int radius, void* stream);
/* convex up-sampling of the flow by `factor` from the up-sampler's 9*factor^2 mask logits (:1237-1258) */
int vfi_convex_upsample(const float* mask_dev, int mask_cs, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int N, int H,
                        int W, int factor, void* stream);
/* MetricNet's 14 input channels: images, -l1 photometric errors after backwarp, normalised flows, fwd/bwd occlusion (:1375-1454) */
int vfi_gmfss_metric_inputs(const float* img0_dev, const float* img1_dev, int img_cs, const float* flow01_dev, const float* flow10_dev,
                            int flow_cs, float* out_dev, int out_cs, int H, int W, void* stream);
/* tanh(x) * scale in place over a channel window (:1465) */
int vfi_tanh_scale(float* x_dev, int cs, int C, int64_t pixels, float scale, void* stream);
/* softsplat(x, flow, metric, "soft"), the part before the summation splat: out [px, C+1] = (x * exp(zs*z), exp(zs*z)),
 * flow_out [px, 2] = fs * flow (vfi_models/ops/cupy_ops/softsplat.py:408-409) */
int vfi_splat_prep(const float* x_dev, int x_cs, const float* z_dev, int z_cs, const float* flow_dev, int flow_cs, float* out_dev,
                   float* flow_out_dev, int C, int64_t pixels, float z_scale, float flow_scale, void* stream);
/* ... and after it: out[p, 0:C] = splat[p, 0:C] / (splat[p, C] + 1e-7) (softsplat.py:415-432) */
int vfi_splat_normalize(const float* splat_dev, float* out_dev, int out_cs, int C, int64_t pixels, void* stream);
/* nn.PixelShuffle(2) on NHWC: in [N,H,W,4C] -> out [N,2H,2W,C] (IFBlock.lastconv rife_arch.py:215-218, GridNet tail :1564-1579) */
int vfi_pixel_shuffle2(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, void* stream);
/* torch.clamp(x, 0, 1)[:, :, :H, :W] into a dense [H,W,C] frame (:1857, gmfss_fortuna/__init__.py:78) */
int vfi_clamp_crop(const float* in_dev, int in_cs, int Hp, int Wp, float* out_dev, int H, int W, int C, void* stream);

/* ---- IFUNet building blocks (vfi_models/ifunet/IFUNet_arch.py; ifunet.py drives them with the layer objects above).
 * Bodies checked on the host (tests/hostcheck) and on the MI355X against the oracle (tests/test_gpu_ifunet.py). --------------- */

/* CBAM ChannelGate pooling (:411-436): stats [N][C][2] = (mean, max) over H*W; workspace >= N*64*C*12 bytes
 * (a larger one is used for more, shorter strips of the first pass, up to 128) */
int vfi_channel_pool(const float* x_dev, int cs, int C, int N, int64_t HW, float* stats_dev, void* workspace_dev, int64_t workspace_bytes,
                     void* stream);
/* scale [N][C] = sigmoid(mlp(mean) + mlp(max)), mlp = Linear(C,R) -> ReLU -> Linear(R,C); w1 [R][C], w2 [C][R] on the device (:447-452) */
int vfi_cbam_gate(const float* stats_dev, const float* w1_dev, const float* b1_dev, const float* w2_dev, const float* b2_dev, int C, int R,
                  int N, float* scale_dev, void* stream);
/* xs = x * scale[n][c] and ChannelPool comp [N*HW][2] = (max_c xs, mean_c xs) (:451-466) */
int vfi_cbam_scale_compress(const float* x_dev, int cs, const float* scale_dev, int C, int N, int64_t HW, float* xs_dev, int xs_cs,
                            float* comp_dev, void* stream);
/* SpatialGate in place: xs *= sigmoid(bn_a * conv7x7(comp) + bn_b); w [7][7][2] on the device, BatchNorm folded (:469-482) */
int vfi_cbam_spatial(float* xs_dev, int cs, const float* comp_dev, const float* w_dev, float bn_a, float bn_b, int C, int N, int H, int W,
                     void* stream);
/* IFBlock.upsample_flow: convex up-sampling by `factor` of a flow with up to 8 channels (:627-638) */
int vfi_convex_upsample_c(const float* mask_dev, int mask_cs, const float* flow_dev, int flow_cs, float* out_dev, int out_cs, int N, int H,
                          int W, int factor, int flow_channels, void* stream);
/* out = a * mask + b * (1 - mask), mask one channel (:764) */
int vfi_lerp_mask(const float* a_dev, int a_cs, const float* b_dev, int b_cs, const float* mask_dev, int mask_cs, float* out_dev,
                  int out_cs, int C, int64_t pixels, void* stream);
/* out = clamp(a + b, 0, 1) (:161) */
int vfi_add_clamp01(const float* a_dev, int a_cs, const float* b_dev, int b_cs, float* out_dev, int out_cs, int C, int64_t pixels,
                    void* stream);
/* ResynNet's blend, cropped to H x W: softmax over (clamp(m0,-4,4), clamp(m1,-4,4), 0) weights img0, img1, deg (:188-192,766) */
int vfi_ifunet_blend(const float* img0_dev, const float* img1_dev, const float* deg_dev, int img_cs, const float* mask0_dev,
                     const float* mask1_dev, int mask_cs, float* out_dev, int Hp, int Wp, int H, int W, void* stream);
/* out[p, 0:C] = value (timestep planes, :667-670) */
int vfi_fill_channels(float* out_dev, int cs, int C, int64_t pixels, float value, void* stream);

/* ---- RIFE 4.7 / 4.9 model --------------------------------------------------------------- */

typedef struct vfi_rife vfi_rife_t;

/* Build the device-resident network from a reference checkpoint.
 * arch_ver_x10: 47 = architecture "4.7" (rife47.pth / rife49.pth, 124 tensors), 417 = "4.17" (rife417.pth, 128
 * tensors: same IFBlocks on 8 feature channels per frame, encoder Head_417, rife_arch.py:355-375,417-433),
 * 426 = "4.26" (rife426.pth, 158 tensors: 5 IFBlocks with carried block features, encoder Head, :378-398,451-457).
 * `tensors[i]` are host pointers to the state_dict tensors in the key order of rife_spec.rife_shapes(arch)
 * (== torch state_dict order of IFNet(arch)), each in the reference's own layout; `numels[i]` their element
 * counts (checked).  Replaces IFNet(arch_ver).load_state_dict(torch.load(path)) + .to(device),
 * vfi_models/rife/__init__.py:129-135. */
vfi_rife_t* vfi_rife_create(int arch_ver_x10 /* 47 | 417 | 426 */, const float* const* tensors,
                            const int64_t* numels, int n_tensors);
void vfi_rife_destroy(vfi_rife_t* net);

/* (Re)size the workspace: frames of H x W (unpadded), up to `max_batch` tasks per forward and
 * `n_slots` cached frames.  scale_factor as in the node widget (scale_list = [8,4,2,1]/sf,
 * vfi_models/rife/__init__.py:157-160): 0.25, 0.5, 1, 2, 4 — block scales >= 1 must divide the padded size,
 * block scales 0.5 / 0.25 (sf 2 / 4) run the block at 2x / 4x the frame resolution (rife_arch.py:237-276). */
int vfi_rife_configure(vfi_rife_t* net, int H, int W, int max_batch, int n_slots, float scale_factor);

/* Upload-side half of IFNet.forward for ONE input frame: clamp to [0,1], zero-pad to x64
 * (rife_arch.py:476-484) and `encode` (rife_arch.py:414-416,501-503) into frame slot `slot`.
 * frame_dev: [H,W,C] fp32, C>=3 (alpha dropped, vfi_utils.py:139-140).
 * The result depends only on the frame, so it is computed once per frame and shared by both
 * adjacent pairs and all timesteps. */
int vfi_rife_load_frame(vfi_rife_t* net, int slot, const float* frame_dev, int C, void* stream);

/* 8-bit frames (the callers either side of the node — video load / save — deal in uint8 images, a
 * quarter of the PCIe bytes): the same as vfi_rife_load_frame on frame_dev[H,W,C] uint8 with x = u8 / 255 computed on the
 * device (== torch's ``frames.float() / 255`` bit for bit), and the way back: out = round(clamp(in, 0, 1) * 255), ties to even. */
int vfi_rife_load_frame_u8(vfi_rife_t* net, int slot, const uint8_t* frame_dev, int C, void* stream);
/* The same for n frames at once: frames_dev[i] ([H,W,C] fp32, or uint8 when is_u8) -> slot slots[i] (distinct).  ONE launch for the
 * whole list on arch 4.7 (what a batch of the node's loop, rife/__init__.py:195-207, needs resident: 2 frames per task); results are
 * bit-identical to n single calls. */
int vfi_rife_load_frames(vfi_rife_t* net, int n, const int* slots, const void* const* frames_dev, int C, int is_u8, void* stream);
int vfi_f32_to_u8(const float* in_dev, uint8_t* out_dev, int64_t n, void* stream);

/* The per-task hot loop: out[b] = clamp(IFNet(frame[slot0[b]], frame[slot1[b]], t[b]), 0, 1)
 * for b < B.  Replaces the model call + clamp at vfi_models/rife/__init__.py:200-207 and
 * IFNet.forward (rife_arch.py:465-732, arch "4.7").   out_dev: [B,H,W,3]. */
int vfi_rife_interpolate(vfi_rife_t* net, int B, const int* slot0, const int* slot1,
                         const float* timestep, float* out_dev, void* stream);

/* The whole node call for a HOST clip, for hosts that do not want to re-implement the node loop:
 * frames_host [N,H,W,C] fp32 (C >= 3; alpha dropped) -> out_host [*n_out,H,W,3]: frame_0, its new frames, frame_1, ...,
 * frame_last (rife/__init__.py:225-230).  multipliers [N-1] (NULL = 2 everywhere; m <= 1 keeps the frame), skip [N-1] flags
 * (NULL = none; a skipped pair keeps the frame) as rife/__init__.py:149-174; scale_factor as the widget; `batch` tasks per
 * launch (1..32).  out_host == NULL only computes *n_out.  Synchronous; configures `net` itself; uses its own streams and
 * pinned staging.  Replaces RIFE_VFI.vfi's body, vfi_models/rife/__init__.py:149-239. */
int vfi_rife_run(vfi_rife_t* net, const float* frames_host, int N, int H, int W, int C, const int* multipliers,
                 const uint8_t* skip, float scale_factor, int batch, float* out_host, int64_t* n_out);

/* Compute units to leave free for a collective kernel that runs beside the library's launches (process-wide; 0 = none, the
 * default).  The library's persistent kernels launch one workgroup per compute unit and fill it (512 registers per SIMD, up to
 * 150 KB of LDS): a resident RCCL kernel on another stream takes whole units away and the displaced workgroups run as a second
 * round (+37 % per launch while it is resident, profiles/r04_reserved_cus.txt).  With n units reserved the persistent grids are sized
 * for the rest — results are bit-identical for any n (work items are independent of the workgroup that computes them).  The
 * multi-process path (torch.distributed: `all_gather_frames`, bench.py --gpus N) sets it around its overlapped all-gather — what the
 * reference leaves to NCCL's own scheduling.  vfi_get_reserved_cus returns the current value. */
int vfi_set_reserved_cus(int n);
int vfi_get_reserved_cus(void);

/* Host pipeline helper: hipMemcpyAsync(dst, src, bytes, kind, stream) with kind 1 = host -> device, 2 = device -> host, 3 = device ->
 * device; host memory should be pinned (pageable memory makes the call synchronous).  What the node's frame uploads / downloads
 * (`frames.to(device)` / `.cpu()`, rife/__init__.py:195-207,225-230) become: issued from worker threads without the framework's
 * per-copy dispatch (which holds the interpreter lock and queries pointer attributes: 0.6-2.7 ms per call under load, measured). */
int vfi_memcpy_async(void* dst, const void* src, int64_t bytes, int kind, void* stream);

/* A HIP stream of the caller's own (hipStreamNonBlocking, on the calling thread's current device).  The nodes' pair lanes and the HIP
 * graph captures of the op-by-op engines run on such streams: the library keys its scratch (split-K sums, attention partials, splat
 * lists) by (device, stream), and a stream drawn from a framework's shared pool can be handed to two owners.  No reference counterpart:
 * the reference runs everything on torch's current stream (rife/__init__.py:195-230). */
int vfi_stream_create(void** stream_out);
int vfi_stream_destroy(void* stream);
/* One workgroup that spins for `microseconds` of the device's real-time clock on `stream`: the probe with which a host finds out whether
 * two of its streams were bound to the same hardware queue (the HIP runtime multiplexes streams onto a handful of them — 4 by default —
 * and two streams of one queue run strictly one after the other: two pair lanes then overlap nothing).  Two spins on two streams take
 * 1x the time on different queues and 2x on one. */
int vfi_stream_spin(void* stream, int microseconds);

/* Work done by one interpolate call for roofline accounting (algorithmic, per task). */
int vfi_rife_work(vfi_rife_t* net, double* conv_flop_per_task, double* hbm_bytes_per_task);

/* ---- one process, several GPUs ------------------------------------------------------------
 * The reference's node contract is ONE vfi() call in ONE ComfyUI process (__init__.py:24-48,
 * vfi_models/rife/__init__.py:77-91), so the multi-GPU form that is a drop-in is single-process: one host thread + one
 * stream per visible device (each thread calls vfi_init(device) once), tasks block-partitioned over the devices, every
 * device copying its own shard of new frames into the shared host output tensor.  RCCL (ncclCommInitAll, bound at first
 * use by dlopen) carries the two exchanges north_star names: the weights, once, as one flat buffer, and the all-gather of new
 * frames for device-side consumers.  All vfi_comm_* calls are made by ONE thread for all devices. */

/* A second copy of `src` for the CURRENT device: same architecture and weight layout, weight arena allocated but EMPTY —
 * fill it with vfi_comm_broadcast over the arenas (vfi_rife_weights).  Configure / load_frame / interpolate as usual. */
vfi_rife_t* vfi_rife_clone_empty(const vfi_rife_t* src);
/* The network's weights as one flat device buffer (every packed tensor of vfi_rife_create, 256-byte aligned pieces). */
int vfi_rife_weights(vfi_rife_t* net, float** arena_dev, int64_t* count);

typedef struct vfi_comm vfi_comm_t;
/* ncclCommInitAll over `devices` (HIP device ids, distinct); NULL + vfi_last_error() when RCCL is unavailable. */
vfi_comm_t* vfi_comm_create(int n_devices, const int* devices);
void vfi_comm_destroy(vfi_comm_t* comm);
int vfi_comm_size(const vfi_comm_t* comm);
/* bufs_dev[i] (on devices[i], `count` floats) <- bufs_dev[root]; streams[i] = a hipStream_t created on devices[i]. */
int vfi_comm_broadcast(vfi_comm_t* comm, float* const* bufs_dev, int64_t count, int root, void* const* streams);
/* In-place all-gather-v: bufs_dev[i] holds sum(counts) floats, rank r's own block already in place at offset
 * counts[0] + ... + counts[r-1]; afterwards every buffer holds every block (grouped per-root broadcasts, so counts may differ). */
int vfi_comm_all_gather_v(vfi_comm_t* comm, float* const* bufs_dev, const int64_t* counts, void* const* streams);

/* The copy list of that in-place all-gather: `n` ranks, per-rank counts -> quadruples (source rank, destination rank, offset,
 * count) into `plan` (4 int64 per copy; cap = capacity in int64; plan may be NULL to count).  Pure host function: what the direct
 * full-mesh path (VFI_ALLGATHER=direct: one hipMemcpyPeerAsync per ordered device pair on its own stream — one xGMI link each)
 * executes.  The default is grouped per-root ncclBroadcast (VFI_ALLGATHER=rccl): the direct form has not yet run on two or more
 * physical devices.  Returns the number of copies or < 0. */
int64_t vfi_comm_plan_all_gather(int n, const int64_t* counts, int64_t* plan, int64_t cap);
/* What vfi_comm_all_gather_v uses in this process: 0 = direct peer copies, 1 = RCCL grouped broadcasts. */
int vfi_comm_all_gather_mode(void);

/* ---- CAIN (vfi_models/cain/cain_arch.py CAIN(depth=3), common.py) ----------------------------------------------------------- */

/* CAIN frame-in for one [H,W,C] fp32 frame (C >= 3; channels 0..2 used): mean_dev[c] = the frame's mean of channel c (sub_mean,
 * common.py:7-10); the mean-free frame reflect-padded to a multiple of 128 (InOutPaddings, floor half before, :12-23) and
 * pixel-unshuffled by 8 (pixel_shuffle(1/8), :208-210) into out[Hp/8, Wp/8, out_cs] channels 0..191 (channel c*64 + dy*8 + dx).
 * The frame is not written.  workspace_dev >= 3 KiB.  Fails when the padding on a side is not smaller than the frame. */
int vfi_cain_frame_in(const float* frame_dev, int C, int H, int W, float* out_dev, int out_cs, float* mean_dev, float* workspace_dev,
                      int64_t workspace_bytes, void* stream);
/* CAIN frame-out: pixel_shuffle(8) of feat [N, Hp/8, Wp/8, 192], cropped to H x W (the inverse padding), + (m0 + m1) / 2 per channel
 * with means_dev [N][2][3] (frame 0's, frame 1's means), into out [N,H,W,3] fp32.  No clamp (cain_arch.py:66-74). */
int vfi_cain_frame_out(const float* feat_dev, const float* means_dev, float* out_dev, int N, int H, int W, void* stream);
/* Squeeze-and-excitation channel attention plus residual (CALayer + RCAB's `out += res`, common.py:132-178), contiguous NHWC:
 * out[n,p,c] = t[n,p,c] * sigmoid(b2 + w2 . relu(b1 + w1 . mean_p t[n,p,:]))[c] + x[n,p,c]; w1 [R][C], w2 [C][R] (1x1 conv weights),
 * C % 4 == 0, C <= 256, R <= 64.  Deterministic: per-workgroup partial sums in fixed slots, summed in a fixed order (no atomics).
 * out may alias t or x.  workspace_dev >= N * 257 * C floats. */
int vfi_channel_attention(const float* t_dev, const float* x_dev, float* out_dev, int N, int64_t HW, int C, const float* w1_dev,
                          const float* b1_dev, const float* w2_dev, const float* b2_dev, int R, void* workspace_dev, int64_t workspace_bytes,
                          void* stream);

typedef struct vfi_cain vfi_cain_t;
/* The 494 state_dict tensors of CAIN(depth=3) in cain_spec.cain_shapes() order (fp32 host memory, copied). */
vfi_cain_t* vfi_cain_create(const float* const* tensors, const int64_t* numels, int n_tensors);
void vfi_cain_destroy(vfi_cain_t* net);
/* model(frame0, frame1)[0] for N pairs in one call (cain_arch.py:56-74): frame0_dev / frame1_dev = host arrays of N device pointers
 * to [H,W,C] fp32 frames (C >= 3), out_dev [N,H,W,3].  Frames are not written.  A pair's result does not depend on its batch mates
 * wherever every layer takes the Winograd kernel (chosen per image: feature maps from about 64 x 128, i.e. 512 x 1024 frames). */
int vfi_cain_forward(vfi_cain_t* net, const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W,
                     float* out_dev, void* stream);
int vfi_cain_release_workspace(vfi_cain_t* net);
int64_t vfi_cain_workspace_bytes(const vfi_cain_t* net);

/* ---- SepConv++ (vfi_models/sepconv/sepconv_enhanced.py Network) ------------------------------------------------------------ */

/* SepConv++'s output stage for N frame pairs in one pass: frame0_dev / frame1_dev = host arrays of N device pointers to [H,W,C] fp32
 * frames (C >= 3, channels 0..2 used; not written); ver0 / ver1 / hor0 / hor1 = the four heads' 51-tap filters (netVerone, netVertwo,
 * netHorone, netHortwo) as NHWC [N, Hp, Wp, head_cs] tensors (Hp >= H, Wp >= W; each pointer at its head's first channel, so one
 * tensor may hold all four).  out_dev [N,H,W,3] = (S0 + S1)[:3] / n with S_f = sepconv(pad25_replicate(frame_f) | 1, ver_f, hor_f) and
 * n = (S0 + S1)[3], set to 1 where |n| < 0.01 (sepconv_enhanced.py:644-700); the frames are read with clamp-to-frame addressing.  No
 * clamp of the result. */
int vfi_sepconv_pair_out(const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W, const float* ver0_dev,
                         const float* ver1_dev, const float* hor0_dev, const float* hor1_dev, int head_cs, int Hp, int Wp, float* out_dev,
                         void* stream);
/* The same output stage for the rows [row0, row0 + rows) of ONE pair's frame (row0 a multiple of 8, the stage's tile rows; the band inside
 * the H-row frame), from filters that exist for those rows only: tap f of the pixel (row0 + r, x) of head h at
 * h_dev[(r * Wp + x) * pixel_stride + f * tap_stride] — NHWC (pixel_stride = the channel stride, tap_stride = 1) or planar (pixel_stride = 1,
 * tap_stride = the band's pixels).  out_dev is the whole frame's [H,W,3]; only the band's rows are written.  The frames are read with
 * clamp-to-frame addressing over all H rows.  row0 = 0, rows = H is one pair of vfi_sepconv_pair_out: same launch, same bits. */
int vfi_sepconv_pair_out_rows(const float* frame0_dev, const float* frame1_dev, int C, int H, int W, const float* ver0_dev, const float* ver1_dev,
                              const float* hor0_dev, const float* hor1_dev, int64_t pixel_stride, int64_t tap_stride, int Wp, int row0, int rows,
                              float* out_dev, void* stream);

typedef struct vfi_sepconvnet vfi_sepconvnet_t;
/* The 88 state_dict tensors of SepConv++'s Network in sepconv_spec.sepconv_shapes() order (fp32 host memory, copied). */
vfi_sepconvnet_t* vfi_sepconvnet_create(const float* const* tensors, const int64_t* numels, int n_tensors);
void vfi_sepconvnet_destroy(vfi_sepconvnet_t* net);
/* model(frame0, frame1) for N pairs in one call (sepconv_enhanced.py:605-700): frame0_dev / frame1_dev = host arrays of N device pointers
 * to [H,W,C] fp32 frames (C >= 3), out_dev [N,H,W,3].  Frames are not written.  The pairs run one after another through the same
 * launches as a call with one pair, so a pair's result does not depend on its batch mates (whichever kernel each layer takes); the
 * workspace is sized for one pair. */
int vfi_sepconvnet_forward(vfi_sepconvnet_t* net, const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W,
                           float* out_dev, void* stream);
int vfi_sepconvnet_release_workspace(vfi_sepconvnet_t* net);
int64_t vfi_sepconvnet_workspace_bytes(const vfi_sepconvnet_t* net);
/* Frame size, in padded pixels (both sides rounded up to even).  Without large frames the head stage materialises the four heads' first
 * layer [Hp, Wp, 256], which the layers serve below 4 GiB: vfi_sepconvnet_max_pixels() = 4 194 303 (up to 2 097 151 on plain layer forms,
 * 1080x1920 among them; above that on the large-image forms).  vfi_sepconvnet_set_large_frames(net, 1) runs the head stage of every frame
 * over 2 097 151 pixels in horizontal bands, so that tensor exists for one band at a time and [Hp, Wp, 64] below 2 GiB sets the limit:
 * vfi_sepconvnet_large_max_pixels() = 8 388 607, which takes 2160x3840.  Frames of at most 2 097 151 pixels run the same launches and give
 * the same bits whatever the switch says.  vfi_sepconvnet_forward refuses a frame over the object's limit
 * (vfi_sepconvnet_object_max_pixels; 0 for a null object), and with large frames on one so wide that a band of 8 rows with its halo of 8,
 * [16, Wp, 256], reaches 2 GiB (Wp > 131 071), before it allocates or launches anything. */
int vfi_sepconvnet_set_large_frames(vfi_sepconvnet_t* net, int on);
int64_t vfi_sepconvnet_max_pixels(void);
int64_t vfi_sepconvnet_large_max_pixels(void);
int64_t vfi_sepconvnet_object_max_pixels(const vfi_sepconvnet_t* net);

/* ---- FLAVR (vfi_models/flavr/flavr_arch.py UNet_3D_3D("unet_18", 4 inputs, "concat", "transpose"), resnet_3D.py) ------------------- */

/* In the functions below a tensor with four time slices is addressed as base + pixel * ps + t * ss + channel (ps = pixel stride, ss =
 * slice stride, in floats, multiples of 4; base 16-byte aligned), which covers the network's bordered [H, W, 6, C] feature maps (base at
 * slice 1, ps = 6 C, ss = C), halves of concat buffers and plain [H, W, 4, C] tensors alike. */

/* FLAVR frame-in for a window of four [H,W,C] fp32 frames (frames_dev = host array of 4 device pointers; C >= 3, channels 0..2 used; not
 * written): replicate padding to Hp x Wp = multiples of 16, floor half before (InputPadder(16), flavr_arch.py:200-209); mean_dev[c] = mean
 * of channel c over the four padded frames (mean_dev[3] = 0); out_dev [Hp, Wp, 4, 4] = (frame_t - mean, 0) time-interleaved.  The mean
 * is deterministic: 256 fixed slots summed in order.  workspace_dev >= 4 KiB. */
int vfi_flavr_frame_in(const float* const* frames_dev, int C, int H, int W, float* out_dev, float* mean_dev, float* workspace_dev, int64_t workspace_bytes,
                       void* stream);
/* FLAVR stem: relu(Conv3d(3, 64, (3,7,7), stride (1,2,2), padding (1,3,3))(x)) for x_dev [Hp, Wp, 4, 4] (frame-in's layout), w_dev
 * [64,3,3,7,7] and bias_dev [64] (nullable) on the device; output pixel (y, x) of ceil(Hp/2) x ceil(Wp/2), slice t, channel c at
 * out_dev[(y * Wo + x) * out_cs + t * 64 + c].  workspace_dev >= 112896 bytes (the repacked weights). */
int vfi_flavr_stem(const float* x_dev, int Hp, int Wp, const float* w_dev, const float* bias_dev, float* out_dev, int out_cs, float* workspace_dev,
                   int64_t workspace_bytes, void* stream);
/* Conv3d(Cin, Cout, 1, stride (1, s, s), bias=False), s = 1 or 2 (BasicBlock.downsample): conv1x1 = a vfi_conv_create_ex(0, w, NULL, Cout,
 * Cin, 1, 1, ...) object; the input (ps / ss addressing, Hin x Win pixels) is sub-sampled into sub_dev [h, w, 4, Cin] (h = ceil(Hin / s))
 * and out_dev [h, w, 4, Cout] is the 1x1 layer on the MFMA kernel over it. */
int vfi_flavr_down1x1(const vfi_conv_t* conv1x1, int Cin, int Cout, const float* in_dev, int64_t in_ps, int64_t in_ss, int Hin, int Win, int stride,
                      float* sub_dev, float* out_dev, void* stream);
/* SEGating fused with what follows it: y = sigmoid(b + w . mean_{pixels, t} x) (w_dev [C][C], b_dev [C]; resnet_3D.py:100-116), then
 * mode 0: out = relu(x * y + res) (BasicBlock, :140-151), mode 1: out = leaky_relu(x * y, 0.2) (decoder, flavr_arch.py:176-188).  x, res
 * and out in ps / ss addressing over `pixels` pixels; out may alias x.  C % 4 == 0, C <= 1024.  Deterministic: at most 1024 fixed slots
 * summed in order.  workspace_dev >= (1024 * C + C) floats. */
int vfi_flavr_gate(const float* x_dev, int64_t x_ps, int64_t x_ss, const float* res_dev, int64_t res_ps, int64_t res_ss, float* out_dev, int64_t out_ps,
                   int64_t out_ss, int64_t pixels, int C, const float* w_dev, const float* b_dev, int mode, float* workspace_dev, int64_t workspace_bytes,
                   void* stream);
/* FLAVR frame-out: Conv2d(64, 3, 7)(ReflectionPad2d(3)(feat)) + bias + mean for the H x W crop at (pad_top, pad_left) of feat_dev
 * [Hp, Wp, 64] (Hp, Wp >= 4): w_dev [>= 3, 64, 7, 7] (the first three output channels are used), bias_dev [>= 3], mean_dev [>= 3] on the
 * device, out_dev [H, W, 3].  No clamp.  workspace_dev >= 50176 bytes. */
int vfi_flavr_frame_out(const float* feat_dev, int Hp, int Wp, const float* w_dev, const float* bias_dev, const float* mean_dev, int pad_top, int pad_left,
                        int H, int W, float* out_dev, float* workspace_dev, int64_t workspace_bytes, void* stream);

typedef struct vfi_flavr vfi_flavr_t;
/* The state_dict tensors of FLAVR in flavr_spec.flavr_shapes(n_outputs) order (59 for n_outputs == 1, else 76; fp32 host memory, copied). */
vfi_flavr_t* vfi_flavr_create(const float* const* tensors, const int64_t* numels, int n_tensors, int n_outputs);
void vfi_flavr_destroy(vfi_flavr_t* net);
/* unpad(model([pad(f) for f in window])[0]) for N windows in one call (vfi_models/flavr/__init__.py:67-84): frames_dev = host array of 4 N
 * device pointers to [H,W,C] fp32 frames (window n = pointers 4 n .. 4 n + 3; C >= 3; not written), out_dev [N,H,W,3].  The windows run
 * one after another through the same launches as a call with one window, so a window's result does not depend on its batch mates; the
 * workspace is sized for one window.  Frames whose padded size exceeds 2^21 - 1 pixels (1088 x 1920 fits) are refused before any launch
 * (vfi_flavr_set_large_frames below raises that limit to 8 388 607). */
int vfi_flavr_forward(vfi_flavr_t* net, const float* const* frames_dev, int N, int C, int H, int W, float* out_dev, void* stream);
int vfi_flavr_release_workspace(vfi_flavr_t* net);
int64_t vfi_flavr_workspace_bytes(const vfi_flavr_t* net);
/* The largest padded frame (Hp * Wp, sides rounded up to multiples of 16) an object serves as created: 2 097 151, the last up-convolution's
 * [Hp, Wp, 256] fp32 tensor below 2 GiB.  After vfi_flavr_set_large_frames(net, 1) the limit of that object is
 * vfi_flavr_large_max_padded_pixels() = (2^31 - 1) / 256 = 8 388 607 (2160 x 3840 fits, 2176 x 3856 does not): the same tensor within the
 * layer kernels' bound for one operand image, every layer object with vfi_conv_allow_huge; about 6.24 KB of workspace per padded pixel.
 * vfi_flavr_object_max_padded_pixels(net) is the limit vfi_flavr_forward applies (0 for a null object).  Frames at or under the first limit
 * take the same launches with the switch on or off. */
int64_t vfi_flavr_max_padded_pixels(void);
int64_t vfi_flavr_large_max_padded_pixels(void);
int64_t vfi_flavr_object_max_padded_pixels(const vfi_flavr_t* net);
/* on != 0: the object serves padded frames up to vfi_flavr_large_max_padded_pixels(); 0 (every object as created): up to vfi_flavr_max_padded_pixels() */
int vfi_flavr_set_large_frames(vfi_flavr_t* net, int on);

/* ---- AMT (vfi_models/amt/amt_arch.py AMT_S / AMT_L / AMT_G): the kernels beside the layer objects ------------------------------------------- */

/* The target side of the correlation pyramid without the volume: corr[q][p] = <f0[q], f1[p]> / sqrt(D) is linear in f1, so
 * avg_pool2d(corr[q]) = <f0[q], avg_pool2d(f1)> (BidirCorrBlock.__init__, :1083-1097).  f_dev [h,w,D] -> pooled_dev = levels 1..3
 * back to back, [h>>l][w>>l][D] each (odd sizes floored as avg_pool2d does): ((h>>1)(w>>1) + (h>>2)(w>>2) + (h>>3)(w>>3)) D floats.
 * D % 4 == 0; h, w >= 16 (below, the coarsest level is one pixel wide and the reference is all-NaN). */
int vfi_amt_pool_features(const float* f_dev, int h, int w, int D, float* pooled_dev, void* stream);
/* One direction of BidirCorrBlock.__call__ (:1099-1131) for radius 3 and 4 levels: for query pixel q with c = (x, y) + flow[q] * scale
 * (two fp32 roundings, as `coord + flow * t_scale`, :1200), out[q, lvl * 49 + a * 7 + b] = bilinear_zero_pad(<fq[q], ft_lvl[.]> / sqrt(D),
 * x = c.x / 2^lvl + (a - 3), y = c.y / 2^lvl + (b - 3)): the first window index moves x (the reference adds its (dy, dx) deltas to (x, y)
 * coordinates, :1112-1120).  fq_dev, ft_dev [h,w,D]; ft_pooled_dev from vfi_amt_pool_features(ft_dev); flow_dev [h,w,flow_cs] = (x, y)
 * first; out_dev [h,w,out_cs], 196 channels written (the other direction goes to out_dev + 196 with fq / ft exchanged).  Nothing of
 * size (h w)^2 exists.  D % 4 == 0, D <= 256; h, w >= 16. */
int vfi_amt_corr_lookup(const float* fq_dev, const float* ft_dev, const float* ft_pooled_dev, const float* flow_dev, int flow_cs, float scale,
                        int h, int w, int D, float* out_dev, int out_cs, void* stream);
/* Conv2d(Cin, Cout, 7, stride 1, padding 3) + bias (nullable) + activation (0 none, 1 leaky relu(slope), 3 PReLU(prelu_dev[Cout])) for thin
 * layers, Cin <= 96, Cout <= 128: convf1 of the update blocks (:977, :1031; 4 -> 128 in AMT-G) and AMT-L's / AMT-G's comb_block (:1322-1326).  in [N,H,W,in_cs], out
 * [N,H,W,out_cs].  w_dev: [7][7][Cin4][CoutP] zero-padded, Cin4 = Cin rounded up to 4, CoutP = Cout rounded up to 4 (Cout <= 4) or 16. */
int vfi_conv7x7(const float* in_dev, int in_cs, const float* w_dev, const float* bias_dev, const float* prelu_dev, float slope, int act,
                int Cin, int Cout, float* out_dev, int out_cs, int N, int H, int W, void* stream);
/* leaky_relu(F.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=False), slope) in one pass, scale 2 or 4: in [N,h,w,in_cs],
 * a C-channel window; out [N,scale h,scale w,out_cs], C channels written, each once.  AMT-G's update3_high / update2_high re-read the low
 * blocks' lookup output resized by 2 / 4 (:1537-1543, :1558-1564) and open with a 1x1 convolution: the object runs that convolution on
 * the low-resolution map and this kernel on its output (the two commute: the bilinear weights sum to 1), so the resized 392-channel tensor
 * never exists.  float4 accesses when C, both strides and both pointers are multiples of 4 floats, scalar ones otherwise. */
int vfi_amt_upsample_lrelu(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int h, int w, int C, int scale, float slope,
                           void* stream);
/* multi_flow_combine up to comb_block's input (:883-900): out[.., 3 i + c] = sigmoid(mask_i) * warp(img0, flow0_i)[c] + (1 - sigmoid(mask_i))
 * * warp(img1, flow1_i)[c] + mean + res_i[c] for the num_flows flow pairs; warp as amt_arch.warp (:26-34: border, align_corners=True).
 * img{0,1} [Hp,Wp,img_cs] mean-removed, fin [Hp,Wp,fin_cs] = flow0 (2 n) | flow1 (2 n) | mask logits (n) | res (3 n), mean_dev[0]. */
int vfi_amt_combine_warps(const float* img0_dev, const float* img1_dev, int img_cs, const float* fin_dev, int fin_cs, const float* mean_dev,
                          int num_flows, float* out_dev, int out_cs, int Hp, int Wp, void* stream);
/* The tail (:901, :1273, InputPadder.unpad): out [H,W,3] = clamp(mean over flows of warps + comb, 0, 1) cropped at (pad_top, pad_left) */
int vfi_amt_combine_out(const float* warps_dev, int warps_cs, const float* comb_dev, int comb_cs, int num_flows, float* out_dev, int Hp,
                        int Wp, int pad_top, int pad_left, int H, int W, void* stream);

typedef struct vfi_amt vfi_amt_t;
/* The state_dict tensors of AMT-S (variant 0: 213), AMT-L (variant 1: 207) or AMT-G (variant 2: 259) in amt_spec.amt_shapes(variant) order
 * (fp32 host memory, copied).  Replaces AMT_S / AMT_L / AMT_G.__init__ + load_state_dict (vfi_models/amt/amt_arch.py:1153-1188, :1297-1332,
 * :1441-1471; amt/__init__.py:61-66). */
vfi_amt_t* vfi_amt_create(const float* const* tensors, const int64_t* numels, int n_tensors, int variant);
void vfi_amt_destroy(vfi_amt_t* net);
/* clamp(unpad(model(pad(frame0), pad(frame1), embt = t)), 0, 1) for ONE pair and n_t timesteps ts_host[0 .. n_t) in (0, 1) (amt_arch.py:1205-1285,
 * :1349-1429; amt/__init__.py:88-97): frames [H,W,C>=3] fp32 (not written), out_dev [n_t,H,W,3].  Once per call: the centred replicate pad to
 * multiples of 16, mean_, the feature encoder on both frames, both pyramid encoders, the pooled feature maps.  Per timestep: decoders, lookups,
 * update blocks, multi_flow_combine, clamp, un-pad; a timestep's result does not depend on the others of its call.  No correlation volume is
 * built.  AMT-G (:1494-1581) adds update3_high / update2_high after the low blocks, at 1/4 and 1/2 resolution, on the same lookup output.
 * Frames whose padded side is below 128 (the reference is all-NaN there) or whose padded size exceeds 2^23 - 1 pixels (AMT-G: 6 100 805,
 * its widest activation has 88 floats per padded pixel; 12 201 611 after vfi_amt_set_large_frames, below) are refused before any launch. */
int vfi_amt_forward(vfi_amt_t* net, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, const float* ts_host, int n_t,
                    float* out_dev, void* stream);
/* Large frames.  on != 0 on an AMT-G object: it serves padded frames up to vfi_amt_large_max_padded_pixels(2) = (2^32 - 1) / 352 =
 * 12 201 611 pixels (2160 x 3840 pads to 8 294 400), its widest buffer staying below 4 GiB: every layer that meets an image of 2 GiB or more
 * has a large-image form (docs/design/amt.md "4K"), and the object's layers are given vfi_conv_allow_large_res_prelu for the one that needs
 * it, the ResBlock's closing residual + PReLU.  0 (every object as created): 6 100 805 pixels, and the launches, refusals and bits of before.
 * AMT-S and AMT-L: the switch changes nothing — vfi_amt_large_max_padded_pixels(0 / 1) is their 2^23 - 1, the call sets nothing on the object
 * or its layers, and the forward issues the same launches.  vfi_amt_object_max_padded_pixels is the limit vfi_amt_forward applies to that
 * object; vfi_amt_large_max_padded_pixels of an unknown variant is 0. */
int vfi_amt_set_large_frames(vfi_amt_t* net, int on);
int64_t vfi_amt_large_max_padded_pixels(int variant);
int64_t vfi_amt_object_max_padded_pixels(const vfi_amt_t* net);
int vfi_amt_release_workspace(vfi_amt_t* net);
int64_t vfi_amt_workspace_bytes(const vfi_amt_t* net);

/* ---- ATM-lite / ATM-base (vfi_models/atm/network_lite.py, network_base.py Network, attention.py): the kernels beside the layer objects and the GMFSS ops */

/* Multi-head (8) attention over fixed windows of token MAPS, for both windowed blocks of ATM: cross != 0 is AttentionToMotion inside ATMFormer
 * (attention.py:187-213, :265-334: q of frame f against k, v of frame f ^ 1, same window), cross == 0 is WindowAttention inside RefineBottleneck
 * (:370-390, :433-495).  q / k / v_dev: channel windows (C channels, head hd at hd * C / 8) of token maps holding the two frames' h x w tokens
 * back to back (token (f h + y) w + x), already normed (norm1) and projected; (C, window) = (224, 8) or (352, 12) (ATM-lite), (384, 8) or (672, 12)
 * (ATM-base), every other pair is refused; shift = 0 or window / 2.
 * pad_if_needed's centre padding to a window multiple, torch.roll by -shift, window_partition and their inverses (:8-71, :275-277, :313, :323-331)
 * are the kernel's addressing: no padded, rolled or partitioned copy exists; a window slot outside the map reads token `pad_token` of q / k / v
 * (the caller keeps one zero token behind the maps, so that after norm1 and the projections it is what the reference's zero padding becomes;
 * required when h or w is no multiple of the window).  Additive mask -100 (not -inf) where the region labels of query and key differ: the nine
 * centre-pad regions and, with a shift, the nine shift regions, BOTH taken at the slot's position in the rolled layout (the reference builds
 * its pad mask before the roll and applies it after, :28-62, :282-303).  Scores and probabilities never leave the chip; q k^T and p v run on
 * the fp32 matrix cores.  out_dev [2,h,w,out_cs]: softmax(q k^T / sqrt(C / 8) + mask) v per head, rows of padding dropped.  offsets_dev
 * (nullable, cross only) [2,h,w,8,2]: per head sum_n p[n] (key x - query x, key y - query y) inside the window, the input of vfi_atm_motion_mlp
 * (:207-208; the relative_coord buffer is not read: atm_spec.load_file checks that it holds exactly these offsets). */
int vfi_atm_window_attention(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, int64_t pad_token,
                             float* out_dev, int out_cs, float* offsets_dev, int h, int w, int C, int window, int shift, int cross, void* stream);
/* The same with the nine centre-pad regions of the mask taken from a label_h x label_w map centred in the padded layout instead of the h x w
 * map itself (both must pad to the same window multiple; label = own is vfi_atm_window_attention).  This is what the reference's shifted
 * block does inside an ensemble forward: it keeps the mask of its first call and re-uses it while the padded map has as many positions
 * (:279-305), so a level whose map pads to the previous level's layout is masked with that level's pad regions.  Tokens, the roll and the
 * nine shift regions are the h x w map's. */
int vfi_atm_window_attention_labels(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, int64_t pad_token,
                                    float* out_dev, int out_cs, float* offsets_dev, int h, int w, int label_h, int label_w, int C, int window,
                                    int shift, int cross, void* stream);
/* AttentionToMotion.mlp over the heads (:143-146, :209-211): out[f * out_frame_stride + p * out_cs + coord] = w2 . gelu(w0 offsets[f][p][:, coord]
 * + b0) + b2 for both frames, tokens p < tokens_per_frame and coord 0 (x), 1 (y); w0 [4][8], b0 [4], w2 [4], b2 [1] on the device. */
int vfi_atm_motion_mlp(const float* offsets_dev, const float* w0_dev, const float* b0_dev, const float* w2_dev, const float* b2_dev, float* out_dev,
                       int out_cs, int64_t out_frame_stride, int64_t tokens_per_frame, void* stream);
/* gelu(Conv2d(C, C, 3, 1, 1, groups = C)(x) + bias): Mlp.dwconv + Mlp.act (:74-85, :116-119).  w_dev [9][C] (tap-major), bias_dev [C]; C % 4 == 0. */
int vfi_atm_dwconv3x3_gelu(const float* in_dev, int in_cs, const float* w_dev, const float* bias_dev, float* out_dev, int out_cs, int N, int H, int W,
                           int C, void* stream);
/* The taps of Conv2d(C, C, 3, stride, padding = dilation, dilation) (CrossScaleFeatureFusion.layers, network_lite.py:38-50: stride 2 / 4,
 * dilation 1 / 2) gathered for a 1x1 layer: out[n, y, x, t C + c] = in[n, y stride + (t / 3 - 1) dilation, x stride + (t % 3 - 1) dilation, c],
 * zero outside; out [N, (H - 1) / stride + 1, (W - 1) / stride + 1, out_cs].  The convolution is vfi_conv_create_ex(0, w1, bias, C, 9 C, 1, 1, ...)
 * with w1[co][t C + ci] = w[co][ci][t] on the MFMA kernel.  C % 4 == 0. */
int vfi_atm_gather_taps(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, int stride, int dilation, void* stream);
/* The interleave of ConvTranspose2d(Cin, C, 2, 2, 0) (deconv(), network_lite.py:27-32, :213-232, :256-268) run as a 1x1 layer with 4 C outputs
 * (output channel (2 ky + kx) C + co; bias and PReLU slopes repeated per tap): out[n, 2 y + ky, 2 x + kx, c] = in[n, y, x, (2 ky + kx) C + c]. */
int vfi_atm_depth_to_space2(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, void* stream);
/* A synthesis step (network_lite.py:488-490, :515-517): w_k = flow_warp(src_k, flow_k) (flow_warp.py:26-60: bilinear, zeros, align_corners=True),
 * I_t = sigmoid(m) w_0 + (1 - sigmoid(m)) w_1 with motion_dev [H,W,motion_cs] = (flow0 xy, flow1 xy, m).  out_dev [H,W,out_cs], 15 channels:
 * (orig0 | w_0 | orig1 | w_1 | I_t), the layout the refinement net reads (:410); orig (nullable, both or none): channels 0..2 / 6..8 are left alone. */
int vfi_atm_blend_warps(const float* src0_dev, const float* src1_dev, int src_cs, const float* orig0_dev, const float* orig1_dev, int orig_cs,
                        const float* motion_dev, int motion_cs, float* out_dev, int out_cs, int H, int W, void* stream);
/* The last step (:421, :524-525, InputPadder.unpad): out [H,W,3] = clamp(I_t + 2 sigmoid(res) - 1, 0, 1) cropped at (pad_top, pad_left) */
int vfi_atm_refine_out(const float* it_dev, int it_cs, const float* res_dev, int res_cs, float* out_dev, int Hp, int Wp, int pad_top, int pad_left, int H,
                       int W, void* stream);
/* The ensemble's score, fused (Network.global_alignmentness, network_lite.py:540-554): loss_dev[0] = mean over [3,Hp,Wp] of |flow_warp(frame 0,
 * flow0) - flow_warp(frame 1, flow1)|.  pair_dev [2,Hp,Wp,pair_cs]: the two frames, channels 0..2; motion_dev [h,w,motion_cs]: a coarse
 * motion map, channels 0..3 = flow0 xy, flow1 xy; Hp = f h and Wp = f w with one whole factor f.  Per full-resolution pixel the four flow
 * channels are interpolated (upsample_flow: F.interpolate align_corners=True, source coordinate = (h - 1) / (Hp - 1) * y, scale 0 for a
 * one-pixel side, so h = 1 or w = 1 gives a constant; values x f), both frames are sampled at pixel + flow with the device function
 * vfi_atm_blend_warps uses, and |a - b| is summed over the channels: no full-resolution flow map or warped image is written.  The sum is
 * deterministic: a fixed tree inside each 256-pixel workgroup (wave shuffles, then LDS), one float per workgroup into scratch_dev
 * (vfi_atm_alignment_scratch_floats(Hp, Wp) floats), and a one-workgroup second launch that adds them in index order in double.  No float
 * atomics; the grid depends on the frame size alone, so the same input gives the same bits on every run and every device. */
int vfi_atm_alignment_loss(const float* pair_dev, int pair_cs, int Hp, int Wp, const float* motion_dev, int motion_cs, int h, int w, float* scratch_dev,
                           float* loss_dev, void* stream);
int64_t vfi_atm_alignment_scratch_floats(int Hp, int Wp);
/* The ensemble's choice on the device (multiscale_global_motion_ensemble, :583-597): level = the first of 0, 1, 2 whose loss equals the
 * smallest of losses_dev[0..2] (Python's min, then the == chain: ties go to the lower level).  motion{k}_dev [h16 >> k, w16 >> k, motion_cs]
 * (h16, w16 >= 4; multiples of 4 in the network).  Channels 0..3 of out_dev [h16,w16,out_cs] = the chosen map's flows resized x 1 / 2 / 4 (upsample_flow:
 * align_corners=True, values x factor: vfi_resize_bilinear_ac's arithmetic; level 0 is copied); channels 4.. of out_dev are not written.
 * record_dev (nullable) [4]: the three losses and the level (as a float).  No host synchronisation. */
int vfi_atm_select_flow(const float* losses_dev, const float* motion0_dev, const float* motion1_dev, const float* motion2_dev, int motion_cs, int h16,
                        int w16, float* out_dev, int out_cs, float* record_dev, void* stream);

typedef struct vfi_atm vfi_atm_t;
/* The 232 weight tensors of ATM-lite in atm_spec.weight_shapes() order = the state dict of network_lite.Network without its four relative_coord
 * buffers (fp32 host memory, copied).  Replaces Network() + load_state_dict (vfi_models/atm/__init__.py:115-142). */
vfi_atm_t* vfi_atm_create(const float* const* tensors, const int64_t* numels, int n_tensors);
/* The same for either model: variant 0 = ATM-lite (what vfi_atm_create makes), 1 = ATM-base (network_base.Network: hidden_dims 24 / 48 / 96 / 192,
 * 384 / 672-wide tokens, mlp_ratio 4, motion heads 576 / 768 wide, refinement width 64).  Both state dicts have the same 232 names in the same
 * order, so a file of the other model is told by its per-tensor element counts: NULL, with an error that names the variant. */
vfi_atm_t* vfi_atm_create_variant(const float* const* tensors, const int64_t* numels, int n_tensors, int variant);
void vfi_atm_destroy(vfi_atm_t* net);
/* Network.forward_normal (network_lite.py:425-538)["I_t"] for ONE pair: frames [H,W,C>=3] fp32 (not written) are padded to multiples of 64
 * (centred, replicate: InputPadder(dims, 64), atm/__init__.py:11-34, :62-68), out_dev [H,W,3] is the un-padded result, clamped to [0, 1].
 * global_motion: 1 = "On", 0 = "Off (fastest)" (:76-80); the multi-scale ensemble is vfi_atm_forward_ensemble's, and any other value
 * is refused here.  A frame whose padded size exceeds
 * vfi_atm_max_padded_pixels() = (2^31 - 1) / 320 = 6 710 886 pixels is refused before any launch: the widest per-image buffer (the refinement
 * net's input, 76 channels padded to 80) has 320 bytes per padded pixel and the layers index an image with 32 bits (1088 x 1920 fits).  That
 * is ATM-lite's limit; the limit that vfi_atm_forward applies is the object's own, vfi_atm_object_max_padded_pixels(net): for ATM-base
 * (2^31 - 1) / 512 = 4 194 303 pixels, its widest per-image buffer being the refinement net's full-resolution concat buffer of 2 * 64 = 128
 * channels (its input is 116 channels padded to 120, the last transposed convolution's taps r8(4 * 101) / 4 = 102 floats per full-resolution
 * pixel, the 4 C MLP buffers 1536 / 64): 1472 x 2560 fits, 2176 x 3840 does not.
 * After vfi_atm_set_large_frames(net, 1) the limit of that object is vfi_atm_large_max_padded_pixels(variant): (2^32 - 1) / 320 = 13 421 772
 * pixels for ATM-lite, (2^32 - 1) / 512 = 8 388 607 for ATM-base (2160 x 3840, padded 2176 x 3840 = 8 355 840, fits both).  The layers whose
 * operand image holds 2 GiB or more take the large-image form of their kernel, which addresses an image below 4 GiB; ATM's full-resolution
 * layers are Conv2d + per-channel PReLU, which the Winograd kernel (3x3 stride 1) and the direct kernel (3x3 stride 1 / 2, 1x1) have in
 * that form (docs/design/atm.md "4K" lists every buffer and kernel concerned). */
int vfi_atm_forward(vfi_atm_t* net, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, int global_motion, float* out_dev, void* stream);
/* Network.forward_global_ensemble (network_lite.py:599-704; network_base.py has the same code)["I_t"] for ONE pair: "On with Ensemble
 * (slowest)".  Frames and out_dev as vfi_atm_forward's.  The global branch (feature extractor, last_feat_extract, global fusion, two ATM blocks,
 * motion head) runs on the padded pair at scales 1, 1/2 and 1/4: level 0 is what "On" computes (the forward's own features are reused: the
 * reference recomputes them from the same input), levels 1 and 2 run on the x0.5 pyramid images the forward already has.  The three flow pairs
 * are scored (vfi_atm_alignment_loss), the winner is chosen and resized to the 1/16 map on the device (vfi_atm_select_flow), and the forward
 * continues as "On" does; the global-level I_t and mask, which the reference does not compute here either, are not made.  One C call, no
 * host synchronisation.  The shifted global block's mask follows the reference's cached one (vfi_atm_window_attention_labels).  Serves both
 * variants at every size "On" serves, 64x64 included (global maps of 4x4, 2x2 and 1x1 tokens).  The size limit is
 * vfi_atm_object_max_padded_pixels(net), as for "On": the ensemble adds no wider per-image buffer (its features are at most hid[0] <= 24
 * floats per pixel of the HALF-resolution image, its token buffers live on the 1/32 and 1/64 maps, the scoring writes one float per 256
 * pixels).  The workspace grows by those buffers (vfi_atm_workspace_bytes reports it). */
int vfi_atm_forward_ensemble(vfi_atm_t* net, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float* out_dev, void* stream);
int64_t vfi_atm_max_padded_pixels(void);
int64_t vfi_atm_object_max_padded_pixels(const vfi_atm_t* net);
/* the limit of a variant (0 = ATM-lite, 1 = ATM-base; 0 for any other) with large frames on; vfi_atm_object_max_padded_pixels follows the switch */
int64_t vfi_atm_large_max_padded_pixels(int variant);
/* on != 0: the object serves padded frames up to vfi_atm_large_max_padded_pixels(its variant), in all three global-motion modes; 0 (every
 * object as created): up to its limit above.  Changes no result at a size both serve. */
int vfi_atm_set_large_frames(vfi_atm_t* net, int on);
int vfi_atm_release_workspace(vfi_atm_t* net);
int64_t vfi_atm_workspace_bytes(const vfi_atm_t* net);

/* ---- XVFI (vfi_models/xvfi/xvfi_arch.py XVFInet, inference path): the kernels beside the layer objects ------------------------------------------ */

/* F.interpolate(x, scale_factor=1/l, mode='bicubic', align_corners=False) for l = 2, 4, 8, ... (VFInet.forward :156): at these ratios a fixed
 * separable 4-tap filter, taps -3/32, 19/32, 19/32, -3/32 over rows / columns l i + l / 2 - 2 .. l i + l / 2 + 1 clamped to the image.  in
 * [N,H,W,in_cs], a C-channel window; out [N,H/l,W/l,out_cs]; l must divide H and W.  (The reference computes this pyramid at every level and,
 * at inference, uses level 0 only, which is the frame itself: vfi_xvfi_forward does not call it.) */
int vfi_xvfi_bicubic_down(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, int l, void* stream);
/* VFInet.bwarp (:240-268): grid_sample(x, grid, bilinear, zeros, align_corners=True) at pixel + flow, the position taken through the
 * reference's normalise / grid_sample's un-normalise in fp32, times the gate that is 0 where the all-ones image sampled the same way is below
 * 0.999.  Image n of in / flow / out starts n * in_ns / flow_ns / out_ns floats behind image 0 (so the two directions of a pair may be channel
 * windows of one tensor); in_swap != 0 samples the partner image n ^ 1.  flow = [dx, dy].  A non-finite position gives 0. */
int vfi_xvfi_bwarp(const float* in_dev, int in_cs, int64_t in_ns, int in_swap, const float* flow_dev, int flow_cs, int64_t flow_ns, float* out_dev,
                   int out_cs, int64_t out_ns, int N, int H, int W, int C, void* stream);
/* Complementary Flow Reversal (:183-198): flow_dev [h,w,flow_cs] = (flow_01 xy, flow_10 xy), z_dev [h,w,z_cs] = the two importance logits;
 * out_dev [h,w,out_cs] = (flow_t0 xy, flow_t1 xy): both z_fwarp splats (:320-415: Gaussian corner weights around floor(t flow) resp.
 * floor((1 - t) flow), weighted by sigmoid(z) + 1e-5), the numerators of Eq. (1) / (2), norm_l and the division where norm_l > 0.
 * Deterministic: a gather per target cell, the contributing sources visited in row-major order, no floating-point atomics.  The search
 * window is the range of floor(t flow) over the sources that reach the image at all (one single-workgroup pass; scratch_dev >= 32 bytes), so
 * the cost is (range_y + 2) (range_x + 2) sources per cell and direction; a non-finite or out-of-image target contributes nothing. */
int vfi_xvfi_cfr(const float* flow_dev, int flow_cs, const float* z_dev, int z_cs, float t, float* out_dev, int out_cs, void* scratch_dev, int h, int w,
                 void* stream);
/* Level 0's RefineUNet input in one pass (:213-221), out_dev [scale h, scale w, out_cs]: channels 0 .. 256 / scale^2 = pixel_shuffle(cat(feat0,
 * feat1, warped0, warped1), scale) from feat_dev / warped_dev [2,h,w,.] (64 channels each), then frame 0, frame 1 (img_dev [2, scale h, scale w,
 * img_cs]), bwarp(frame 0, flow_t0), bwarp(frame 1, flow_t1), flow_t0, flow_t1 with flow_t* = scale * F.interpolate(flow_dev's channels 0..1 /
 * 2..3, scale_factor=scale, 'bilinear', align_corners=False).  scale 2 or 4. */
int vfi_xvfi_assemble(const float* feat_dev, int feat_cs, const float* warped_dev, int warped_cs, const float* flow_dev, int flow_cs, const float* img_dev,
                      int img_cs, float* out_dev, int out_cs, int h, int w, int scale, void* stream);
/* The occlusion blend plus residual (:222-226) and the node's crop: out [H,W,3] = ((1 - t) occ0 w0 + t occ1 w1) / ((1 - t) occ0 + t occ1) + res with
 * occ0 = sigmoid(refine[0]), occ1 = 1 - occ0, res = refine[1..3]; warped_dev = (w0 rgb | w1 rgb) per pixel of the padded Hp x Wp frame.  Not clamped. */
int vfi_xvfi_blend_out(const float* refine_dev, int refine_cs, const float* warped_dev, int warped_cs, float t, float* out_dev, int Hp, int Wp, int H, int W,
                       void* stream);

typedef struct vfi_xvfi vfi_xvfi_t;
/* The state_dict tensors of XVFInet in xvfi_spec.xvfi_shapes() order, aliased keys included (72 for module_scale_factor 2, 74 for 4; fp32 host
 * memory, copied); S_tst = the lowest scale level at inference.  Replaces XVFInet(args).load_state_dict (vfi_models/xvfi/__init__.py:25-37). */
vfi_xvfi_t* vfi_xvfi_create(const float* const* tensors, const int64_t* numels, int n_tensors, int scale, int S_tst);
void vfi_xvfi_destroy(vfi_xvfi_t* net);
/* model(I0, I1, t) of the node for ONE pair and one timestep (xvfi/__init__.py:39-46, :84-114; XVFInet.forward with is_training=False): frames
 * [H,W,C>=3] fp32 (not written) are zero-padded at the bottom / right to multiples of 2^S_tst * scale * 4, out_dev [H,W,3] is the cropped
 * result, not clamped.  The features of both frames at every level, the level flows and level 0's flow_l_tmp do not depend on t: they are
 * computed when the pair differs from the one the object holds (compared bit for bit on the device; one stream synchronisation) and kept while t
 * varies.  A frame whose padded size exceeds vfi_xvfi_max_padded_pixels() = (2^31 - 1) / 320 = 6 710 886 pixels is refused before any launch:
 * the widest per-image buffer (the RefineUNet's input at scale 2) has 80 floats per padded pixel and the layers index an image with 32 bits.
 * After vfi_xvfi_set_large_frames(net, 1) the limit of that object is vfi_xvfi_large_max_padded_pixels() = (2^32 - 1) / 320 = 13 421 772 pixels
 * (2160 x 3840 fits both configurations: 2160 x 3840 padded pixels for Vimeo, 2560 x 4096 for X4K; 3072 x 4608 does not): the layers whose
 * image holds 2 GiB or more take the large-image form of their kernel, which addresses an image below 4 GiB. */
int vfi_xvfi_forward(vfi_xvfi_t* net, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float t, float* out_dev, void* stream);
/* out_dev [Hp / scale, Wp / scale, 6] = level 0's flow_l_tmp (:177) of the pair the object holds */
int vfi_xvfi_level0_flow(vfi_xvfi_t* net, float* out_dev, void* stream);
int64_t vfi_xvfi_max_padded_pixels(void);
/* the limit with large frames on, and the limit vfi_xvfi_forward applies to this object (one of the two) */
int64_t vfi_xvfi_large_max_padded_pixels(void);
int64_t vfi_xvfi_object_max_padded_pixels(const vfi_xvfi_t* net);
/* on != 0: the object serves padded frames up to vfi_xvfi_large_max_padded_pixels(); 0 (every object as created): up to
 * vfi_xvfi_max_padded_pixels().  Changes no result at a size both serve. */
int vfi_xvfi_set_large_frames(vfi_xvfi_t* net, int on);
int vfi_xvfi_release_workspace(vfi_xvfi_t* net);
int64_t vfi_xvfi_workspace_bytes(const vfi_xvfi_t* net);

#ifdef __cplusplus
}
#endif
#endif /* VFI_HIP_H */
