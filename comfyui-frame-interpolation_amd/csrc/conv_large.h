// Address arithmetic of the LARGE kernel forms (conv_mfma2.hip, conv_wino.hip), shared by device code, launchers and the stand-alone
// host check (tests/hostcheck/conv_large_addr.cpp, built with the undefined-behaviour sanitizer).
//
// A LARGE launch never forms a byte offset from an image's start.  Each tile (direct kernel) or region (Winograd kernel) gets a buffer
// descriptor of its own: a 64-bit base at the first row it touches, a size of the rows it spans; every per-lane offset counts from that
// row.  What has to fit in 32 bits is therefore
//   * the floats of one image (the kernels keep Hin * Win * in_cs in an int and index images with it): <= kConvHugeMaxFloats, and
//   * the bytes of the rows one tile / region spans, which double as the range the descriptor checks: < 2^31, so that the "outside"
//     offset 0x80000000 is out of range and reads as zero.
// Below 4 GiB per image a layer object takes this form on its own (2 GiB mark: option large_image_bytes); from 4 GiB on only with the
// object's permission (vfi_conv_allow_huge), up to kConvHugeMaxFloats floats = 8 GiB - 4 bytes per operand image.
#pragma once
#include <cstddef>
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace vfi {

constexpr long kConvHugeMaxFloats = 0x7fffffffL;      // floats of one operand image with the permission (bound of the audited arithmetic)
constexpr long kConvLargeMaxBytes = 0xffffffffL;      // bytes of one operand image without it

// first row of a descriptor whose tile / patch starts at row `first` (negative: the halo above the image)
__host__ __device__ inline int large_row0(int first) { return first > 0 ? first : 0; }
// rows the descriptor spans: `span` rows from r0, cut at the image's end
__host__ __device__ inline int large_rows(int H, int r0, int span) { return H - r0 < span ? H - r0 : span; }
// floats from the operand's pointer to the descriptor's base: image n (img_floats each), row r0 of W pixels of cs floats
__host__ __device__ inline size_t large_base_floats(int n, int img_floats, int r0, int W, int cs) {
    return (size_t)n * img_floats + (size_t)r0 * W * cs;
}
// ... the same for an operand indexed by rows (the Winograd epilogue's output and residual): row n * H + r0
__host__ __device__ inline size_t large_row_base_floats(int n, int H, int r0, int W, int cs) { return ((size_t)n * H + r0) * W * cs; }
// bytes the descriptor spans (its num_records): int arithmetic, the launchers refuse a layer whose widest span reaches 2^31
__host__ __device__ inline int large_span_bytes(int rows, int W, int cs) { return rows * W * cs * 4; }
// byte offset of float `f` of pixel (iy, ix) from the descriptor's base: pixels are pstr floats apart
__host__ __device__ inline int large_lane_bytes(int iy, int r0, int W, int ix, int pstr, int f) { return (((iy - r0) * W + ix) * pstr + f) * 4; }

// ---- the transposed convolution's interleaved store (conv_wino.hip: SHUF 2 in its LARGE form) ----
// A region of RH input rows from oy0 writes the output rows [2 oy0, 2 oy0 + 2 RH) of the [2H, 2W] image of cs-float pixels; its descriptor
// starts at output row 2 oy0 of image n and spans those rows, cut at the image's end.
__host__ __device__ inline int large_deconv_rows(int H, int oy0, int RH) { return large_rows(2 * H, 2 * oy0, 2 * RH); }
__host__ __device__ inline size_t large_deconv_base_floats(int n, int H, int oy0, int W, int cs) { return large_row_base_floats(n, 2 * H, 2 * oy0, 2 * W, cs); }
__host__ __device__ inline int large_deconv_span_bytes(int rows, int W, int cs) { return large_span_bytes(rows, 2 * W, cs); }
// byte offsets from that base.  Lane part: parity g = 2 py + px of the lane's channel group, channel cg of out_cs, the lane's first input column
__host__ __device__ inline int large_deconv_lane_bytes(int g, int xlane, int W, int cs, int cg) { return (((g >> 1) * 2 * W + (g & 1) + 2 * xlane) * cs + cg) * 4; }
// ... per-store part: input row oyr of the region (two output rows each), input column xq from the lane's first
__host__ __device__ inline int large_deconv_store_bytes(int oyr, int xq, int W, int cs) { return oyr * 4 * W * cs * 4 + 2 * xq * cs * 4; }

// Host side: may one operand image of H x W pixels of cs floats be served?  huge = the layer object's permission.
inline bool large_image_ok(int H, int W, int cs, bool huge) {
    const long floats = (long)H * W * cs;
    return huge ? floats <= kConvHugeMaxFloats : floats * 4 <= kConvLargeMaxBytes;
}
// ... and do the `span` rows of one tile / region stay below the descriptor's 2^31 bytes?
inline bool large_span_ok(int span, int W, int cs) { return (long)span * W * cs * 4 < 0x7fffffffL; }

}  // namespace vfi
