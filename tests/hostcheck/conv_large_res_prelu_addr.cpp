// Stand-alone check of the address arithmetic of the LARGE form of Conv2d 3x3 stride 1 + residual + per-channel PReLU (csrc/conv_large.h as
// conv_wino.hip's MODE 13 and conv_mfma2.hip's 3x3 stride-1 tiles use it).  Host code only, its own main, never loaded into Python; a
// companion of conv_large_addr.cpp, which covers the 16x8 region's input and output descriptors on FILM's layers.  Build and run:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -Xarch_host -fsanitize=undefined,signed-integer-overflow -Xarch_host -fno-sanitize-recover=all \
//         tests/hostcheck/conv_large_res_prelu_addr.cpp -o tests/hostcheck/_build/conv_large_res_prelu_addr && tests/hostcheck/_build/conv_large_res_prelu_addr
//
// What this form adds: a third descriptor per Winograd region, the residual's, formed like the output's with its own pixel stride, and the
// 32x4 region shape (4 output rows, a 6-row patch, 32 columns).  For every region of both shapes it walks the helper calls the device code
// makes and asserts: base + span stays inside the image, every live offset stays inside the span and below 2^31, the "outside" offset
// 0x80000000 is out of range of every span.  It is a walk of the conv_large.h helpers: bases, spans and the input's lane offsets come from
// them; the epilogue's row and lane offsets have no helper (wino_epilogue forms them in place) and are restated here by hand, so a change
// of the kernel's expression is caught by the GPU tests (tests/test_gpu_conv_large_res_prelu.py), not by this program.
// The direct kernel rebases its input only (its epilogue forms 64-bit addresses): its 16x16 and 16x8 tiles are walked on the same inputs.  Cases: AMT-G's rb[4] (x3 of 352 floats -> r5 of 256 + r0 of 256, 252 channels) at
// 2160x3840's half resolution, at 2816x4320's (next to the object's limit of 12 201 611 padded pixels, the input just below 4 GiB), and a
// residual wider than the output at an odd size.  The sanitizer turns any signed overflow inside the helpers into a failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../comfyui-frame-interpolation_amd/csrc/conv_large.h"

using namespace vfi;

#define CHECK(c)                                                                              \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);        \
            std::exit(1);                                                                     \
        }                                                                                     \
    } while (0)

static long g_descriptors = 0;

// an input descriptor: rows [first, first + span) of an H x W x cs image (first may be -1: the halo above), columns [x0 - 1, x0 + cols]
static void check_input(int H, int W, int cs, int first, int span, int x0, int cols, int win_floats) {
    const int64_t img_floats64 = (int64_t)H * W * cs;
    CHECK(img_floats64 <= kConvHugeMaxFloats);
    const int img_floats = (int)img_floats64;      // what the kernels keep
    const int r0 = large_row0(first), rows = large_rows(H, r0, span);      // as make_rsrc / make_arsrc form them
    CHECK(r0 >= 0 && rows >= 1 && r0 + rows <= H);
    const size_t base = large_base_floats(0, img_floats, r0, W, cs);
    const int bytes = large_span_bytes(rows, W, cs);
    CHECK(bytes > 0 && (uint32_t)bytes < 0x80000000u);                                  // the outside offset is out of range
    CHECK((int64_t)base * 4 + bytes <= img_floats64 * 4);                               // base + span inside the image
    CHECK(base == (size_t)((int64_t)r0 * W * cs));
    const int xs[2] = {x0 - 1 < 0 ? 0 : x0 - 1, x0 + cols < W ? x0 + cols : W - 1};
    const int ys[2] = {r0, r0 + rows - 1};
    for (int y : ys)
        for (int x : xs)
            for (int f : {0, win_floats - 4}) {
                const int off = large_lane_bytes(y, r0, W, x, cs, f);
                CHECK(off >= 0 && (int64_t)off + 16 <= bytes);
            }
    ++g_descriptors;
}

// one epilogue descriptor of a Winograd region (output or residual): rows [Ry0, Ry0 + RH) of an H x W image of cs-float pixels, the
// region's columns [Rx0, Rx0 + RW), `chans` channels stored / read per pixel
static void check_region_rows(int H, int W, int cs, int chans, int Ry0, int Rx0, int RH, int RW) {
    const int lrows = large_rows(H, Ry0, RH);
    CHECK(lrows >= 1 && Ry0 + lrows <= H);
    const int ob = large_span_bytes(lrows, W, cs);
    CHECK(ob > 0 && (uint32_t)ob < 0x80000000u);
    CHECK((int64_t)large_row_base_floats(0, H, Ry0, W, cs) * 4 + ob <= (int64_t)H * W * cs * 4);
    CHECK(large_row_base_floats(1, H, Ry0, W, cs) == (size_t)((int64_t)(H + Ry0) * W * cs));      // image 1 of a batch: rows n * H + r0
    const int xl = Rx0 + RW - 1 < W ? Rx0 + RW - 1 : W - 1;
    // the epilogue's offset of the region's last live value: row part + lane part (wino_epilogue: rowo / rowr, lane_o / lane_r, xq)
    const int64_t last = (int64_t)(lrows - 1) * W * cs * 4 + ((int64_t)xl * cs + chans - 1) * 4;
    CHECK(last >= 0 && last + 4 <= ob);
    ++g_descriptors;
}

// every region of both shapes and every direct tile of the layer: input H x W x in_cs (window win_floats), output out_cs, residual res_cs
static void walk_layer(const char* what, int H, int W, int in_cs, int win_floats, int out_cs, int res_cs, int chans, bool huge) {
    CHECK(large_image_ok(H, W, in_cs, huge) && large_image_ok(H, W, out_cs, huge) && large_image_ok(H, W, res_cs, huge));
    const long before = g_descriptors;
    const int shapes[2][2] = {{8, 16}, {4, 32}};      // RH x RW: 16x8 regions (RTX 8), 32x4 regions (RTX 16); patch RH + 2 rows
    for (const auto& r : shapes) {
        CHECK(large_span_ok(r[0] + 2, W, in_cs) && large_span_ok(r[0], W, out_cs) && large_span_ok(r[0], W, res_cs));
        for (int Ry0 = 0; Ry0 < H; Ry0 += r[0])
            for (int Rx0 = 0; Rx0 < W; Rx0 += r[1]) {
                check_input(H, W, in_cs, Ry0 - 1, r[0] + 2, Rx0, r[1], win_floats);
                check_region_rows(H, W, out_cs, chans, Ry0, Rx0, r[0], r[1]);
                check_region_rows(H, W, res_cs, chans, Ry0, Rx0, r[0], r[1]);
            }
    }
    const int tiles[2][2] = {{16, 16}, {8, 16}};      // direct kernel: THO x TWO (halo THO + 2 rows)
    for (const auto& t : tiles) {
        CHECK(large_span_ok(t[0] + 2, W, in_cs));
        for (int Y0 = 0; Y0 < H; Y0 += t[0])
            for (int X0 = 0; X0 < W; X0 += t[1]) check_input(H, W, in_cs, Y0 - 1, t[0] + 2, X0, t[1], win_floats);
    }
    std::printf("%-44s %5d x %5d x %4d floats = %11lld bytes: %ld descriptors\n", what, H, W, in_cs, (long long)H * W * in_cs * 4, g_descriptors - before);
}

int main() {
    walk_layer("AMT-G rb[4] at 1080 x 1920", 1080, 1920, 352, 352, 256, 256, 252, false);
    CHECK((int64_t)2816 * 4320 <= 12201611 && (int64_t)1408 * 2160 * 352 * 4 <= kConvLargeMaxBytes && (int64_t)1416 * 2160 * 352 * 4 > kConvLargeMaxBytes);
    walk_layer("AMT-G rb[4] at 1408 x 2160", 1408, 2160, 352, 352, 256, 256, 252, false);
    walk_layer("res_cs > out_cs, odd size: 1083 x 1925", 1083, 1925, 352, 352, 256, 264, 252, false);
    // the first half-resolution map over the object's limit is over the 4 GiB bound of the form without vfi_conv_allow_huge
    CHECK(!large_image_ok(1416, 2160, 352, false));
    std::printf("conv_large_res_prelu_addr: ok, %ld descriptors checked\n", g_descriptors);
    return 0;
}
