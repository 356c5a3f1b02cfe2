// Stand-alone check of the address arithmetic the LARGE kernel forms share with their launchers (csrc/conv_large.h).  Host code only, its
// own main, never loaded into Python.  Build and run (docs/design/film.md, "Address check"):
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -Xarch_host -fsanitize=undefined,signed-integer-overflow -Xarch_host -fno-sanitize-recover=all \
//         tests/hostcheck/conv_large_addr.cpp -o tests/hostcheck/_build/conv_large_addr && tests/hostcheck/_build/conv_large_addr
//
// For every tile of the direct kernel (the tile shapes conv_pick_variant can give a 3x3 stride-1 layer: 16x16, 16x8, with their 18- and
// 10-row halos) and every region of the Winograd kernel (16x8 outputs, 10-row patch; its output descriptor of 8 rows) it walks the helper
// calls the device code makes and asserts: base + span stays inside the image, every live per-lane offset stays inside the span and below
// 2^31, the "outside" offset 0x80000000 is out of range of every span.  Cases: FILM's three layers at 2160x3840 whose operand is over
// 4 GiB, an image at the stated bound (2^31 - 1 floats), and one just over it, which the host guard must refuse.  The sanitizer turns any
// signed overflow inside the helpers into a failure.
#include <cassert>
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

// one descriptor: rows [first, first + span) of an H x W x cs image (first may be -1: the halo above), columns [x0 - 1, x0 + cols]
static void check_descriptor(int H, int W, int cs, int first, int span, int x0, int cols, int win_floats) {
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
    CHECK(large_row_base_floats(0, H, r0, W, cs) == base);
    // the extreme live lanes: first / last row of the span, first / last column of the tile inside the image, last 16-byte piece of the window
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

// every tile / region of a 3x3 stride-1 layer on an H x W x cs input whose window holds win_floats floats, output cs out_cs
static void walk_layer(const char* what, int H, int W, int cs, int win_floats, int out_cs) {
    CHECK(large_image_ok(H, W, cs, true) && large_image_ok(H, W, out_cs, true));
    const long before = g_descriptors;
    const int tiles[2][2] = {{16, 16}, {8, 16}};      // direct kernel: THO x TWO (halo THO + 2 rows)
    for (const auto& t : tiles) {
        CHECK(large_span_ok(t[0] + 2, W, cs));
        for (int Y0 = 0; Y0 < H; Y0 += t[0])
            for (int X0 = 0; X0 < W; X0 += t[1]) check_descriptor(H, W, cs, Y0 - 1, t[0] + 2, X0, t[1], win_floats);
    }
    CHECK(large_span_ok(10, W, cs) && large_span_ok(10, W, out_cs));
    for (int Ry0 = 0; Ry0 < H; Ry0 += 8)
        for (int Rx0 = 0; Rx0 < W; Rx0 += 16) {
            check_descriptor(H, W, cs, Ry0 - 1, 10, Rx0, 16, win_floats);      // Winograd input patch
            // Winograd output region: rows [Ry0, Ry0 + 8), offsets row * W * out_cs * 4 + lane part
            const int lrows = large_rows(H, Ry0, 8);
            const int ob = large_span_bytes(lrows, W, out_cs);
            CHECK(ob > 0 && (uint32_t)ob < 0x80000000u);
            CHECK((int64_t)large_row_base_floats(0, H, Ry0, W, out_cs) * 4 + ob <= (int64_t)H * W * out_cs * 4);
            const int xl = Rx0 + 15 < W ? Rx0 + 15 : W - 1;
            CHECK((int64_t)(lrows - 1) * W * out_cs * 4 + ((int64_t)xl * out_cs + out_cs - 1) * 4 + 4 <= ob);
        }
    std::printf("%-44s %5d x %5d x %4d floats = %11lld bytes: %ld descriptors\n", what, H, W, cs, (long long)H * W * cs * 4, g_descriptors - before);
}

int main() {
    // FILM at 2160x3840: pred[0][0] reads [4, 132) of tw[k][0]; fuse[3][1] reads al[0] through its channel map; fuse[2][1] reads al[1]
    walk_layer("FILM pred[0][0]: window 128 at 4 of 132", 2160, 3840, 132, 128, 32);
    walk_layer("FILM fuse[3][1]: 204 -> 64 on 208", 2160, 3840, 208, 208, 64);
    walk_layer("FILM fuse[2][1]: 528 on 1080 x 1920", 1080, 1920, 528, 528, 128);
    walk_layer("the issue's 2160 x 4096 with 208 floats", 2160, 4096, 208, 208, 64);
    // at the bound: the largest H x 4096 x 208 image within 2^31 - 1 floats is H = 2520 (2 146 959 360 floats)
    CHECK((int64_t)2520 * 4096 * 208 <= kConvHugeMaxFloats && (int64_t)2521 * 4096 * 208 > kConvHugeMaxFloats);
    walk_layer("at the bound: 2520 x 4096 x 208", 2520, 4096, 208, 208, 64);
    // ... and the guard alone at the last image within the bound and the first over it (one row of 4-float pixels)
    CHECK(large_image_ok(1, 0x7fffffff / 4, 4, true) && !large_image_ok(1, 0x7fffffff / 4 + 1, 4, true));
    // just over: refused by the host guard with and without the permission; 4 GiB itself needs the permission
    CHECK(!large_image_ok(2521, 4096, 208, true) && !large_image_ok(2521, 4096, 208, false));
    CHECK(!large_image_ok(2176, 4800, 208, true));
    CHECK(large_image_ok(2160, 3840, 208, true) && !large_image_ok(2160, 3840, 208, false));
    CHECK(large_image_ok(2560, 4096, 100, false) && !large_image_ok(2560, 4096, 104, false) && large_image_ok(2560, 4096, 104, true));
    // a row span at or over 2^31 bytes is refused whatever the image
    CHECK(!large_span_ok(18, 1 << 20, 32) && large_span_ok(18, 4096, 528));
    std::printf("conv_large_addr: ok, %ld descriptors checked\n", g_descriptors);
    return 0;
}
