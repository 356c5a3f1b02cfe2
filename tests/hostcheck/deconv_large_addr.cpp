// Stand-alone check of the address arithmetic of the transposed convolution's LARGE form (conv_wino_kernel<8, 0, 2, 0, LARGE>): the
// store-side helpers of csrc/conv_large.h (large_deconv_*) and the input side's per-region rebase.  Host code only, its own main, never
// loaded into Python.  Build and run:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -Xarch_host -fsanitize=undefined,signed-integer-overflow -Xarch_host -fno-sanitize-recover=all \
//         tests/hostcheck/deconv_large_addr.cpp -o tests/hostcheck/_build/deconv_large_addr && tests/hostcheck/_build/deconv_large_addr
//
// For every 16x8 region of FLAVR's two transposed layers at 2160x3840 (docs/design/flavr.md "4K"), and of a layer whose output sits at the
// bound of 2^31 - 1 floats, it walks the helper calls the epilogue makes for every parity group, both lane halves, every tile row and
// column step, and asserts: the descriptor's base + span stays inside the output image, every live offset stays inside the span, base +
// offset IS the address of output pixel (2 oy + py, 2 ox + px), channel cg, and the "outside" offset 0x80000000 is out of range.  The
// sanitizer turns any signed overflow inside the helpers into a failure.
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

static long g_regions = 0, g_stores = 0;

constexpr int RW = 16, RH = 8, PH = RH + 2;      // WinoGeom<8>: a region's input pixels and its patch rows

// H x W input pixels of in_cs floats (the window holds win floats), LO output channels at out_off of an out_cs-float pixel, N images
static void walk_layer(const char* what, int N, int H, int W, int in_cs, int win, int LO, int out_cs, bool huge) {
    CHECK(large_image_ok(H, W, in_cs, huge) && large_image_ok(2 * H, 2 * W, out_cs, huge));
    CHECK(large_span_ok(PH, W, in_cs) && large_span_ok(2 * RH, 2 * W, out_cs));      // conv_wino_launch's guards
    const int64_t in_img = (int64_t)H * W * in_cs, out_img = (int64_t)4 * H * W * out_cs;
    const int img_floats = (int)in_img;      // what the kernel keeps
    const long before = g_regions;
    for (int n = 0; n < N; ++n)
        for (int Ry0 = 0; Ry0 < H; Ry0 += RH)
            for (int Rx0 = 0; Rx0 < W; Rx0 += RW) {
                // input patch: rows [Ry0 - 1, Ry0 + RH], columns [Rx0 - 1, Rx0 + RW]
                const int r0 = large_row0(Ry0 - 1), rows = large_rows(H, r0, PH);
                CHECK(r0 >= 0 && rows >= 1 && r0 + rows <= H);
                const size_t ibase = large_base_floats(n, img_floats, r0, W, in_cs);
                const int ibytes = large_span_bytes(rows, W, in_cs);
                CHECK(ibytes > 0 && (uint32_t)ibytes < 0x80000000u);
                CHECK(ibase == (size_t)(n * in_img + (int64_t)r0 * W * in_cs) && (int64_t)ibase + ibytes / 4 <= (n + 1) * in_img);
                const int xs[2] = {Rx0 - 1 < 0 ? 0 : Rx0 - 1, Rx0 + RW < W ? Rx0 + RW : W - 1};
                for (int y : {r0, r0 + rows - 1})
                    for (int x : xs)
                        for (int f : {0, win - 4}) {
                            const int off = large_lane_bytes(y, r0, W, x, in_cs, f);
                            CHECK(off >= 0 && (int64_t)off + 16 <= ibytes);
                        }
                // output: rows [2 Ry0, 2 Ry0 + 2 RH) of [2H, 2W]
                const int lrows = large_deconv_rows(H, Ry0, RH);
                CHECK(lrows >= 2 && lrows <= 2 * RH && 2 * Ry0 + lrows <= 2 * H);
                const size_t obase = large_deconv_base_floats(n, H, Ry0, W, out_cs);
                const int obytes = large_deconv_span_bytes(lrows, W, out_cs);
                CHECK(obytes > 0 && (uint32_t)obytes < 0x80000000u);
                CHECK((int64_t)obase + obytes / 4 <= (n + 1) * out_img && (int64_t)obase >= n * out_img);
                for (int half = 0; half < 2; ++half) {
                    const int xlane = Rx0 + 8 * half;
                    for (int g = 0; g < 4; ++g)
                        for (int cg : {0, LO - 1}) {
                            const int lane = large_deconv_lane_bytes(g, xlane, W, out_cs, cg);
                            CHECK(lane >= 0);
                            for (int oyr = 0; oyr < RH && Ry0 + oyr < H; ++oyr)
                                for (int xq = 0; xq < 8; ++xq) {
                                    if (xlane + xq >= W) continue;      // the epilogue's `ok`: such a store gets the outside offset
                                    const int st = large_deconv_store_bytes(oyr, xq, W, out_cs);
                                    const int64_t off = (int64_t)lane + st;
                                    CHECK(st >= 0 && off + 4 <= obytes);
                                    const int64_t want = n * out_img + (((int64_t)(2 * (Ry0 + oyr) + (g >> 1)) * 2 * W + 2 * (xlane + xq) + (g & 1)) * out_cs + cg);
                                    CHECK((int64_t)obase * 4 + off == want * 4);
                                    ++g_stores;
                                }
                        }
                }
                ++g_regions;
            }
    std::printf("%-52s in %11lld bytes, out %11lld bytes: %ld regions\n", what, (long long)in_img * 4, (long long)out_img * 4, g_regions - before);
}

int main() {
    // FLAVR at 2160x3840 (padded the same): dec[2] reads the window of 768 of cat[2]'s [6, 256] pixel at 540x960 and writes 64 channels of
    // e2[1]'s [6, 64] pixel at 1080x1920; dec[4] reads 384 of cat[0]'s [6, 128] pixel at 1080x1920 and writes 64 of fin's [4, 64] at 2160x3840
    walk_layer("FLAVR dec[2]: 768 of 1536 -> 64 of 384", 1, 540, 960, 1536, 768, 64, 384, false);
    walk_layer("FLAVR dec[4]: 384 of 768 -> 64 of 256", 1, 1080, 1920, 768, 384, 64, 256, true);
    CHECK(!large_image_ok(2160, 3840, 256, false) && !large_image_ok(1080, 1920, 768, false));      // dec[4] needs the permission
    // at FLAVR's large limit: 4 * 889 * 2359 = 8 388 604 padded pixels, the last multiple of 4 within 8 388 607 (2 147 482 624 floats of fin)
    CHECK((int64_t)4 * 889 * 2359 * 256 <= kConvHugeMaxFloats && (int64_t)8388607 * 256 <= kConvHugeMaxFloats && (int64_t)8388608 * 256 > kConvHugeMaxFloats);
    walk_layer("at the limit: 889 x 2359, 384 of 768 -> 64 of 256", 1, 889, 2359, 768, 384, 64, 256, true);
    // two images and partial regions, small
    walk_layer("two images, 131 x 133, 16 of 28 -> 24 of 384", 2, 131, 133, 28, 16, 24, 384, false);
    // 2176 x 3856 is over the limit: the host guard refuses fin with and without the permission
    CHECK(!large_image_ok(2176, 3856, 256, true) && !large_image_ok(2176, 3856, 256, false));
    std::printf("deconv_large_addr: ok, %ld regions, %ld stores checked\n", g_regions, g_stores);
    return 0;
}
