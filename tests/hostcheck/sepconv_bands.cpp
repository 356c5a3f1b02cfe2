// Stand-alone check of the band arithmetic of SepConv++'s banded head stage (csrc/sepconv_bands.h, the header csrc/sepconv_net.hip plans
// its bands with).  Host code only, its own main, never loaded into Python.  Build and run:
//
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -Xarch_host -fsanitize=undefined,signed-integer-overflow -Xarch_host -fno-sanitize-recover=all \
//         tests/hostcheck/sepconv_bands.cpp -o tests/hostcheck/_build/sepconv_bands && tests/hostcheck/_build/sepconv_bands
//
// For a sweep of frame sizes (2x2, heights 8k +- 1 and +- 2, 2160x3840, 2x4194303 and the largest legal shapes) and EVERY legal band height
// of each it walks the bands and asserts: the bands tile the padded rows without gap or overlap (every output row in exactly one band);
// band origins are multiples of 8 (even, and whole output tiles); the halos are 4 / 2 rows clipped to the frame and even at their first
// row; with that halo the two stacked 3x3 layers, modelled as F(2x2, 3x3) tiles on the call's own even grid, give every kept row from real
// rows only; every band operand (x2 rows, x1, heads, planar) is below 2^31 - 1 bytes and fits the block the workspace gives it; and every
// quantity the kernels and launches keep in an int (the band's pixels, its first pixel inside the heads, grid sizes) is in range.  The
// sanitizer turns a signed overflow inside the header into a failure.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../comfyui-frame-interpolation_amd/csrc/sepconv_bands.h"

using namespace vfi::sepbands;

#define CHECK(c)                                                                                                          \
    do {                                                                                                                  \
        if (!(c)) {                                                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s (frame %dx%d, band height %d)\n", __FILE__, __LINE__, #c, g_H, g_W, g_bh); \
            std::exit(1);                                                                                                 \
        }                                                                                                                 \
    } while (0)

static int g_H = 0, g_W = 0, g_bh = 0;
static long g_frames = 0, g_plans = 0, g_bands = 0, g_rows = 0, g_refused = 0;

// a row of a 3x3 layer call over the rows [c0, c1) of a frame of Hp rows is the whole-frame call's iff the four input rows of its F(2x2, 3x3)
// tile, on the grid that starts at c0, are each inside the call and good there, or outside the FRAME (zero padding in both calls)
static bool tile_rows_good(int r, int c0, int c1, int Hp, int good0, int good1) {
    if ((c0 & 1) != 0) return false;      // another tile grid than the frame's
    const int t = r & ~1;
    for (int y = t - 1; y <= t + 2; ++y) {
        if (y < 0 || y >= Hp) continue;
        if (y < c0 || y >= c1 || y < good0 || y >= good1) return false;
    }
    return true;
}

static void walk_plan(int Hp, int Wp, int bh, bool every_row) {
    CHECK(band_rows_legal(Hp, Wp, bh));
    const int nb = band_count(Hp, bh);
    CHECK(nb >= 1);
    const int64_t x1_block = x1_band_floats(Hp, Wp, bh), heads_block = heads_band_floats(Hp, Wp, bh);
    CHECK(x1_block * 4 < kOperandBytes && heads_block * 4 < kOperandBytes);
    CHECK(planar_band_floats(Hp, Wp, bh) <= x1_block);      // the planar heads reuse x1's block
    int next = 0;
    for (int b = 0; b < nb; ++b) {
        const Band d = band_at(Hp, bh, b);
        CHECK(d.y0 == next && d.y1 > d.y0 && d.y1 <= Hp && d.y1 - d.y0 <= bh);      // no gap, no overlap
        next = d.y1;
        CHECK(d.y0 % kTileRows == 0 && d.y0 % 2 == 0);
        // halos: 4 and 2 rows, clipped to the frame
        CHECK(d.in0 == (d.y0 >= kHaloIn ? d.y0 - kHaloIn : 0) && d.in1 == (d.y1 + kHaloIn <= Hp ? d.y1 + kHaloIn : Hp));
        CHECK(d.mid0 == (d.y0 >= kHaloMid ? d.y0 - kHaloMid : 0) && d.mid1 == (d.y1 + kHaloMid <= Hp ? d.y1 + kHaloMid : Hp));
        CHECK(0 <= d.in0 && d.in0 <= d.mid0 && d.mid0 <= d.y0 && d.y1 <= d.mid1 && d.mid1 <= d.in1 && d.in1 <= Hp);
        CHECK(d.in0 % 2 == 0 && d.mid0 % 2 == 0);
        // the kept rows come from real rows through both layers: head1 over [in0, in1) of x2 (all real), the head2 layers over [mid0, mid1) of x1
        auto x1_good = [&](int r) { return tile_rows_good(r, d.in0, d.in1, Hp, 0, Hp); };
        int good0 = d.mid0, good1 = d.mid1;      // the good x1 rows among those the head2 layers read
        while (good0 < good1 && !x1_good(good0)) ++good0;
        while (good1 > good0 && !x1_good(good1 - 1)) --good1;
        CHECK(good0 == d.mid0 && good1 == d.mid1);       // head2 reads no wrong x1 row at all
        if (every_row) {
            for (int r = d.y0; r < d.y1; ++r) CHECK(tile_rows_good(r, d.mid0, d.mid1, Hp, good0, good1));
            g_rows += d.y1 - d.y0;
        } else {
            const int probe[4] = {d.y0, d.y0 + 1 < d.y1 ? d.y0 + 1 : d.y0, d.y1 - 2 >= d.y0 ? d.y1 - 2 : d.y0, d.y1 - 1};
            for (int r : probe) CHECK(tile_rows_good(r, d.mid0, d.mid1, Hp, good0, good1));
        }
        // operands of the band's launches
        const int64_t in_rows = d.in1 - d.in0, mid_rows = d.mid1 - d.mid0, out_rows_ = d.y1 - d.y0;
        CHECK(in_rows * Wp * kX2C * 4 < kOperandBytes);                                  // head1's input
        CHECK(in_rows * Wp * kX1C <= x1_block && in_rows * Wp * kX1C * 4 < kOperandBytes);      // x1
        CHECK(mid_rows * Wp * kHeadC <= heads_block);                                    // heads
        CHECK(out_rows_ * Wp * kPlanes <= x1_block);                                     // planar heads
        // offsets into the whole-frame x2 and the band's x1 / heads: 64-bit, inside their tensors
        const int64_t x2_off = (int64_t)d.in0 * Wp * kX2C, x2_end = x2_off + in_rows * Wp * kX2C;
        CHECK(x2_off >= 0 && x2_end <= (int64_t)Hp * Wp * kX2C);
        const int64_t x1_off = (int64_t)(d.mid0 - d.in0) * Wp * kX1C;
        CHECK(x1_off >= 0 && x1_off + mid_rows * Wp * kX1C <= in_rows * Wp * kX1C);
        const int64_t pin = (int64_t)(d.y0 - d.mid0) * Wp, Pb = out_rows_ * Wp;
        CHECK(pin >= 0 && pin + Pb <= mid_rows * Wp);
        // what the kernels keep in an int, and the launch grids
        CHECK(Pb <= INT_MAX && pin <= INT_MAX && (Pb + 63) / 64 <= 0x7fffffffLL);
        CHECK((out_rows_ + kTileRows - 1) / kTileRows <= 65535);
        ++g_bands;
    }
    CHECK(next == Hp);
    ++g_plans;
}

// every legal band height of an H x W frame; returns false where the banded form refuses the frame
static bool walk_frame(int H, int W) {
    g_H = H, g_W = W, g_bh = 0;
    ++g_frames;
    const int64_t Hp64 = (int64_t)H + H % 2, Wp64 = (int64_t)W + W % 2;
    CHECK(Hp64 <= INT_MAX && Wp64 <= INT_MAX);
    const int Hp = (int)Hp64, Wp = (int)Wp64;
    if (Hp64 * Wp64 > kLargeMaxPixels || widest_whole_bytes(Hp, Wp) >= kOperandBytes) {
        ++g_refused;
        return false;
    }
    const int top = max_band_rows(Hp, Wp);
    CHECK(top % kTileRows == 0 && top >= 0);
    if (top == 0) {      // too wide: not even 8 rows with their halo
        CHECK(!band_rows_legal(Hp, Wp, kTileRows) && (int64_t)(kTileRows + 2 * kHaloIn) * Wp > kBandMaxPixels);
        ++g_refused;
        return false;
    }
    CHECK(band_rows_legal(Hp, Wp, top));
    // the next multiple of 8 is illegal, or taller than the frame (then it is the same single band)
    CHECK(!band_rows_legal(Hp, Wp, top + kTileRows) || top >= Hp || top == kMaxBandRows);
    const int dflt = default_band_rows(Hp, Wp);
    CHECK(band_rows_legal(Hp, Wp, dflt) && dflt <= kDefaultBandRows);
    const bool every_row = (int64_t)Hp * (top / kTileRows) <= 4000000;
    for (int bh = kTileRows; bh <= top; bh += kTileRows) {
        g_bh = bh;
        walk_plan(Hp, Wp, bh, every_row);
    }
    return true;
}

int main() {
    static_assert(kWholeMaxPixels == 2097151 && kMaxPixels == 4194303 && kLargeMaxPixels == 8388607, "the limits of include/vfi_hip.h");
    static_assert(kWholeMaxPixels * kX1C * 4 < kOperandBytes && (kWholeMaxPixels + 1) * kX1C * 4 >= kOperandBytes, "x1 below 2 GiB");
    static_assert(kLargeMaxPixels * kX2C * 4 < kOperandBytes && (kLargeMaxPixels + 1) * kX2C * 4 >= kOperandBytes, "x2 below 2 GiB");
    CHECK(walk_frame(2, 2) && walk_frame(1, 1));
    for (int k = 1; k <= 6; ++k)
        for (int dlt = -2; dlt <= 2; ++dlt)
            for (int W : {2, 40, 179}) CHECK(walk_frame(8 * k + dlt, W));
    for (int H : {24, 25, 26, 64, 90, 101}) CHECK(walk_frame(H, 96));
    CHECK(walk_frame(1080, 1920) && walk_frame(1440, 2560));
    CHECK(walk_frame(2160, 3840) && max_band_rows(2160, 3840) == 536 && default_band_rows(2160, 3840) == kDefaultBandRows);
    CHECK(walk_frame(2160, 3842));                                   // 8 298 720 pixels
    CHECK(!walk_frame(2898, 2896));                                  // 8 392 608: over the limit
    CHECK(!walk_frame(2, 4194303));                                  // pads to 2 x 4 194 304: one pixel over the limit
    CHECK(!walk_frame(2, 4194302));                                  // inside the limit, but no band of it fits: too wide
    CHECK(!walk_frame(16, 131072 + 2));                              // 16 rows of 131 074 columns: too wide as well
    CHECK(walk_frame(64, 131070));                                   // the widest frame that has a band: 8 rows only
    CHECK(max_band_rows(64, 131070) == 8);
    CHECK(walk_frame(2896, 2896) && walk_frame(2046, 4095) && walk_frame(4095, 2046));      // the largest near-square and 2:1 shapes
    CHECK(walk_frame(131056, 64));                                   // tall and narrow, sides multiples of 16: 8 387 584 pixels
    CHECK(walk_frame(524286, 16) && !walk_frame(524288, 16));        // 8 388 576 pixels; two rows more are 8 388 608, one over the limit
    CHECK(!walk_frame(4194302, 2));                                  // an odd coarse level up-sampled past 2 GiB: refused by the exact tensor check
    std::printf("sepconv_bands: ok (%ld frames, %ld refused, %ld plans, %ld bands, %ld rows walked one by one)\n", g_frames, g_refused, g_plans, g_bands,
                g_rows);
    return 0;
}
