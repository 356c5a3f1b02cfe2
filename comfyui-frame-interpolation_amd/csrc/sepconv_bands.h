// SepConv++ head stage in horizontal bands: the size limits of the net object and the band arithmetic of csrc/sepconv_net.hip, in plain
// C++ so that the host check tests/hostcheck/sepconv_bands.cpp runs the same code (docs/design/sepconv.md "4K").
//
// The head stage is up2(row1) = x2 [Hp, Wp, 64] -> head1 (3x3, 64 -> 256, per-channel PReLU) = x1 -> four head2 (3x3, 64 -> 51) = heads
// [., ., 208] -> planar [204][pixels] -> the output stage.  Band b owns the output rows [y0, y1) = [b * bh, min((b + 1) * bh, Hp)).
//
// Halo.  Both 3x3 layers run as Winograd F(2x2, 3x3) wherever the launch has enough work: the rows (2t, 2t + 1) of a layer call's output
// come from the rows 2t - 1 .. 2t + 2 of its input, counted from the first row the call was given, and have the whole-frame call's bits
// only if the call's tile grid is the frame's (an even first row) and all four rows are the real ones (the transform's terms that cancel
// in exact arithmetic do not cancel bit-exactly against a zero row).  With y0 even:
//   heads rows [y0, y1)       read x1 rows [y0 - 1, y1 + 1);
//   x1 rows y0 - 1 and y1     sit in the tiles (y0 - 2, y0 - 1) and (y1, y1 + 1), which read x2 rows [y0 - 3, y1 + 3);
//   an even first row         makes that head1 on the x2 rows [y0 - 4, y1 + 4) — its first and last tile read one zero row and are wrong,
//                             the x1 rows [y0 - 2, y1 + 2) are the frame's — and head2 on exactly those x1 rows, whose first and last
//                             output tile are wrong in turn and [y0, y1) are the frame's.
// So 4 real x2 rows above and below the band (kHaloIn) and 2 x1 rows (kHaloMid), each clipped to the frame: at the frame's own top and
// bottom the layers' zero padding applies as it does in the whole-frame call.  The direct kernel (small launches) sums per output pixel
// and needs one real row per layer, which the same halo covers.
#pragma once
#include <cstdint>

namespace vfi {
namespace sepbands {

constexpr int kTileRows = 8;        // rows of the output stage's 64 x 8 tile: band heights are multiples of it, so a band's tiles are the frame's
constexpr int kHaloIn = 4;          // x2 rows above / below the band that head1 reads
constexpr int kHaloMid = 2;         // x1 rows above / below the band that the head2 layers read
constexpr int kX2C = 64;            // up2(row1)
constexpr int kX1C = 256;           // head1's output
constexpr int kHeadC = 208;         // heads, NHWC: 4 x 52
constexpr int kPlanes = 204;        // heads, planar: 4 x 51
constexpr int64_t kOperandBytes = 0x7fffffffLL;      // a plain layer form serves operand images BELOW this (include/vfi_hip.h: vfi_conv_allow_huge)

// whole-frame form on plain layer forms only: x1 = [Hp, Wp, 256] below 2 GiB
constexpr int64_t kWholeMaxPixels = (kOperandBytes - 1) / (kX1C * 4);                // 2 097 151
// whole-frame form at all: x1 below 4 GiB, the large-image forms' bound without vfi_conv_allow_huge
constexpr int64_t kMaxPixels = 0xffffffffLL / (kX1C * 4);                            // 4 194 303
// banded form: x2 = [Hp, Wp, 64], the widest tensor that stays whole, below 2 GiB
constexpr int64_t kLargeMaxPixels = (kOperandBytes - 1) / (kX2C * 4);                // 8 388 607
// rows x Wp of the widest band tensor, x1: below 2 GiB
constexpr int64_t kBandMaxPixels = kWholeMaxPixels;

constexpr int kDefaultBandRows = 256;     // measured at 2160 x 3840 (profiles/sepconv_bench.json "band_sweep"): within 0.3 % of the largest legal height, 2 GB less workspace

struct Band {
    int y0, y1;        // output rows = the heads rows that are kept; y0 even
    int in0, in1;      // x2 rows head1 reads = the rows of the band's x1
    int mid0, mid1;    // x1 rows the head2 layers read = the rows of the band's heads
};

inline int band_count(int Hp, int bh) { return (Hp + bh - 1) / bh; }

inline Band band_at(int Hp, int bh, int b) {
    Band d;
    d.y0 = b * bh;      // b < band_count: below Hp
    d.y1 = Hp - d.y0 < bh ? Hp : d.y0 + bh;
    d.in0 = d.y0 < kHaloIn ? 0 : d.y0 - kHaloIn;
    d.in1 = Hp - d.y1 < kHaloIn ? Hp : d.y1 + kHaloIn;
    d.mid0 = d.y0 < kHaloMid ? 0 : d.y0 - kHaloMid;
    d.mid1 = Hp - d.y1 < kHaloMid ? Hp : d.y1 + kHaloMid;
    return d;
}

// rows of the tallest band's x1 / heads
inline int x1_rows(int Hp, int bh) { return Hp - 2 * kHaloIn < bh ? Hp : bh + 2 * kHaloIn; }
inline int heads_rows(int Hp, int bh) { return Hp - 2 * kHaloMid < bh ? Hp : bh + 2 * kHaloMid; }
inline int out_rows(int Hp, int bh) { return Hp < bh ? Hp : bh; }

inline int64_t x1_band_floats(int Hp, int Wp, int bh) { return (int64_t)x1_rows(Hp, bh) * Wp * kX1C; }
inline int64_t heads_band_floats(int Hp, int Wp, int bh) { return (int64_t)heads_rows(Hp, bh) * Wp * kHeadC; }
inline int64_t planar_band_floats(int Hp, int Wp, int bh) { return (int64_t)out_rows(Hp, bh) * Wp * kPlanes; }      // fits x1's block: 204 bh <= 256 (bh + 8)

constexpr int kMaxBandRows = 65535 * kTileRows;      // the output stage's launch has one grid row per tile row

// a legal band height: a positive multiple of the output tile's rows whose x1 (the widest band operand) stays below 2 GiB
inline bool band_rows_legal(int Hp, int Wp, int bh) {
    return bh > 0 && bh <= kMaxBandRows && bh % kTileRows == 0 && (int64_t)x1_rows(Hp, bh) * Wp <= kBandMaxPixels;
}

// The widest tensor of the part that stays whole-frame, in bytes: x2 = [Hp, Wp, 64], or — frames with an odd row or column count at a
// coarse level, where the up-sampled size 2 ceil(h / 2) exceeds h — a Ver block's up-sampled input or its middle tensor.  The banded form
// needs it below kOperandBytes; for every frame whose sides are multiples of 16 that is the pixel limit and nothing more.
inline int64_t widest_whole_bytes(int Hp, int Wp) {
    static const int ch[5] = {32, 64, 128, 256, 512};
    int64_t h[5], w[5];
    h[0] = Hp, w[0] = Wp;
    for (int r = 1; r < 5; ++r) h[r] = (h[r - 1] + 1) / 2, w[r] = (w[r - 1] + 1) / 2;
    int64_t floats = h[0] * w[0] * kX2C;
    for (int r = 1; r < 4; ++r) {
        const int64_t up = 2 * h[r + 1] * 2 * w[r + 1];
        if (up * ch[r + 1] > floats) floats = up * ch[r + 1];
    }
    return floats * 4;
}

// the largest legal band height that is not taller than the frame rounded up to whole tiles; 0: even 8 rows with their halo do not fit
inline int max_band_rows(int Hp, int Wp) {
    const int64_t tiles = ((int64_t)Hp + kTileRows - 1) / kTileRows * kTileRows;
    const int whole = (int)(tiles < kMaxBandRows ? tiles : kMaxBandRows);
    if ((int64_t)Hp * Wp <= kBandMaxPixels) return whole;
    const int64_t rows = kBandMaxPixels / Wp - 2 * kHaloIn;      // bh + 8 <= rows
    const int64_t bh = rows < kTileRows ? 0 : rows / kTileRows * kTileRows;
    return (int)(bh < whole ? bh : whole);
}

// automatic choice: the measured default where it is legal, else the largest legal height
inline int default_band_rows(int Hp, int Wp) {
    const int top = max_band_rows(Hp, Wp);
    return top < kDefaultBandRows ? top : kDefaultBandRows;
}

}  // namespace sepbands
}  // namespace vfi
