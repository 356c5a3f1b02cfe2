// SepConv++ (vfi_models/sepconv/sepconv_enhanced.py:527-700, Network with intChannels [32, 64, 128, 256, 512]) as a C-side object:
// vfi_sepconvnet_create / _forward / _destroy — weights packed once, workspace owned, the ~70 launches of a frame pair issued by one call.
//
// Forward: replicate-pad both frames to even H, W and normalise them by the joint mean / unbiased std of the padded pair (vfi_m2m_normalize:
// the same code as M2M's), netInput 3 -> 16 on each frame (one block-diagonal 8 -> 32 layer over the two frames side by side = row 0),
// encoder rows 1..4 = conv3(prelu(sconv3_s2(prelu(row[r-1])))), decoder: the Hor blocks row[r] += conv3(prelu(conv3(prelu(row[r])))) on rows
// 4..1, then the Ver chain row[r] += crop(conv3(prelu(conv3(up2(prelu(row[r+1])))))) from row 3 down to row 1, the crop (dropping the last
// row / column when the result is one larger than row[r]) AFTER both convs.  Four heads conv3(prelu(conv3(up2(row1)))) give the 51-tap
// vertical / horizontal filters of both frames; the output is the normalised sum of the two separable convolutions (below).
//
// Scalar PReLUs that follow a conv run in its epilogue (act 1: x > 0 ? x : slope * x, which is what a one-parameter PReLU computes); the
// pre-activations in front of a block's first conv (whose raw input the block still needs) are vfi_prelu_scalar passes.  The four heads'
// first convs are one 64 -> 256 layer with per-channel PReLU (act 3, each head's slope repeated 64 times) reading up2(row1) once.
//
// Two forms of the head stage (ensure_workspace, forward_pair): whole-frame, which materialises x1 = [Hp, Wp, 256] and heads = [Hp, Wp, 208]
// and serves every frame of at most 2 097 151 padded pixels on plain layer forms, and banded (vfi_sepconvnet_set_large_frames; csrc/sepconv_bands.h), which runs
// head1, the head2 layers, the transpose and the output stage per band of output rows and keeps those two tensors for one band only.
//
// New kernels: the fused output stage (sepconv_pair_out_kernel) and three data-movement helpers (the side-by-side interleave of the
// normalised frames, the cropped residual add, the heads' transpose to planar, which makes the output stage's tap loads coalesced).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/vfi_hip.h"
#include "net_object.h"
#include "sepconv_bands.h"
#include "vfi_common.h"

using namespace vfi;

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int K = 51;                                  // filter taps each way
constexpr int R = K / 2;                               // 25: the reference's replicate pad around the frame
constexpr int CH[5] = {32, 64, 128, 256, 512};         // rows 0..4
constexpr int HEAD_CS = 208;                           // head outputs: 4 x 52 channels (51 taps + one gap channel), 16-byte aligned
constexpr int NORM_WS = 64 << 10;                      // vfi_m2m_normalize's workspace

// ---- fused output stage ------------------------------------------------------------------------------------------------------------
// out[y, x, c] = (S0[c] + S1[c]) / n,  S_f[c] = sum_fy ver_f[fy] * sum_fx frame_f[clamp(y + fy - 25), clamp(x + fx - 25), c] * hor_f[fx],
// c = 0..2 and c = 3 the ones channel (n = S0[3] + S1[3], set to 1 where |n| < 0.01).  The replicate pad to even size followed by the
// replicate pad of 25 is a clamp to the frame, so the frame is read in place: no padded copy and no ones channel in memory.
//
// Mapping as sepconv_tile_kernel<51> (ref_ops.hip): a workgroup owns a 64 x 8 output tile, a thread the pixel pair (y, x), (y + 1, x) and
// the four lanes (r, g, b, 1); input rows stream through LDS 8 at a time as float4, so one ds_read_b128 feeds 8 FMAs.  Both frames go
// through the same accumulators.  What differs is the tap storage: the compiler kept every horizontal tap duplicated in both halves of a
// register pair for v_pk_fma_f32 (204 VGPRs of taps, 2 waves per SIMD).  Here the taps sit in pairs (t[2i], t[2i+1]) and
// the packed FMA broadcasts one half to both lanes through op_sel / op_sel_hi: 104 VGPRs of taps for the two pixels.
constexpr int PO_TX = 64, PO_TY = 8, PO_RS = 8;
constexpr int NPAIR = (K + 1) / 2;                     // 26 tap pairs, the last one's high half is 0

template <int SEL>
__device__ __forceinline__ void pk_fma_bcast(f2& acc, f2 a, f2 taps) {
    // acc = a * taps[SEL] + acc in both lanes (one rounding, as an fma)
    if constexpr (SEL == 0)
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(a), "v"(taps));
    else
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(a), "v"(taps));
}

template <bool A, bool B>
__device__ __forceinline__ void row_sums(const float4* __restrict__ row, const f2* ta, const f2* tb, f2& ra_lo, f2& ra_hi, f2& rb_lo,
                                         f2& rb_hi) {
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        {
            const float4 v = row[2 * i];
            const f2 lo = {v.x, v.y}, hi = {v.z, v.w};
            if (A) pk_fma_bcast<0>(ra_lo, lo, ta[i]), pk_fma_bcast<0>(ra_hi, hi, ta[i]);
            if (B) pk_fma_bcast<0>(rb_lo, lo, tb[i]), pk_fma_bcast<0>(rb_hi, hi, tb[i]);
        }
        if (2 * i + 1 < K) {
            const float4 v = row[2 * i + 1];
            const f2 lo = {v.x, v.y}, hi = {v.z, v.w};
            if (A) pk_fma_bcast<1>(ra_lo, lo, ta[i]), pk_fma_bcast<1>(ra_hi, hi, ta[i]);
            if (B) pk_fma_bcast<1>(rb_lo, lo, tb[i]), pk_fma_bcast<1>(rb_hi, hi, tb[i]);
        }
    }
}

__global__ __launch_bounds__(256) void sepconv_pair_out_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int C, int H, int W,
                                                               const float* __restrict__ v0, const float* __restrict__ v1,
                                                               const float* __restrict__ h0, const float* __restrict__ h1, long pstr, long fstr,
                                                               int Wp, int yo, int nrows, float* __restrict__ out) {
    constexpr int LW = PO_TX + K - 1;
    constexpr int ROWS = PO_TY + K - 1;
    __shared__ float4 lds[PO_RS][LW];
    const int tid = threadIdx.x;
    const int tx = tid & 63, tp = tid >> 6;            // tp = wave = pixel-row pair
    // the launch owns the output rows [yo, yo + nrows) (yo a multiple of PO_TY, yo + nrows <= H) and the heads hold those rows only: row yo of
    // the frame is the heads' row 0.  The whole frame is yo = 0, nrows = H.
    const int x0 = blockIdx.x * PO_TX, y0 = yo + blockIdx.y * PO_TY;
    const int x = x0 + tx, ya = y0 + 2 * tp, yb = ya + 1;
    const bool va = x < W && ya < yo + nrows, vb = x < W && yb < yo + nrows;
    // tap f of pixel p at head[p * pstr + f * fstr]: NHWC (pstr = channel stride, fstr = 1) or planar (pstr = 1, fstr = the heads' pixels)
    const size_t pa = ((size_t)(ya - yo) * Wp + x) * pstr, pb = ((size_t)(yb - yo) * Wp + x) * pstr;
    f2 aa_lo = {0.f, 0.f}, aa_hi = {0.f, 0.f}, ab_lo = {0.f, 0.f}, ab_hi = {0.f, 0.f};
    for (int fr = 0; fr < 2; ++fr) {
        const float* __restrict__ f = fr ? f1 : f0;
        const float* __restrict__ ver = fr ? v1 : v0;
        const float* __restrict__ hor = fr ? h1 : h0;
        f2 ta[NPAIR], tb[NPAIR];
        {
            const float* qa = hor + (va ? pa : 0);       // walked tap by tap: one address add per tap, no table of 51 offsets
            const float* qb = hor + (vb ? pb : 0);
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const float a0 = va ? qa[0] : 0.f, b0 = vb ? qb[0] : 0.f;
                qa += fstr, qb += fstr;
                float a1 = 0.f, b1 = 0.f;
                if (2 * i + 1 < K) {
                    a1 = va ? qa[0] : 0.f, b1 = vb ? qb[0] : 0.f;
                    qa += fstr, qb += fstr;
                }
                ta[i] = f2{a0, a1};
                tb[i] = f2{b0, b1};
            }
        }
        for (int r0 = 0; r0 < ROWS; r0 += PO_RS) {
            __syncthreads();
            for (int i = tid; i < PO_RS * LW; i += 256) {
                const int rr = i / LW, cc = i - rr * LW;
                const int gy = min(max(y0 + r0 + rr - R, 0), H - 1), gx = min(max(x0 + cc - R, 0), W - 1);
                const float* p = f + ((size_t)gy * W + gx) * C;
                lds[rr][cc] = make_float4(p[0], p[1], p[2], 1.f);
            }
            __syncthreads();
            // vertical taps one row ahead of their use (the load of row rr + 1 is in flight during row rr's FMAs)
            auto vtap = [&](int rr, float& wa, float& wb) {
                const int fa = r0 + rr - 2 * tp;
                wa = va && fa >= 0 && fa < K ? ver[pa + (size_t)fa * fstr] : 0.f;
                wb = vb && fa >= 1 && fa <= K ? ver[pb + (size_t)(fa - 1) * fstr] : 0.f;
            };
            float wa_n, wb_n;
            vtap(0, wa_n, wb_n);
            for (int rr = 0; rr < PO_RS; ++rr) {
                const float wa = wa_n, wb = wb_n;
                if (rr + 1 < PO_RS) vtap(rr + 1, wa_n, wb_n);
                const int fa = r0 + rr - 2 * tp;        // tap row of the upper pixel; the lower one's is fa - 1
                if (fa < 0 || fa > K) continue;         // wave-uniform
                // both pixels' row sums; at the first / last tap row one of the two weights is 0 (wa / wb above), which keeps one code path
                f2 ra_lo = {0.f, 0.f}, ra_hi = {0.f, 0.f}, rb_lo = {0.f, 0.f}, rb_hi = {0.f, 0.f};
                row_sums<true, true>(&lds[rr][tx], ta, tb, ra_lo, ra_hi, rb_lo, rb_hi);
                aa_lo += ra_lo * wa;
                aa_hi += ra_hi * wa;
                ab_lo += rb_lo * wb;
                ab_hi += rb_hi * wb;
            }
        }
    }
    auto put = [&](int y, f2 lo, f2 hi) {
        float n = hi.y;
        if (fabsf(n) < 0.01f) n = 1.f;
        float* o = out + ((size_t)y * W + x) * 3;
        o[0] = lo.x / n;
        o[1] = lo.y / n;
        o[2] = hi.x / n;
    };
    if (va) put(ya, aa_lo, aa_hi);
    if (vb) put(yb, ab_lo, ab_hi);
}

// ---- data movement ---------------------------------------------------------------------------------------------------------------------
// nrm [2, P, 4] (vfi_m2m_normalize's two images, channels 0..2) -> side [P, 8] = (frame 0 rgb, 0, frame 1 rgb, 0)
__global__ __launch_bounds__(256) void sepnet_side_by_side_kernel(const float* __restrict__ nrm, long P, float* __restrict__ side) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 a = ((const float4*)nrm)[p], b = ((const float4*)nrm)[P + p];
    ((float4*)side)[2 * p] = make_float4(a.x, a.y, a.z, 0.f);
    ((float4*)side)[2 * p + 1] = make_float4(b.x, b.y, b.z, 0.f);
}

// dst [h, w, C] += src [hs, ws, C] cropped to h x w (hs >= h, ws >= w); C % 4 == 0
__global__ __launch_bounds__(256) void sepnet_add_crop_kernel(float* __restrict__ dst, const float* __restrict__ src, int h, int w, int ws, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)h * w * C4) return;
    const int q = (int)(i % C4);
    const long p = i / C4;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    float4 d = ((float4*)dst)[i];
    const float4 s = ((const float4*)src)[((long)y * ws + x) * C4 + q];
    d.x += s.x, d.y += s.y, d.z += s.z, d.w += s.w;
    ((float4*)dst)[i] = d;
}

unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

// heads NHWC [P, HEAD_CS] (head k at channel 52 k) -> planar [4 * 51][P] (head k's tap f at plane 51 k + f), 64 pixels per workgroup through LDS:
// the output stage then reads each tap of 64 neighbouring pixels as one contiguous 256-byte run.  The P pixels start at pixel pin of `in`
// (a band's kept rows inside its heads, which begin with halo rows; the whole frame: 0) and are pixel 0.. of `out`, whose plane stride is P.
__global__ __launch_bounds__(256) void sepnet_heads_planar_kernel(const float* __restrict__ in, long pin, long P, float* __restrict__ out) {
    __shared__ float t[HEAD_CS][65];
    const long p0 = (long)blockIdx.x * 64;
    const int np = P - p0 < 64 ? (int)(P - p0) : 64;
    for (int i = threadIdx.x; i < np * HEAD_CS; i += 256) {
        const int p = i / HEAD_CS, c = i - p * HEAD_CS;
        t[c][p] = in[(pin + p0 + p) * HEAD_CS + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * K * 64; i += 256) {
        const int pl = i >> 6, p = i & 63;
        if (p < np) out[(size_t)pl * P + p0 + p] = t[(pl / K) * 52 + pl % K][p];
    }
}

int pair_out_launch(const float* f0, const float* f1, int C, int H, int W, const float* v0, const float* v1, const float* h0, const float* h1,
                    long pstr, long fstr, int Wp, int yo, int nrows, float* out, hipStream_t st) {
    TraceScope ts("sepconv_pair_out", st);
    sepconv_pair_out_kernel<<<dim3((W + PO_TX - 1) / PO_TX, (nrows + PO_TY - 1) / PO_TY), 256, 0, st>>>(f0, f1, C, H, W, v0, v1, h0, h1, pstr, fstr,
                                                                                                     Wp, yo, nrows, out);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

struct vfi_sepconvnet : NetObject {
    vfi_conv_t* in = nullptr;                         // netInput of both frames: block-diagonal 8 -> 32
    vfi_conv_t* enc[5][2] = {};                       // rows 1..4: sconv3 s2, conv3
    vfi_conv_t* hor[5][2] = {};                       // rows 1..4
    vfi_conv_t* ver[5][2] = {};                       // rows 1..3 (built from row r + 1)
    vfi_conv_t* head1 = nullptr;                      // the four heads' first convs, 64 -> 256, per-channel PReLU
    vfi_conv_t* head2[4] = {};                        // 64 -> 51 each
    vfi_conv_t* head1s[4] = {};                       // the same first convs as four 64 -> 64 layers (A/B option sepconv_split_heads)
    float head_s[4] = {};
    float enc_s[5][2] = {}, hor_s[5][2] = {}, ver_s[5][2] = {};
    // workspace for one pair at Hp x Wp (the pairs of a call run one after another)
    int Hp = 0, Wp = 0;
    int h[5] = {}, w[5] = {};
    float *nrm = nullptr, *side = nullptr, *stats = nullptr, *nws = nullptr;
    float* row[5][2] = {};
    int cur[5] = {};
    float *x1 = nullptr, *x2 = nullptr, *x3 = nullptr, *heads = nullptr;
    bool large = false;                               // vfi_sepconvnet_set_large_frames: frames over kWholeMaxPixels take the banded head stage
    int band = 0;                                     // the workspace's form: 0 whole-frame, > 0 banded with this band height
};

namespace {

// band: 0 = the whole-frame form, > 0 = the banded form with that band height (x1 and heads sized for one band with its halo)
int ensure_workspace(vfi_sepconvnet* m, int Hp, int Wp, int band) {
    if (m->ws.live() && m->Hp == Hp && m->Wp == Wp && m->band == band) return 0;
    if (m->ws.release()) return -1;
    auto get = [&](float** p, size_t floats) { return m->ws.alloc(p, floats, Workspace::kNoFill, nullptr); };
    const size_t P = (size_t)Hp * Wp;
    m->h[0] = Hp, m->w[0] = Wp;
    for (int r = 1; r < 5; ++r) m->h[r] = (m->h[r - 1] + 1) / 2, m->w[r] = (m->w[r - 1] + 1) / 2;
    // scratch sizes: x1 = a pre-activated row (<= 32 P) or the heads' 256-channel layer; x2 = up-sampled rows (<= 128 channels at
    // 2h2 x 2w2 <= 32 P) or up2(row1) (64 P); x3 = a block's middle tensor (<= 64 channels at row 1's size, or the Ver convs at 2h x 2w)
    size_t x3 = 0, x2 = 64 * P;
    for (int r = 1; r < 5; ++r) x3 = std::max(x3, (size_t)m->h[r] * m->w[r] * CH[r]);
    for (int r = 1; r < 4; ++r) {
        const size_t up = (size_t)(2 * m->h[r + 1]) * (2 * m->w[r + 1]);
        x3 = std::max(x3, up * CH[r]);
        x2 = std::max(x2, up * CH[r + 1]);
    }
    size_t x1 = 256 * P, heads = P * HEAD_CS;
    if (band) {
        // x1 outside the head stage: the pre-activated rows of the encoder and the decoder blocks and, where a Ver block crops, its second
        // conv's output at 2 h x 2 w
        x1 = (size_t)sepbands::x1_band_floats(Hp, Wp, band);
        for (int r = 0; r < 5; ++r) x1 = std::max(x1, (size_t)m->h[r] * m->w[r] * CH[r]);
        for (int r = 1; r < 4; ++r) x1 = std::max(x1, (size_t)(2 * m->h[r + 1]) * (2 * m->w[r + 1]) * CH[r]);
        heads = (size_t)sepbands::heads_band_floats(Hp, Wp, band);
    }
    if (get(&m->nrm, 2 * P * 4) || get(&m->side, P * 8) || get(&m->stats, 64) || get(&m->nws, NORM_WS / 4) || get(&m->x1, x1) ||
        get(&m->x2, x2) || get(&m->x3, x3) || get(&m->heads, heads) || get(&m->row[0][0], P * CH[0]))
        return -1;
    for (int r = 1; r < 5; ++r)
        for (int j = 0; j < 2; ++j)
            if (get(&m->row[r][j], (size_t)m->h[r] * m->w[r] * CH[r])) return -1;
    m->Hp = Hp, m->Wp = Wp, m->band = band;
    return 0;
}

int conv(const vfi_conv_t* L, const float* in, int in_cs, int h, int w, float* out, int out_cs, int act, float slope, const float* res,
         int res_cs, hipStream_t st) {
    return vfi_conv_forward_ex(L, in, in_cs, h, w, out, out_cs, 1, act, slope, 0.f, 0.f, res, res_cs, st);
}

int prelu(const float* in, float* out, int C, int h, int w, float slope, hipStream_t st) {
    return vfi_prelu_scalar(in, C, out, C, C, (int64_t)h * w, slope, st);
}

int up2(const float* in, float* out, int C, int h, int w, hipStream_t st) {
    // F.interpolate(scale_factor=2.0, bilinear, align_corners=False): output 2h x 2w, source step (float)(1 / 2)
    return vfi_resize_bilinear_ratio(in, C, out, C, 1, h, w, 2 * h, 2 * w, C, 0.5f, 0.5f, 1.f, st);
}

// The head stage from x2 = up2(row1) on, band by band (csrc/sepconv_bands.h: rows, halo and why the bits are the whole-frame form's): the
// default forms only (one 64 -> 256 head1 layer, planar heads).  Every layer call is sized as the frame's (ConvDecideRows), so a band takes
// the kernel and the tile the whole-frame call takes.
int head_stage_bands(vfi_sepconvnet* m, const float* f0, const float* f1, int C, int H, int W, float* out, hipStream_t st) {
    const int Hp = m->Hp, Wp = m->Wp, bh = m->band;
    ConvDecideRows as_frame(Hp);
    for (int b = 0; b < sepbands::band_count(Hp, bh); ++b) {
        const sepbands::Band d = sepbands::band_at(Hp, bh, b);
        const float* x2 = m->x2 + (size_t)d.in0 * Wp * 64;
        if (conv(m->head1, x2, 64, d.in1 - d.in0, Wp, m->x1, 256, 3, 0.f, nullptr, 0, st)) return -1;
        const float* x1 = m->x1 + (size_t)(d.mid0 - d.in0) * Wp * 256;
        for (int k = 0; k < 4; ++k)
            if (conv(m->head2[k], x1 + 64 * k, 256, d.mid1 - d.mid0, Wp, m->heads + 52 * k, HEAD_CS, 0, 0.f, nullptr, 0, st)) return -1;
        const int nrows = std::min(d.y1, H) - d.y0;      // >= 1: y0 <= Hp - 2 < H
        const long Pb = (long)(d.y1 - d.y0) * Wp;        // the planar band: all Wp columns of the band's rows, as the whole-frame form keeps them
        {   // planar into x1 (free again)
            TraceScope ts("sepnet_heads_planar", st);
            sepnet_heads_planar_kernel<<<(unsigned)((Pb + 63) / 64), 256, 0, st>>>(m->heads, (long)(d.y0 - d.mid0) * Wp, Pb, m->x1);
            VFI_CHECK_HIP(hipGetLastError());
        }
        if (pair_out_launch(f0, f1, C, H, W, m->x1, m->x1 + K * Pb, m->x1 + 2 * K * Pb, m->x1 + 3 * K * Pb, 1, Pb, Wp, d.y0, nrows, out, st)) return -1;
    }
    return 0;
}

int forward_pair(vfi_sepconvnet* m, const float* f0, const float* f1, int C, int H, int W, float* out, hipStream_t st) {
    const int Hp = m->Hp, Wp = m->Wp;
    const long P = (long)Hp * Wp;
    // input: even pad + joint normalisation, both frames side by side, netInput of each into row 0's two 16-channel halves
    if (vfi_m2m_normalize(f0, f1, C, H, W, Hp, Wp, m->nrm, 4, 0, m->stats, m->nws, NORM_WS, st)) return -1;
    {
        TraceScope ts("sepnet_side_by_side", st);
        sepnet_side_by_side_kernel<<<blocks(P), 256, 0, st>>>(m->nrm, P, m->side);
        VFI_CHECK_HIP(hipGetLastError());
    }
    float* row[5];
    for (int r = 0; r < 5; ++r) m->cur[r] = 0, row[r] = m->row[r][0];
    if (conv(m->in, m->side, 8, Hp, Wp, row[0], CH[0], 0, 0.f, nullptr, 0, st)) return -1;
    const int* h = m->h;
    const int* w = m->w;
    // encoder: row[r] = conv3(prelu(sconv3_s2(prelu(row[r-1]))))
    for (int r = 1; r < 5; ++r) {
        if (prelu(row[r - 1], m->x1, CH[r - 1], h[r - 1], w[r - 1], m->enc_s[r][0], st) ||
            conv(m->enc[r][0], m->x1, CH[r - 1], h[r - 1], w[r - 1], m->x3, CH[r], 1, m->enc_s[r][1], nullptr, 0, st) ||
            conv(m->enc[r][1], m->x3, CH[r], h[r], w[r], row[r], CH[r], 0, 0.f, nullptr, 0, st))
            return -1;
    }
    auto swap_row = [&](int r) { m->cur[r] ^= 1, row[r] = m->row[r][m->cur[r]]; };
    // decoder Hor blocks, rows 4..1: row[r] += conv3(prelu(conv3(prelu(row[r]))))
    for (int r = 4; r >= 1; --r) {
        float* dst = m->row[r][m->cur[r] ^ 1];
        if (prelu(row[r], m->x1, CH[r], h[r], w[r], m->hor_s[r][0], st) ||
            conv(m->hor[r][0], m->x1, CH[r], h[r], w[r], m->x3, CH[r], 1, m->hor_s[r][1], nullptr, 0, st) ||
            conv(m->hor[r][1], m->x3, CH[r], h[r], w[r], dst, CH[r], 0, 0.f, row[r], CH[r], st))
            return -1;
        swap_row(r);
    }
    // decoder Ver chain, rows 3..1: row[r] += crop(conv3(prelu(conv3(up2(prelu(row[r+1]))))))
    for (int r = 3; r >= 1; --r) {
        const int hu = 2 * h[r + 1], wu = 2 * w[r + 1];
        if (prelu(row[r + 1], m->x1, CH[r + 1], h[r + 1], w[r + 1], m->ver_s[r][0], st) || up2(m->x1, m->x2, CH[r + 1], h[r + 1], w[r + 1], st) ||
            conv(m->ver[r][0], m->x2, CH[r + 1], hu, wu, m->x3, CH[r], 1, m->ver_s[r][1], nullptr, 0, st))
            return -1;
        if (hu == h[r] && wu == w[r]) {
            if (conv(m->ver[r][1], m->x3, CH[r], hu, wu, m->row[r][m->cur[r] ^ 1], CH[r], 0, 0.f, row[r], CH[r], st)) return -1;
            swap_row(r);
        } else {
            if (conv(m->ver[r][1], m->x3, CH[r], hu, wu, m->x1, CH[r], 0, 0.f, nullptr, 0, st)) return -1;
            TraceScope ts("sepnet_add_crop", st);
            sepnet_add_crop_kernel<<<blocks((long)h[r] * w[r] * CH[r] / 4), 256, 0, st>>>(row[r], m->x1, h[r], w[r], wu, CH[r] / 4);
            VFI_CHECK_HIP(hipGetLastError());
        }
    }
    // heads: conv3(prelu(conv3(up2(row1)))) x 4, the first convs as one 64 -> 256 layer
    if (up2(row[1], m->x2, CH[1], h[1], w[1], st)) return -1;
    if (m->band) return head_stage_bands(m, f0, f1, C, H, W, out, st);
    if (option(kOptSepconvSplitHeads)) {
        for (int k = 0; k < 4; ++k)
            if (conv(m->head1s[k], m->x2, 64, Hp, Wp, m->x1, 64, 1, m->head_s[k], nullptr, 0, st) ||
                conv(m->head2[k], m->x1, 64, Hp, Wp, m->heads + 52 * k, HEAD_CS, 0, 0.f, nullptr, 0, st))
                return -1;
    } else {
        if (conv(m->head1, m->x2, 64, Hp, Wp, m->x1, 256, 3, 0.f, nullptr, 0, st)) return -1;
        for (int k = 0; k < 4; ++k)
            if (conv(m->head2[k], m->x1 + 64 * k, 256, Hp, Wp, m->heads + 52 * k, HEAD_CS, 0, 0.f, nullptr, 0, st)) return -1;
    }
    // heads order: netVerone, netVertwo, netHorone, netHortwo
    if (!option(kOptSepconvPlanar))
        return pair_out_launch(f0, f1, C, H, W, m->heads, m->heads + 52, m->heads + 104, m->heads + 156, HEAD_CS, 1, Wp, 0, H, out, st);
    {   // planar into x1 (free again: 4 * 51 planes <= its 256)
        TraceScope ts("sepnet_heads_planar", st);
        sepnet_heads_planar_kernel<<<(unsigned)((P + 63) / 64), 256, 0, st>>>(m->heads, 0, P, m->x1);
        VFI_CHECK_HIP(hipGetLastError());
    }
    return pair_out_launch(f0, f1, C, H, W, m->x1, m->x1 + K * P, m->x1 + 2 * K * P, m->x1 + 3 * K * P, 1, P, Wp, 0, H, out, st);
}

}  // namespace

extern "C" {

int vfi_sepconv_pair_out(const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W, const float* ver0_dev,
                         const float* ver1_dev, const float* hor0_dev, const float* hor1_dev, int head_cs, int Hp, int Wp, float* out_dev,
                         void* stream) {
    VFI_REQUIRE(frame0_dev && frame1_dev && ver0_dev && ver1_dev && hor0_dev && hor1_dev && out_dev && N > 0 && C >= 3 && H > 0 && W > 0 &&
                    Hp >= H && Wp >= W && head_cs >= K,
                "vfi_sepconv_pair_out: bad arguments (N=%d C=%d H=%d W=%d Hp=%d Wp=%d head_cs=%d)", N, C, H, W, Hp, Wp, head_cs);
    const size_t item = (size_t)Hp * Wp * head_cs;
    for (int n = 0; n < N; ++n) {
        VFI_REQUIRE(frame0_dev[n] && frame1_dev[n], "vfi_sepconv_pair_out: null frame pointer for pair %d", n);
        if (int rc = pair_out_launch(frame0_dev[n], frame1_dev[n], C, H, W, ver0_dev + n * item, ver1_dev + n * item, hor0_dev + n * item,
                                     hor1_dev + n * item, head_cs, 1, Wp, 0, H, out_dev + (size_t)n * H * W * 3, (hipStream_t)stream))
            return rc;
    }
    return 0;
}

int vfi_sepconv_pair_out_rows(const float* frame0_dev, const float* frame1_dev, int C, int H, int W, const float* ver0_dev, const float* ver1_dev,
                              const float* hor0_dev, const float* hor1_dev, int64_t pixel_stride, int64_t tap_stride, int Wp, int row0, int rows,
                              float* out_dev, void* stream) {
    VFI_REQUIRE(frame0_dev && frame1_dev && ver0_dev && ver1_dev && hor0_dev && hor1_dev && out_dev && C >= 3 && H > 0 && W > 0 && Wp >= W &&
                    pixel_stride > 0 && tap_stride > 0,
                "vfi_sepconv_pair_out_rows: bad arguments (C=%d H=%d W=%d Wp=%d)", C, H, W, Wp);
    VFI_REQUIRE(row0 >= 0 && row0 % PO_TY == 0 && rows > 0 && rows <= H - row0,
                "vfi_sepconv_pair_out_rows: rows [%d, %d + %d) must start at a multiple of %d and lie inside the %d-row frame", row0, row0, rows, PO_TY, H);
    return pair_out_launch(frame0_dev, frame1_dev, C, H, W, ver0_dev, ver1_dev, hor0_dev, hor1_dev, (long)pixel_stride, (long)tap_stride, Wp, row0, rows,
                           out_dev, (hipStream_t)stream);
}

vfi_sepconvnet_t* vfi_sepconvnet_create(const float* const* tensors, const int64_t* numels, int n_tensors) {
    const int want = 88;
    if (!tensors || !numels || n_tensors != want) {
        set_error("vfi_sepconvnet_create: expected the %d state_dict tensors of SepConv++ in sepconv_spec.sepconv_shapes() order, got %d", want,
                  n_tensors);
        return nullptr;
    }
    vfi_sepconvnet* m = new vfi_sepconvnet();
    TensorCursor cur(tensors, numels, n_tensors, "vfi_sepconvnet_create");
    auto layer = [&](const float* w, const float* b, int cout, int cin, int stride, const float* prelu) {
        return m->add_layer(vfi_conv_create_ex(0, w, b, cout, cin, 3, stride, 0, nullptr, cin, prelu));
    };
    auto make = [&](vfi_conv_t** L, int cout, int cin, int stride) {
        const float* w = cur.take((int64_t)cout * cin * 9);
        const float* b = cur.take(cout);
        if (!cur.ok()) return;
        *L = layer(w, b, cout, cin, stride, nullptr);
        if (*L && stride == 2 && vfi_conv_accept_odd(*L, 1)) m->failed = true;     // the encoder's rows reach odd sizes (135 at 1080p)
    };
    {   // netInput 3 -> 16 on each frame = one 8 -> 32 layer over (frame 0 rgb, 0, frame 1 rgb, 0)
        const float* w = cur.take(16 * 3 * 9);
        const float* b = cur.take(16);
        if (cur.ok()) {
            std::vector<float> w8((size_t)32 * 8 * 9, 0.f), b8(32);
            for (int f = 0; f < 2; ++f)
                for (int co = 0; co < 16; ++co) {
                    b8[f * 16 + co] = b[co];
                    for (int ci = 0; ci < 3; ++ci)
                        for (int t = 0; t < 9; ++t) w8[((size_t)(f * 16 + co) * 8 + f * 4 + ci) * 9 + t] = w[((size_t)co * 3 + ci) * 9 + t];
                }
            m->in = layer(w8.data(), b8.data(), 32, 8, 1, nullptr);
        }
    }
    for (int r = 1; r < 5 && cur.ok(); ++r) {     // netEncode.0.netVer.r: prelu, sconv, prelu, conv
        m->enc_s[r][0] = cur.scalar();
        make(&m->enc[r][0], CH[r], CH[r - 1], 2);
        m->enc_s[r][1] = cur.scalar();
        make(&m->enc[r][1], CH[r], CH[r], 1);
    }
    for (int i = 0; i < 4 && cur.ok(); ++i) {     // netDecode.0.netHor.i = row 4 - i
        const int r = 4 - i;
        m->hor_s[r][0] = cur.scalar();
        make(&m->hor[r][0], CH[r], CH[r], 1);
        m->hor_s[r][1] = cur.scalar();
        make(&m->hor[r][1], CH[r], CH[r], 1);
    }
    for (int i = 1; i < 4 && cur.ok(); ++i) {     // netDecode.0.netVer.i = row 4 - i from row 5 - i
        const int r = 4 - i;
        m->ver_s[r][0] = cur.scalar();
        make(&m->ver[r][0], CH[r], CH[r + 1], 1);
        m->ver_s[r][1] = cur.scalar();
        make(&m->ver[r][1], CH[r], CH[r], 1);
    }
    {   // heads (netVerone, netVertwo, netHorone, netHortwo): conv 64 -> 64, prelu, conv 64 -> 51
        std::vector<float> w1((size_t)256 * 64 * 9), b1(256), s1(256);
        for (int hd = 0; hd < 4; ++hd) {
            const float* w = cur.take(64 * 64 * 9);
            const float* b = cur.take(64);
            const float s = cur.scalar();
            const float* w2 = cur.take((int64_t)K * 64 * 9);
            const float* b2 = cur.take(K);
            if (!cur.ok()) break;
            memcpy(w1.data() + (size_t)hd * 64 * 64 * 9, w, 64 * 64 * 9 * sizeof(float));
            memcpy(b1.data() + hd * 64, b, 64 * sizeof(float));
            std::fill(s1.begin() + hd * 64, s1.begin() + hd * 64 + 64, s);
            m->head2[hd] = layer(w2, b2, K, 64, 1, nullptr);
            m->head1s[hd] = layer(w, b, 64, 64, 1, nullptr);
            m->head_s[hd] = s;
        }
        if (cur.ok()) m->head1 = layer(w1.data(), b1.data(), 256, 64, 1, s1.data());
    }
    if (!cur.finish() || m->failed) {
        vfi_sepconvnet_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_sepconvnet_destroy(vfi_sepconvnet_t* m) { delete m; }

int vfi_sepconvnet_release_workspace(vfi_sepconvnet_t* m) {
    VFI_REQUIRE(m, "vfi_sepconvnet_release_workspace: null object");
    return m->ws.release();
}

int64_t vfi_sepconvnet_workspace_bytes(const vfi_sepconvnet_t* m) { return m ? m->ws.bytes() : 0; }

// The largest padded frame (sides rounded up to even) without large frames: the whole-frame head stage materialises the four heads' first
// layer x1 = [Hp, Wp, 256] fp32, which the layers' large-image forms serve below 4 GiB: Hp * Wp * 1024 <= 2^32 - 1.  (Up to 2 097 151 pixels
// that tensor is below 2 GiB and every layer takes its plain form.)
int64_t vfi_sepconvnet_max_pixels(void) { return sepbands::kMaxPixels; }

// ... with vfi_sepconvnet_set_large_frames: x1 and the heads exist for one band of rows at a time, and the widest tensor that stays whole is
// up2(row1) = x2 = [Hp, Wp, 64] fp32, an operand of plain layer forms: Hp * Wp * 256 < 2^31 - 1 (2160x3840 fits, 2898x2896 does not)
int64_t vfi_sepconvnet_large_max_pixels(void) { return sepbands::kLargeMaxPixels; }

// the limit vfi_sepconvnet_forward holds this object to: one of the two above (0 for a null object)
int64_t vfi_sepconvnet_object_max_pixels(const vfi_sepconvnet_t* m) { return !m ? 0 : (m->large ? sepbands::kLargeMaxPixels : sepbands::kMaxPixels); }

// on: padded frames over 2 097 151 pixels take the banded head stage and the limit is vfi_sepconvnet_large_max_pixels(); smaller frames run
// the whole-frame form, the same launches and bits, either way.  Off (default): today's whole-frame form up to vfi_sepconvnet_max_pixels().
// A workspace of the other form is released at the next forward (its key holds the form).
int vfi_sepconvnet_set_large_frames(vfi_sepconvnet_t* m, int on) {
    VFI_REQUIRE(m, "vfi_sepconvnet_set_large_frames: null object");
    m->large = on != 0;
    return 0;
}

int vfi_sepconvnet_forward(vfi_sepconvnet_t* m, const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W,
                           float* out_dev, void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && out_dev && N > 0 && C >= 3 && H > 0 && W > 0, "vfi_sepconvnet_forward: bad arguments");
    for (int n = 0; n < N; ++n) VFI_REQUIRE(frame0_dev[n] && frame1_dev[n], "vfi_sepconvnet_forward: null frame pointer for pair %d", n);
    hipStream_t st = (hipStream_t)stream;
    // refusals first: nothing is allocated or launched for a frame the object cannot serve (64-bit sums: H + 1 and the product fit)
    const int64_t Hp64 = (int64_t)H + H % 2, Wp64 = (int64_t)W + W % 2, px = Hp64 * Wp64;
    VFI_REQUIRE(m->large || px <= sepbands::kMaxPixels,
                "vfi_sepconvnet_forward: a %dx%d frame (padded %lldx%lld) is over the size limit of %lld padded pixels: the heads' first layer "
                "[Hp, Wp, 256] must stay below 4 GiB; vfi_sepconvnet_set_large_frames raises the limit to %lld",
                H, W, (long long)Hp64, (long long)Wp64, (long long)sepbands::kMaxPixels, (long long)sepbands::kLargeMaxPixels);
    VFI_REQUIRE(!m->large || px <= sepbands::kLargeMaxPixels,
                "vfi_sepconvnet_forward: a %dx%d frame (padded %lldx%lld) is over the size limit with large frames on, %lld padded pixels: "
                "up2(row1) = [Hp, Wp, 64] must stay below 2 GiB",
                H, W, (long long)Hp64, (long long)Wp64, (long long)sepbands::kLargeMaxPixels);
    const int Hp = (int)Hp64, Wp = (int)Wp64;
    int band = (int)option(kOptSepconvBandRows);      // 0 outside the test library
    if (band > 0) {
        VFI_REQUIRE(sepbands::band_rows_legal(Hp, Wp, band), "vfi_sepconvnet_forward: sepconv_band_rows = %d is no legal band height for %dx%d (a "
                    "multiple of %d whose [rows + 8, Wp, 256] tensor stays below 2 GiB)", band, Hp, Wp, sepbands::kTileRows);
    } else if (m->large && px > sepbands::kWholeMaxPixels) {
        band = sepbands::default_band_rows(Hp, Wp);
        VFI_REQUIRE(band > 0, "vfi_sepconvnet_forward: a %dx%d frame is too wide for the banded head stage: a band of %d rows with its halo, "
                    "[%d, Wp, 256], must stay below 2 GiB (Wp <= %lld)", H, W, sepbands::kTileRows, sepbands::kTileRows + 2 * sepbands::kHaloIn,
                    (long long)(sepbands::kBandMaxPixels / (sepbands::kTileRows + 2 * sepbands::kHaloIn)));
    }
    VFI_REQUIRE(!band || sepbands::widest_whole_bytes(Hp, Wp) < sepbands::kOperandBytes,
                "vfi_sepconvnet_forward: a %dx%d frame has a decoder tensor of %lld bytes (an odd coarse level up-sampled past its finer one): it must "
                "stay below 2 GiB", H, W, (long long)sepbands::widest_whole_bytes(Hp, Wp));
    VFI_REQUIRE(!band || (!option(kOptSepconvSplitHeads) && option(kOptSepconvPlanar)),
                "vfi_sepconvnet_forward: the banded head stage has the default forms only (sepconv_split_heads 0, sepconv_planar 1)");
    if (ensure_workspace(m, Hp, Wp, band)) return -1;
    for (int n = 0; n < N; ++n)
        if (forward_pair(m, frame0_dev[n], frame1_dev[n], C, H, W, out_dev + (size_t)n * H * W * 3, st)) return -1;
    return 0;
}

}  // extern "C"
