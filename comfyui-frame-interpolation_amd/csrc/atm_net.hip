// ATM-lite and ATM-base (vfi_models/atm/network_lite.py / network_base.py Network, attention.py ATMFormer / RefineBottleneck): the kernels the
// network needs beyond the shared layer objects and GMFSS ops, and the network object (vfi_atm_create / _create_variant / _forward / ..., at
// the end of the file) that runs one frame pair over them.  The two models share one forward and one module tree; their widths are kCfg's.
//
//   atm_attn            multi-head window attention on token MAPS, 8 heads: centre pad, roll, window cut and their inverses are addressing;
//                       scores and probabilities live in registers; q k^T and p v on the fp32 matrix cores (v_mfma_f32_16x16x4_f32); the
//                       motion read-out rides along as two extra value columns (key x, key y)
//   atm_motion_mlp      the 8 -> 4 -> GELU -> 1 MLP over the heads' offsets, per coordinate
//   atm_dwconv          depthwise 3x3 + bias + GELU (Mlp.dwconv + act)
//   atm_gather_taps     the nine taps of a strided, dilated 3x3 convolution gathered into 9 C channels: the convolution itself is then a 1x1
//                       layer on the MFMA kernel (CrossScaleFeatureFusion.layers)
//   atm_depth_to_space  ConvTranspose2d(k 2, s 2) = a 1x1 layer with 4 Cout outputs + this interleave
//   atm_blend / atm_out the two synthesis steps
//   atm_copy            channel-window copies with an optional per-channel PReLU (the pad is net_object.h's pad_frame_pair)
//   atm_alignment_*     the ensemble's score ("On with Ensemble (slowest)", network_lite.py:540-554): flow up-sampling, both warps and the L1
//                       mean in one pass over the full-resolution pair, summed in a fixed order in two launches (no atomics)
//   atm_select_flow     the ensemble's choice and the winner's resize to the 1/16 map, on the device
//
// Built with -ffp-contract=off (csrc/build.py): `score * scale + mask` and the warp coordinates round as torch rounds them.
#include <cstring>

#include "../../include/vfi_hip.h"
#include "../../include/vfi_hip_test_atm.h"
#include "gmfss_bodies.h"
#include "net_object.h"
#include "vfi_common.h"

namespace vfi {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHeads = 8;

// One workgroup = one window of one frame and one head; four waves, each owning 16-query tiles.  Tokens are addressed in the un-padded maps:
// slot (ty, tx) of window (wy, wx) sits at (r, c) = (wy WIN + ty, wx WIN + tx) of the rolled, padded layout, which is position ((r + shift) %
// hp, (c + shift) % wp) of the padded layout and (that - (top, left)) of the map; a slot outside the map reads token `pad_tok` (norm1 of a
// zero token, projected like the others).  Labels: the nine pad regions and the nine shift regions, both at (r, c) (attention.py:28-62,
// :282-303: the pad mask is built on the un-rolled layout and applied to the rolled windows).  K and V of the head are staged in LDS (V with
// the columns D, D + 1 = the key's x, y inside the window); a wave computes S^T = K Q^T for its 16 queries, so that a lane holds the scores
// of ONE query (column lane & 15) against keys 4 (lane >> 4) + i of every key tile: the softmax is a reduction over the lane's registers and
// two xor-shuffles, and the same registers are the A operand of P V with the key order of the B operand permuted alike.
// lh x lw: the map the PAD labels are taken from, centred in the same hp x wp layout (h x w everywhere but in the ensemble's shifted global
// block, vfi_atm_window_attention_labels); the tokens are addressed by h x w alone.
template <int WIN, int D>
__global__ __launch_bounds__(256) void atm_attn_kernel(const float* __restrict__ q, int q_cs, const float* __restrict__ k, int k_cs,
                                                       const float* __restrict__ v, int v_cs, long pad_tok, float* __restrict__ out, int out_cs,
                                                       float* __restrict__ offs, int h, int w, int hp, int wp, int lh, int lw, int shift, int cross, float scale) {
    constexpr int N = WIN * WIN, NT = N / 16, KS = D / 4, CT = (D + 2 + 15) / 16, DV = CT * 16, KST = D + 1;
    __shared__ float k_s[N * KST];
    __shared__ float v_s[N * DV];
    __shared__ int tok_s[N], lab_s[N];
    const int tid = threadIdx.x;
    const int nwx = wp / WIN, wy = blockIdx.x / nwx, wx = blockIdx.x % nwx;
    const int f = blockIdx.y / kHeads, head = blockIdx.y % kHeads;
    const int top = (hp - h) / 2, left = (wp - w) / 2, ltop = (hp - lh) / 2, lleft = (wp - lw) / 2;
    const bool padded = hp != lh || wp != lw;
    if (tid < N) {
        const int r = wy * WIN + tid / WIN, c = wx * WIN + tid % WIN;
        int lab = 0;
        if (padded) lab = 3 * ((r >= ltop) + (r >= lh + ltop)) + (c >= lleft) + (c >= lw + lleft);
        if (shift) lab = lab * 9 + 3 * ((r >= hp - WIN) + (r >= hp - shift)) + (c >= wp - WIN) + (c >= wp - shift);
        const int y = (r + shift) % hp - top, x = (c + shift) % wp - left;
        tok_s[tid] = (y >= 0 && y < h && x >= 0 && x < w) ? y * w + x : -1;
        lab_s[tid] = lab;
    }
    __syncthreads();
    const long fq = (long)f * h * w, fk = (long)(cross ? f ^ 1 : f) * h * w;
    for (int i = tid; i < N * D; i += 256) {
        const int n = i / D, j = i % D;
        const int t = tok_s[n];
        const size_t idx = t < 0 ? (size_t)pad_tok : (size_t)(fk + t);
        k_s[n * KST + j] = k[idx * k_cs + head * D + j];
        v_s[n * DV + j] = v[idx * v_cs + head * D + j];
    }
    for (int i = tid; i < N * (DV - D); i += 256) {
        const int n = i / (DV - D), j = i % (DV - D);
        v_s[n * DV + D + j] = j == 0 ? (float)(n % WIN) : j == 1 ? (float)(n / WIN) : 0.f;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    for (int qt = wave; qt < NT; qt += 4) {
        const int qn = qt * 16 + l16;
        const int tq = tok_s[qn];
        const float* qp = q + (tq < 0 ? (size_t)pad_tok : (size_t)(fq + tq)) * q_cs + head * D;
        float qr[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) qr[s] = qp[4 * s + g];
        f32x4 S[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k_s[(nt * 16 + l16) * KST + 4 * s + g], qr[s], acc, 0, 0, 0);
            S[nt] = acc;
        }
        // S[nt][i] = <k[nt 16 + 4 g + i], q[qn]>
        const int qlab = lab_s[qn];
        float mx = -3.0e38f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sc = S[nt][i] * scale + (lab_s[nt * 16 + 4 * g + i] != qlab ? -100.0f : 0.0f);
                S[nt][i] = sc;
                mx = fmaxf(mx, sc);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float e = expf(S[nt][i] - mx);
                S[nt][i] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        f32x4 O[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) O[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float p = S[nt][i] * inv;
                const float* vr = v_s + (nt * 16 + 4 * g + i) * DV + l16;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) O[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, vr[ct * 16], O[ct], 0, 0, 0);
            }
        // O[ct][i] = out[query qt 16 + 4 g + i][column ct 16 + l16]; rows of padding are dropped
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int qo = qt * 16 + 4 * g + i;
            const int to = tok_s[qo];
            if (to < 0) continue;
            const size_t dst = (size_t)(fq + to);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int c = ct * 16 + l16;
                if (c < D) out[dst * out_cs + head * D + c] = O[ct][i];
                else if (offs && c < D + 2) offs[dst * (2 * kHeads) + head * 2 + (c - D)] = O[ct][i] - (float)(c == D ? qo % WIN : qo / WIN);
            }
        }
    }
}

__device__ inline float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// motion[f][p][coord] = w2 . gelu(w0 offs[f][p][:, coord] + b0) + b2 (AttentionToMotion.mlp over the heads, attention.py:143-146, :207-211)
__global__ void atm_motion_mlp_kernel(const float* __restrict__ offs, const float* __restrict__ w0, const float* __restrict__ b0,
                                      const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out, int out_cs, long out_fs,
                                      long tpf) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * tpf) return;
    const int coord = (int)(idx & 1);
    const long tok = idx >> 1, f = tok / tpf, p = tok % tpf;
    const float* o = offs + (size_t)tok * (2 * kHeads) + coord;
    float r = b2[0];
#pragma unroll
    for (int j = 0; j < kHeads / 2; ++j) {
        float a = b0[j];
#pragma unroll
        for (int hd = 0; hd < kHeads; ++hd) a = fmaf(w0[j * kHeads + hd], o[2 * hd], a);
        r = fmaf(w2[j], gelu_erf(a), r);
    }
    out[(size_t)f * out_fs + (size_t)p * out_cs + coord] = r;
}

// out = gelu(depthwise 3x3 (zero padding 1) + bias); wp [9][C]; one thread per pixel and four channels
__global__ void atm_dwconv_kernel(const float* __restrict__ in, int in_cs, const float* __restrict__ wp, const float* __restrict__ bias,
                                  float* __restrict__ out, int out_cs, int N, int H, int W, int C) {
    const int C4 = C / 4;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * H * W * C4) return;
    const int c = (int)(idx % C4) * 4;
    const long p = idx / C4;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const long n = p / ((long)W * H);
    float4 a = *(const float4*)(bias + c);
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = x + kx - 1;
            if (xx < 0 || xx >= W) continue;
            const float4 v = *(const float4*)(in + ((size_t)(n * H + yy) * W + xx) * in_cs + c);
            const float4 wv = *(const float4*)(wp + (size_t)(ky * 3 + kx) * C + c);
            a.x = fmaf(v.x, wv.x, a.x), a.y = fmaf(v.y, wv.y, a.y), a.z = fmaf(v.z, wv.z, a.z), a.w = fmaf(v.w, wv.w, a.w);
        }
    }
    *(float4*)(out + (size_t)p * out_cs + c) = make_float4(gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w));
}

// out[n, y, x, t C + c] = in[n, y s + (ky - 1) d, x s + (kx - 1) d, c], t = 3 ky + kx, zero outside: Conv2d(k 3, stride s, dilation d, padding d)
__global__ void atm_gather_taps_kernel(const float* __restrict__ in, int in_cs, float* __restrict__ out, int out_cs, int N, int H, int W, int C,
                                       int Ho, int Wo, int stride, int dil) {
    const int C4 = C / 4;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * Ho * Wo * 9 * C4) return;
    const int c = (int)(idx % C4) * 4;
    long p = idx / C4;
    const int t = (int)(p % 9);
    p /= 9;
    const int x = (int)(p % Wo), y = (int)((p / Wo) % Ho);
    const long n = p / ((long)Wo * Ho);
    const int yy = y * stride + (t / 3 - 1) * dil, xx = x * stride + (t % 3 - 1) * dil;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = *(const float4*)(in + ((size_t)(n * H + yy) * W + xx) * in_cs + c);
    *(float4*)(out + (size_t)p * out_cs + t * C + c) = v;
}

// out[n, 2 y + ky, 2 x + kx, c] = in[n, y, x, (2 ky + kx) C + c]
__global__ void atm_depth_to_space_kernel(const float* __restrict__ in, int in_cs, float* __restrict__ out, int out_cs, int N, int H, int W, int C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * 4 * H * W * C) return;
    const int c = (int)(idx % C);
    const long p = idx / C;
    const int X = (int)(p % (2 * W)), Y = (int)((p / (2 * W)) % (2 * H));
    const long n = p / ((long)4 * W * H);
    out[(size_t)p * out_cs + c] = in[((size_t)(n * H + (Y >> 1)) * W + (X >> 1)) * in_cs + ((Y & 1) * 2 + (X & 1)) * C + c];
}

// flow_warp (flow_warp.py:26-60) of a 3-channel image at one pixel: grid_sample's normalise / un-normalise round trip, zeros outside; the
// normalised coordinate is brought next to [-1, 1] first so that the tap index stays an int whatever the flow (NaN: every tap outside)
__device__ inline void warp3(const float* img, int cs, int W, int H, int X, int Y, float fx, float fy, float* o) {
    float gx = 2.0f * ((float)X + fx) / (float)(W - 1) - 1.0f, gy = 2.0f * ((float)Y + fy) / (float)(H - 1) - 1.0f;
    gx = gx == gx ? fminf(fmaxf(gx, -4.0f), 4.0f) : -4.0f, gy = gy == gy ? fminf(fmaxf(gy, -4.0f), 4.0f) : -4.0f;
    const vfi_gmfss::ZTap t = vfi_gmfss::ztap_from_norm(gx, gy, W, H);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = vfi_gmfss::ztap_read(img, cs, W, H, t, c);
}

// out[.., 0..14] = (orig0 | w0 = warp(src0, flow0) | orig1 | w1 = warp(src1, flow1) | sigmoid(m) w0 + (1 - sigmoid(m)) w1); motion = (flow0 xy,
// flow1 xy, m).  orig null: channels 0..2 and 6..8 are left alone.
__global__ void atm_blend_kernel(const float* __restrict__ src0, const float* __restrict__ src1, int src_cs, const float* __restrict__ orig0,
                                 const float* __restrict__ orig1, int orig_cs, const float* __restrict__ motion, int motion_cs, float* __restrict__ out,
                                 int out_cs, int H, int W) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int X = (int)(idx % W), Y = (int)(idx / W);
    const float* mo = motion + (size_t)idx * motion_cs;
    float* o = out + (size_t)idx * out_cs;
    float w0[3], w1[3];
    warp3(src0, src_cs, W, H, X, Y, mo[0], mo[1], w0);
    warp3(src1, src_cs, W, H, X, Y, mo[2], mo[3], w1);
    const float m = 1.0f / (1.0f + expf(-mo[4])), om = 1.0f - m;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (orig0) o[c] = orig0[(size_t)idx * orig_cs + c], o[6 + c] = orig1[(size_t)idx * orig_cs + c];
        o[3 + c] = w0[c], o[9 + c] = w1[c];
        o[12 + c] = m * w0[c] + om * w1[c];
    }
}

// out [H,W,3] = clamp(I_t + 2 sigmoid(res) - 1, 0, 1) cropped at (top, left) of the padded frame
__global__ void atm_out_kernel(const float* __restrict__ it, int it_cs, const float* __restrict__ res, int res_cs, float* __restrict__ out, int Wp,
                               int top, int left, int H, int W) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const size_t p = (size_t)((int)(idx / W) + top) * Wp + ((int)(idx % W) + left);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = 1.0f / (1.0f + expf(-res[p * res_cs + c]));
        out[(size_t)idx * 3 + c] = fminf(fmaxf(it[p * it_cs + c] + (2.0f * s - 1.0f), 0.f), 1.f);
    }
}

// out[p, c] = prelu(in[p, c]) over a channel window (slopes null: a copy)
__global__ void atm_copy_kernel(const float* __restrict__ in, int in_cs, const float* __restrict__ slopes, float* __restrict__ out, int out_cs,
                                long pixels, int C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pixels * C) return;
    const int c = (int)(idx % C);
    const long p = idx / C;
    const float v = in[(size_t)p * in_cs + c];
    out[(size_t)p * out_cs + c] = (slopes && v < 0.f) ? v * slopes[c] : v;
}

// F.interpolate(align_corners=True) of a coarse [hi,wi] map at destination pixel (y, x) of an [ho,wo] one: the taps and weights of
// resize_ac_body (csrc/gmfss_bodies.h): PyTorch's area-pixel scale (in - 1) / (out - 1), 0 for a one-pixel destination, so a one-pixel source
// gives a constant
struct AcTap {
    int i00, i01, i10, i11;      // pixel indices into the coarse map
    float hy, ly, hx, lx;
};
__device__ inline AcTap ac_tap(int y, int x, int hi, int wi, int ho, int wo) {
    const float ry = ho > 1 ? (float)(hi - 1) / (float)(ho - 1) : 0.f, rx = wo > 1 ? (float)(wi - 1) / (float)(wo - 1) : 0.f;
    const float sy = ry * (float)y, sx = rx * (float)x;
    const int y0 = min((int)sy, hi - 1), x0 = min((int)sx, wi - 1);      // (the min never binds for y < ho, x < wo: it keeps the taps inside whatever the caller passes)
    const int y1 = y0 + (y0 < hi - 1 ? 1 : 0), x1 = x0 + (x0 < wi - 1 ? 1 : 0);
    AcTap t;
    t.i00 = y0 * wi + x0, t.i01 = y0 * wi + x1, t.i10 = y1 * wi + x0, t.i11 = y1 * wi + x1;
    t.ly = sy - (float)y0, t.lx = sx - (float)x0, t.hy = 1.0f - t.ly, t.hx = 1.0f - t.lx;
    return t;
}
__device__ inline float ac_read(const float* map, int cs, const AcTap& t, int c, float mul) {
    return (t.hy * (t.hx * map[(size_t)t.i00 * cs + c] + t.lx * map[(size_t)t.i01 * cs + c]) +
            t.ly * (t.hx * map[(size_t)t.i10 * cs + c] + t.lx * map[(size_t)t.i11 * cs + c])) * mul;
}

constexpr int kLossBlock = 256;      // pixels (= threads) per workgroup of the scoring kernel; its grid follows from the frame size alone

// global_alignmentness (network_lite.py:540-554), stage 1: per full-resolution pixel the four flow channels of the coarse motion map are
// interpolated (upsample_flow: align_corners=True, values x f), both frames are warped there (warp3: the warps' own arithmetic) and |a - b| is
// summed over the three channels; nothing full-resolution is written.  The workgroup's 256 terms are summed in a fixed tree: xor-shuffles
// over the wave (32, 16, .., 1), then the four wave sums in wave order through LDS.  partial[blockIdx.x] = that sum.
__global__ __launch_bounds__(kLossBlock) void atm_alignment_partial_kernel(const float* __restrict__ pair, int cs, int Hp, int Wp,
                                                                            const float* __restrict__ motion, int mcs, int h, int w, float f,
                                                                            float* __restrict__ partial) {
    __shared__ float wave_s[kLossBlock / 64];
    const long idx = (long)blockIdx.x * kLossBlock + threadIdx.x;
    float v = 0.f;
    if (idx < (long)Hp * Wp) {
        const int X = (int)(idx % Wp), Y = (int)(idx / Wp);
        const AcTap t = ac_tap(Y, X, h, w, Hp, Wp);
        float a[3], b[3];
        warp3(pair, cs, Wp, Hp, X, Y, ac_read(motion, mcs, t, 0, f), ac_read(motion, mcs, t, 1, f), a);
        warp3(pair + (size_t)Hp * Wp * cs, cs, Wp, Hp, X, Y, ac_read(motion, mcs, t, 2, f), ac_read(motion, mcs, t, 3, f), b);
        v = (fabsf(a[0] - b[0]) + fabsf(a[1] - b[1])) + fabsf(a[2] - b[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wave_s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wave_s[0] + wave_s[1]) + wave_s[2]) + wave_s[3];
}

// stage 2, ONE workgroup: thread t adds partial[t], partial[t + 256], .. in index order in double, the 256 sums are added in a fixed LDS tree;
// loss = sum / (3 Hp Wp).  No atomics, and no dependence on the number of CUs: the same input gives the same bits.
__global__ __launch_bounds__(256) void atm_alignment_final_kernel(const float* __restrict__ partial, int n, double count, float* __restrict__ loss) {
    __shared__ double sum_s[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    sum_s[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sum_s[threadIdx.x] += sum_s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(sum_s[0] / count);
}

// multiscale_global_motion_ensemble's choice (network_lite.py:583-595) on the device: level = the first of 0, 1, 2 whose loss equals the
// smallest (Python's min, then the == chain), and channels 0..3 of out [h16,w16] = that level's flows resized x 1 / 2 / 4 (upsample_flow:
// align_corners=True, values x factor; level 0 is copied).  Every thread reads the three losses; thread 0 writes the record.
__global__ void atm_select_flow_kernel(const float* __restrict__ losses, const float* __restrict__ m0, const float* __restrict__ m1,
                                       const float* __restrict__ m2, int mcs, int h16, int w16, float* __restrict__ out, int out_cs,
                                       float* __restrict__ record) {
    const float l0 = losses[0], l1 = losses[1], l2 = losses[2];
    const float mn = fminf(fminf(l0, l1), l2);
    const int level = l0 == mn ? 0 : l1 == mn ? 1 : 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0 && record) record[0] = l0, record[1] = l1, record[2] = l2, record[3] = (float)level;
    if (idx >= (long)h16 * w16) return;
    float* o = out + (size_t)idx * out_cs;
    if (level == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = m0[(size_t)idx * mcs + c];
        return;
    }
    const float* m = level == 1 ? m1 : m2;
    const AcTap t = ac_tap((int)(idx / w16), (int)(idx % w16), h16 >> level, w16 >> level, h16, w16);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = ac_read(m, mcs, t, c, (float)(1 << level));
}

}  // namespace
}  // namespace vfi

using namespace vfi;

extern "C" {

int vfi_atm_window_attention(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, int64_t pad_token,
                             float* out_dev, int out_cs, float* offsets_dev, int h, int w, int C, int window, int shift, int cross, void* stream) {
    return vfi_atm_window_attention_labels(q_dev, q_cs, k_dev, k_cs, v_dev, v_cs, pad_token, out_dev, out_cs, offsets_dev, h, w, h, w, C, window, shift,
                                           cross, stream);
}

int vfi_atm_window_attention_labels(const float* q_dev, int q_cs, const float* k_dev, int k_cs, const float* v_dev, int v_cs, int64_t pad_token,
                                    float* out_dev, int out_cs, float* offsets_dev, int h, int w, int label_h, int label_w, int C, int window,
                                    int shift, int cross, void* stream) {
    VFI_REQUIRE(q_dev && k_dev && v_dev && out_dev && h > 0 && w > 0 && q_cs >= C && k_cs >= C && v_cs >= C && out_cs >= C,
                "vfi_atm_window_attention: bad arguments");
    VFI_REQUIRE(((C == 224 || C == 384) && window == 8) || ((C == 352 || C == 672) && window == 12),
                "vfi_atm_window_attention: C = %d with window %d: the kernel is built for 224 / 8 and 352 / 12 (ATM-lite: 8 heads of 28 / 44) and for "
                "384 / 8 and 672 / 12 (ATM-base: 8 heads of 48 / 84)", C, window);
    VFI_REQUIRE(shift == 0 || shift == window / 2, "vfi_atm_window_attention: shift %d must be 0 or half the window (%d)", shift, window / 2);
    VFI_REQUIRE(!offsets_dev || cross, "vfi_atm_window_attention: the motion read-out belongs to the cross kind");
    const int hp = round_up(h, window), wp = round_up(w, window);
    VFI_REQUIRE(label_h > 0 && label_w > 0 && round_up(label_h, window) == hp && round_up(label_w, window) == wp,
                "vfi_atm_window_attention: the %dx%d label map does not pad to the %dx%d layout of the %dx%d map", label_h, label_w, hp, wp, h, w);
    VFI_REQUIRE((hp == h && wp == w) || pad_token >= 0, "vfi_atm_window_attention: a %dx%d map is padded to %dx%d and needs a pad token", h, w, hp, wp);
    VFI_REQUIRE((long)2 * h * w * 3 * C < (1L << 31) && pad_token < (1L << 31) / (3 * C), "vfi_atm_window_attention: a %dx%d map is beyond the kernel's index arithmetic", h, w);
    TraceScope ts(cross ? "atm_attn_cross" : "atm_attn_self", (hipStream_t)stream);
    const dim3 grid((hp / window) * (wp / window), 2 * kHeads);
#define ATM_ATTN(WIN, D)                                                                                                                              \
    hipLaunchKernelGGL((atm_attn_kernel<WIN, D>), grid, dim3(256), 0, (hipStream_t)stream, q_dev, q_cs, k_dev, k_cs, v_dev, v_cs, (long)pad_token, \
                       out_dev, out_cs, offsets_dev, h, w, hp, wp, label_h, label_w, shift, cross, (float)(1.0 / sqrt((double)D)))
    if (C == 224) ATM_ATTN(8, 28);
    else if (C == 352) ATM_ATTN(12, 44);
    else if (C == 384) ATM_ATTN(8, 48);
    else ATM_ATTN(12, 84);
#undef ATM_ATTN
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_motion_mlp(const float* offsets_dev, const float* w0_dev, const float* b0_dev, const float* w2_dev, const float* b2_dev, float* out_dev,
                       int out_cs, int64_t out_frame_stride, int64_t tokens_per_frame, void* stream) {
    VFI_REQUIRE(offsets_dev && w0_dev && b0_dev && w2_dev && b2_dev && out_dev && out_cs >= 2 && tokens_per_frame > 0 &&
                    tokens_per_frame < (1L << 26), "vfi_atm_motion_mlp: bad arguments");
    TraceScope ts("atm_motion_mlp", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_motion_mlp_kernel, dim3(nblk(4 * tokens_per_frame, 256)), dim3(256), 0, (hipStream_t)stream, offsets_dev, w0_dev, b0_dev,
                       w2_dev, b2_dev, out_dev, out_cs, (long)out_frame_stride, (long)tokens_per_frame);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_dwconv3x3_gelu(const float* in_dev, int in_cs, const float* w_dev, const float* bias_dev, float* out_dev, int out_cs, int N, int H, int W,
                           int C, void* stream) {
    VFI_REQUIRE(in_dev && w_dev && bias_dev && out_dev && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && in_cs >= C && out_cs >= C &&
                    in_cs % 4 == 0 && out_cs % 4 == 0 && aligned16(in_dev) && aligned16(out_dev) && aligned16(w_dev) && aligned16(bias_dev),
                "vfi_atm_dwconv3x3_gelu: bad arguments (C = %d and both strides multiples of 4, buffers 16-byte aligned)", C);
    VFI_REQUIRE((long)N * H * W * in_cs < (1L << 31) && (long)N * H * W * out_cs < (1L << 31), "vfi_atm_dwconv3x3_gelu: %d x %dx%d is beyond the kernel's index arithmetic", N, H, W);
    TraceScope ts("atm_dwconv", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_dwconv_kernel, dim3(nblk((long)N * H * W * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, w_dev, bias_dev,
                       out_dev, out_cs, N, H, W, C);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_gather_taps(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, int stride, int dilation, void* stream) {
    VFI_REQUIRE(in_dev && out_dev && N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && in_cs >= C && out_cs >= 9 * C && in_cs % 4 == 0 &&
                    out_cs % 4 == 0 && aligned16(in_dev) && aligned16(out_dev) && (stride == 2 || stride == 4) && (dilation == 1 || dilation == 2),
                "vfi_atm_gather_taps: bad arguments (C = %d and both strides multiples of 4, stride %d in {2, 4}, dilation %d in {1, 2})", C, stride, dilation);
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    VFI_REQUIRE((long)N * H * W * in_cs < (1L << 31) && (long)N * Ho * Wo * out_cs < (1L << 31), "vfi_atm_gather_taps: %d x %dx%d is beyond the kernel's index arithmetic", N, H, W);
    TraceScope ts("atm_gather_taps", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_gather_taps_kernel, dim3(nblk((long)N * Ho * Wo * 9 * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, out_dev,
                       out_cs, N, H, W, C, Ho, Wo, stride, dilation);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_depth_to_space2(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, void* stream) {
    VFI_REQUIRE(in_dev && out_dev && N > 0 && H > 0 && W > 0 && C > 0 && in_cs >= 4 * C && out_cs >= C, "vfi_atm_depth_to_space2: bad arguments");
    VFI_REQUIRE((long)N * H * W * in_cs < (1L << 31) && (long)N * 4 * H * W * out_cs < (1L << 31), "vfi_atm_depth_to_space2: %d x %dx%d is beyond the kernel's index arithmetic", N, H, W);
    TraceScope ts("atm_depth_to_space", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_depth_to_space_kernel, dim3(nblk((long)N * 4 * H * W * C, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, out_dev,
                       out_cs, N, H, W, C);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_blend_warps(const float* src0_dev, const float* src1_dev, int src_cs, const float* orig0_dev, const float* orig1_dev, int orig_cs,
                        const float* motion_dev, int motion_cs, float* out_dev, int out_cs, int H, int W, void* stream) {
    VFI_REQUIRE(src0_dev && src1_dev && motion_dev && out_dev && src_cs >= 3 && motion_cs >= 5 && out_cs >= 15 && H > 1 && W > 1 &&
                    (!orig0_dev == !orig1_dev) && (!orig0_dev || orig_cs >= 3), "vfi_atm_blend_warps: bad arguments");
    VFI_REQUIRE((long)H * W * out_cs < (1L << 31) && (long)H * W * motion_cs < (1L << 31), "vfi_atm_blend_warps: a %dx%d frame is beyond the kernel's index arithmetic", H, W);
    TraceScope ts("atm_blend", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_blend_kernel, dim3(nblk((long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, src0_dev, src1_dev, src_cs, orig0_dev, orig1_dev,
                       orig_cs, motion_dev, motion_cs, out_dev, out_cs, H, W);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_refine_out(const float* it_dev, int it_cs, const float* res_dev, int res_cs, float* out_dev, int Hp, int Wp, int pad_top, int pad_left, int H,
                       int W, void* stream) {
    VFI_REQUIRE(it_dev && res_dev && out_dev && it_cs >= 3 && res_cs >= 3 && H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0 && pad_top + H <= Hp &&
                    pad_left + W <= Wp, "vfi_atm_refine_out: bad arguments (the %dx%d crop at (%d, %d) must lie inside %dx%d)", H, W, pad_top, pad_left, Hp, Wp);
    VFI_REQUIRE((long)Hp * Wp * it_cs < (1L << 31) && (long)Hp * Wp * res_cs < (1L << 31), "vfi_atm_refine_out: a %dx%d frame is beyond the kernel's index arithmetic", Hp, Wp);
    TraceScope ts("atm_out", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_out_kernel, dim3(nblk((long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, it_dev, it_cs, res_dev, res_cs, out_dev, Wp, pad_top,
                       pad_left, H, W);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t vfi_atm_alignment_scratch_floats(int Hp, int Wp) { return Hp > 0 && Wp > 0 ? ((int64_t)Hp * Wp + kLossBlock - 1) / kLossBlock : 0; }

int vfi_atm_alignment_loss(const float* pair_dev, int pair_cs, int Hp, int Wp, const float* motion_dev, int motion_cs, int h, int w, float* scratch_dev,
                           float* loss_dev, void* stream) {
    VFI_REQUIRE(pair_dev && motion_dev && scratch_dev && loss_dev && pair_cs >= 3 && motion_cs >= 4 && h > 0 && w > 0 && Hp > 1 && Wp > 1,
                "vfi_atm_alignment_loss: bad arguments");
    VFI_REQUIRE(Hp % h == 0 && Wp % w == 0 && Hp / h == Wp / w, "vfi_atm_alignment_loss: a %dx%d frame is no whole multiple of the %dx%d motion map (one "
                "factor for both sides)", Hp, Wp, h, w);
    VFI_REQUIRE((long)2 * Hp * Wp * pair_cs < (1L << 31) && (long)h * w * motion_cs < (1L << 31),
                "vfi_atm_alignment_loss: a %dx%d frame is beyond the kernel's index arithmetic", Hp, Wp);
    TraceScope ts("atm_alignment_loss", (hipStream_t)stream);
    const int blocks = (int)vfi_atm_alignment_scratch_floats(Hp, Wp);
    hipLaunchKernelGGL(atm_alignment_partial_kernel, dim3(blocks), dim3(kLossBlock), 0, (hipStream_t)stream, pair_dev, pair_cs, Hp, Wp, motion_dev, motion_cs,
                       h, w, (float)(Hp / h), scratch_dev);
    VFI_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(atm_alignment_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)scratch_dev, blocks, 3.0 * Hp * Wp, loss_dev);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_atm_select_flow(const float* losses_dev, const float* motion0_dev, const float* motion1_dev, const float* motion2_dev, int motion_cs, int h16,
                        int w16, float* out_dev, int out_cs, float* record_dev, void* stream) {
    VFI_REQUIRE(losses_dev && motion0_dev && motion1_dev && motion2_dev && out_dev && motion_cs >= 4 && out_cs >= 4 && h16 >= 4 && w16 >= 4,
                "vfi_atm_select_flow: bad arguments (a %dx%d map: both sides at least 4, level k is [h16 >> k, w16 >> k])", h16, w16);
    VFI_REQUIRE((long)h16 * w16 * out_cs < (1L << 31) && (long)h16 * w16 * motion_cs < (1L << 31),
                "vfi_atm_select_flow: a %dx%d map is beyond the kernel's index arithmetic", h16, w16);
    TraceScope ts("atm_select_flow", (hipStream_t)stream);
    hipLaunchKernelGGL(atm_select_flow_kernel, dim3(nblk((long)h16 * w16, 256)), dim3(256), 0, (hipStream_t)stream, losses_dev, motion0_dev, motion1_dev,
                       motion2_dev, motion_cs, h16, w16, out_dev, out_cs, record_dev);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- the network object: ATM-lite / ATM-base on csrc/net_object.h --------------------------------------------------------------------------------------

namespace {

constexpr int kMotion = 5, kTensors = 232;

// What tells ATM-lite (network_lite.py:88-273) and ATM-base (network_base.py:88-260) apart; the module tree, the 232 tensors and the forward are
// shared.  local_c = hid[3] + hid[2] + 2 hid[1] tokens on the 1/8 map, last = last_feat_extract's width, global_c = last + hid[3] + 2 hid[2] on
// the 1/16 map.  px_floats: the widest per-image buffer in floats per padded pixel (the layers index one image with 32 bits of bytes).  lite:
// the refinement net's input, local_c / 4 + 5 + 15 = 76 channels padded to 80 (its 2 ref_hid = 64-channel concat buffer is narrower).  base:
// the refinement net's full-resolution concat buffer (up3 | proj), 2 ref_hid = 128 channels; its input is 116 padded to 120, the last
// up-sampling level's taps r8(4 * 101) / 4 = 102, the 4 C MLP buffers 1536 / 64.  The limit is signed (every object as created) or unsigned
// (after vfi_atm_set_large_frames: every layer that meets an image of 2 GiB or more has a large-image form, docs/design/atm.md "4K").
struct Cfg {
    int hid[4], local_c, global_c, last, mlp_ratio, local_head, global_head, ref_hid, px_floats;
    const char* name;
};
const Cfg kCfg[2] = {{{16, 32, 64, 96}, 224, 352, 128, 2, 224, 352, 32, 80, "ATM-lite"},
                     {{24, 48, 96, 192}, 384, 672, 288, 4, 576, 768, 64, 128, "ATM-base"}};

struct Fusion {       // CrossScaleFeatureFusion: three tap-gathered convolutions as 1x1 layers, proj, norm
    vfi_conv_t *l[3] = {}, *proj = nullptr;
    float *nw = nullptr, *nb = nullptr;
};
struct Block {        // ATMFormer (cross) / RefineBottleneck
    float *n1w = nullptr, *n1b = nullptr, *n2w = nullptr, *n2b = nullptr, *m0w = nullptr, *m0b = nullptr, *m2w = nullptr, *m2b = nullptr, *dww = nullptr,
          *dwb = nullptr;
    vfi_conv_t *q = nullptr, *kv = nullptr, *qkv = nullptr, *proj = nullptr, *fc1 = nullptr, *fc2 = nullptr;
};
struct Head {         // a motion head: two 3x3 + PReLU, one 1x1
    vfi_conv_t* c[3] = {};
};
struct Up {           // a level of upsample_pyramid
    float* pre = nullptr;      // the PReLU in front (levels 1, 2)
    vfi_conv_t *de = nullptr, *c1 = nullptr, *c2 = nullptr;
    int cin = 0, c = 0;
};

}  // namespace

struct vfi_atm : PaddedNet {
    vfi_conv_t* fe[4][2] = {};
    vfi_conv_t* last[2] = {};
    Fusion lf, gf;
    Block enh[2], loc[2], glo[2];
    Head lh, gh;
    Up up[3];
    vfi_conv_t *proj = nullptr, *down1 = nullptr, *down2[2] = {}, *down3[3] = {}, *up1d = nullptr, *up1c = nullptr, *up2d = nullptr, *up2c = nullptr,
               *up3d = nullptr, *rh[2] = {};
    int variant = 0;
    bool large = false;      // vfi_atm_set_large_frames: padded frames up to max_padded_pixels_large(px_floats) are served
    // the ensemble's device record: [0..2] the three losses and [3] the chosen level as vfi_atm_select_flow wrote them, [4..6] the losses as the
    // scoring kernels wrote them; ens_ran: an ensemble forward has been enqueued on ens_stream
    float* ens_rec = nullptr;
    hipStream_t ens_stream = nullptr;
    bool ens_ran = false;
};

namespace {

struct Run : NetRun<vfi_atm> {
    int copy(const float* in, int ics, float* out, int ocs, long px, int C, const float* slopes = nullptr) {
        hipLaunchKernelGGL(atm_copy_kernel, dim3(nblk(px * C, 256)), dim3(256), 0, st, in, ics, slopes, out, ocs, px, C);
        VFI_CHECK_HIP(hipGetLastError());
        return 0;
    }
    // ConvTranspose2d(k 2, s 2) + PReLU: the 1x1 layer with 4 c outputs (slopes repeated per tap), then the interleave
    int deconv(const vfi_conv_t* L, int c, const float* in, int ics, int h, int w, float* out, int ocs) {
        float* t = buf("deconv_taps", 1, h, w, r8(4 * c));
        if (bad) return -1;
        VFI_DO(conv(L, in, ics, h, w, t, r8(4 * c), 1, 3));
        return vfi_atm_depth_to_space2(t, r8(4 * c), out, ocs, 1, h, w, c, st);
    }
};

// CrossScaleFeatureFusion (network_lite.py:34-85) into `cat` [2,h,w,C], whose last channels already hold the coarsest map: mid (c1 channels, twice
// the size) and fine (c0 channels, four times the size) -> tokens tok [2 h (+1 zero row), w, C] after proj and the LayerNorm
int run_fusion(Run& r, const Fusion& F, const float* fine, int fine_cs, int c0, const float* mid, int mid_cs, int c1, float* cat, int C, int h, int w,
               float* tok) {
    float *t1 = r.buf("fus_taps1", 2, h, w, 9 * c1), *t0 = r.buf("fus_taps0", 2, h, w, 9 * c0), *pr = r.buf("fus_proj", 2, h, w, C);
    if (r.bad) return -1;
    VFI_DO(vfi_atm_gather_taps(mid, mid_cs, t1, 9 * c1, 2, 2 * h, 2 * w, c1, 2, 1, r.st));
    VFI_DO(r.conv(F.l[0], t1, 9 * c1, h, w, cat, C, 2, 0));
    for (int d = 1; d <= 2; ++d) {
        VFI_DO(vfi_atm_gather_taps(fine, fine_cs, t0, 9 * c0, 2, 4 * h, 4 * w, c0, 4, d, r.st));
        VFI_DO(r.conv(F.l[d], t0, 9 * c0, h, w, cat + c1 + (d - 1) * c0, C, 2, 0));
    }
    VFI_DO(r.conv(F.proj, cat, C, h, w, pr, C, 2, 0));
    return vfi_layernorm(pr, C, C, (int64_t)2 * h * w, F.nw, F.nb, tok, C, r.st);
}

// One windowed block on tok [2 h + 1 rows, w, C] (the last row is zero: the pad token) -> out (same layout, 2 h rows written).  cross: the motion
// read-out goes to mot[f * 2 + p * mot_cs + {0, 1}].  lab_h x lab_w: the map the pad labels come from (0: h x w, the block's own).
int run_block(Run& r, const Block& B, const float* tok, float* out, int h, int w, int C, int win, int shift, bool cross, float* mot, int mot_cs,
              int lab_h = 0, int lab_w = 0) {
    const int rows = 2 * h + 1;
    const long ntok = (long)2 * h * w;
    float *xn = r.buf("blk_xn", 1, rows, w, C), *qkv = r.buf("blk_qkv", 1, rows, w, 3 * C), *ao = r.buf("blk_ao", 2, h, w, C);
    float *of = r.buf("blk_offs", 2, h, w, 2 * kHeads), *y = r.buf("blk_y", 2, h, w, C), *t2 = r.buf("blk_t2", 2, h, w, C);
    const int M = kCfg[r.m->variant].mlp_ratio * C;      // Mlp's hidden width
    float *h1 = r.buf("blk_h1", 2, h, w, M), *h2 = r.buf("blk_h2", 2, h, w, M);
    if (r.bad) return -1;
    VFI_DO(vfi_layernorm(tok, C, C, (int64_t)rows * w, B.n1w, B.n1b, xn, C, r.st));
    if (cross) {
        VFI_DO(r.conv(B.q, xn, C, rows, w, qkv, 3 * C, 1, 0));
        VFI_DO(r.conv(B.kv, xn, C, rows, w, qkv + C, 3 * C, 1, 0));
    } else {
        VFI_DO(r.conv(B.qkv, xn, C, rows, w, qkv, 3 * C, 1, 0));
    }
    VFI_DO(vfi_atm_window_attention_labels(qkv, 3 * C, qkv + C, 3 * C, qkv + 2 * C, 3 * C, ntok, ao, C, cross ? of : nullptr, h, w, lab_h ? lab_h : h,
                                           lab_w ? lab_w : w, C, win, shift, cross, r.st));
    if (cross) VFI_DO(vfi_atm_motion_mlp(of, B.m0w, B.m0b, B.m2w, B.m2b, mot, mot_cs, 2, (int64_t)h * w, r.st));
    VFI_DO(r.conv(B.proj, ao, C, 2 * h, w, y, C, 1, 0, xn, C));      // norm1(x) + proj(attention): the residual is the NORMED token
    VFI_DO(vfi_layernorm(y, C, C, ntok, B.n2w, B.n2b, t2, C, r.st));
    VFI_DO(r.conv(B.fc1, t2, C, 2 * h, w, h1, M, 1, 0));
    VFI_DO(vfi_atm_dwconv3x3_gelu(h1, M, B.dww, B.dwb, h2, M, 2, h, w, M, r.st));
    return r.conv(B.fc2, h2, M, 2 * h, w, out, C, 1, 0, y, C);
}

// two ATM blocks and the motion head (hidden width Ch): tok -> tok (in place through a second buffer), out5 [h,w,8] = (flow0 xy, flow1 xy, mask logit).
// lab_h x lab_w: the pad-label map of the SHIFTED block (0: its own)
int run_motion(Run& r, const Block* B, const Head& H, float* tok, float* tok2, int h, int w, int C, int Ch, int win, float* out5, int lab_h = 0,
               int lab_w = 0) {
    const int mcs = 2 * kHeads / 2 + 2 * C;      // 8 motion channels | frame 0 tokens | frame 1 tokens
    float *mh = r.buf("mh_in", 1, h, w, mcs), *a = r.buf("mh_a", 1, h, w, Ch), *b = r.buf("mh_b", 1, h, w, Ch);
    if (r.bad) return -1;
    VFI_DO(run_block(r, B[0], tok, tok2, h, w, C, win, 0, true, mh, mcs));
    VFI_DO(run_block(r, B[1], tok2, tok, h, w, C, win, win / 2, true, mh + 4, mcs, lab_h, lab_w));
    const long px = (long)h * w;
    VFI_DO(r.copy(tok, C, mh + 8, mcs, px, C));
    VFI_DO(r.copy(tok + (size_t)px * C, C, mh + 8 + C, mcs, px, C));
    VFI_DO(r.conv(H.c[0], mh, mcs, h, w, a, Ch, 1, 3));
    VFI_DO(r.conv(H.c[1], a, Ch, h, w, b, Ch, 1, 3));
    return r.conv(H.c[2], b, Ch, h, w, out5, 8, 1, 0);
}

// The four feature-extractor stages on an image pair x [2,h0,w0,8] (h0 x w0 = the size of level `first` of hs / wsz): stage i -> f[i], channel
// stride fcs[i].  Scratch names carry the level, so that the ensemble's smaller passes keep buffers of their own.
int run_features(Run& r, const float* x, const int* hs, const int* wsz, int first, float* const* f, const int* fcs) {
    const Cfg& g = kCfg[r.m->variant];
    static const char* an[3][4] = {{"fe_a0", "fe_a1", "fe_a2", "fe_a3"}, {"e1_fe_a0", "e1_fe_a1", "e1_fe_a2", "e1_fe_a3"}, {"e2_fe_a0", "e2_fe_a1", "e2_fe_a2", "e2_fe_a3"}};
    int xcs = 8;
    for (int i = 0; i < 4; ++i) {
        const int hi = hs[first + (i ? i - 1 : 0)], wi = wsz[first + (i ? i - 1 : 0)], ho = hs[first + i], wo = wsz[first + i], c = g.hid[i];
        float* a = r.buf(an[first][i], 2, ho, wo, c);
        if (r.bad) return -1;
        VFI_DO(r.conv(r.m->fe[i][0], x, xcs, hi, wi, a, c, 2, 3));
        VFI_DO(r.conv(r.m->fe[i][1], a, c, ho, wo, f[i], fcs[i], 2, 3));
        x = f[i], xcs = fcs[i];
    }
    return 0;
}

// estimate_global_motion (network_lite.py:383-407) at one image level: last_feat_extract on the stage-3 features f3 [2,2h,2w] (channel stride
// f3cs), the global fusion with the stage-2 features fine [2,4h,4w,hid[2]], the two ATM blocks (window 12) and the motion head -> out5 [h,w,8] =
// (flow0 xy, flow1 xy, mask logit) on this level's h x w map.  Scratch is keyed by size: every level has its own.  lab_h x lab_w: run_motion's.
int run_global(Run& r, const float* fine, const float* f3, int f3cs, int h, int w, float* out5, int lab_h = 0, int lab_w = 0) {
    vfi_atm* m = r.m;
    const Cfg& g = kCfg[m->variant];
    const int CG = g.global_c;
    float *g0 = r.buf("gl_a", 2, h, w, g.last), *cat_g = r.buf("cat_g", 2, h, w, CG);
    float *gtok = r.buf("gtok_a", 1, 2 * h + 1, w, CG), *gtok2 = r.buf("gtok_b", 1, 2 * h + 1, w, CG);
    if (r.bad) return -1;
    VFI_DO(r.conv(m->last[0], f3, f3cs, 2 * h, 2 * w, g0, g.last, 2, 3));
    VFI_DO(r.conv(m->last[1], g0, g.last, h, w, cat_g + (CG - g.last), CG, 2, 3));
    VFI_DO(run_fusion(r, m->gf, fine, g.hid[2], g.hid[2], f3, f3cs, g.hid[3], cat_g, CG, h, w, gtok));
    return run_motion(r, m->glo, m->gh, gtok, gtok2, h, w, CG, g.global_head, 12, out5, lab_h, lab_w);
}

// mode: 0 = "Off (fastest)", 1 = "On", 2 = "On with Ensemble (slowest)"
int atm_forward(vfi_atm* m, const float* f0, const float* f1, int Cf, int H, int W, int mode, float* out, hipStream_t st) {
    const Cfg& g = kCfg[m->variant];
    const int CL = g.local_c, CG = g.global_c;      // the local / global token widths
    const int rcs = r8(CL / 4 + kMotion + 15);      // the refinement net's input: 76 -> 80 / 116 -> 120 floats per pixel
    const int Hp = m->Hp, Wp = m->Wp, top = (Hp - H) / 2, left = (Wp - W) / 2;
    const int hs[7] = {Hp, Hp / 2, Hp / 4, Hp / 8, Hp / 16, Hp / 32, Hp / 64}, wsz[7] = {Wp, Wp / 2, Wp / 4, Wp / 8, Wp / 16, Wp / 32, Wp / 64};
    const int h8 = hs[3], w8 = wsz[3], h16 = hs[4], w16 = wsz[4];
    Run r{{m, st}};
    // padded frames and their x0.5 pyramids (bilinear, align_corners=True)
    float* pyr[4];
    const char* pyr_names[4] = {"img0", "img1", "img2", "img3"};
    for (int i = 0; i < 4; ++i) pyr[i] = r.buf(pyr_names[i], 2, hs[i], wsz[i], 8);
    if (r.bad) return -1;
    VFI_DO(pad_frame_pair(f0, f1, Cf, H, W, pyr[0], Hp, Wp, top, left, true, st));      // InputPadder(dims, 64) (atm/__init__.py:11-23): centred, replicate
    for (int i = 1; i < 4; ++i) VFI_DO(vfi_resize_bilinear_ac(pyr[i - 1], 8, pyr[i], 8, 2, hs[i - 1], wsz[i - 1], hs[i], wsz[i], 3, 1.0f, st));
    // feature extraction on both frames; the 1/8 map lands in the last hid[3] channels of the local fusion's concat buffer
    float* cat_l = r.buf("cat_l", 2, h8, w8, CL);
    if (r.bad) return -1;
    float* feat[4] = {r.buf("fe_f0", 2, hs[0], wsz[0], g.hid[0]), r.buf("fe_f1", 2, hs[1], wsz[1], g.hid[1]), r.buf("fe_f2", 2, hs[2], wsz[2], g.hid[2]),
                      cat_l + (CL - g.hid[3])};
    const int fcs[4] = {g.hid[0], g.hid[1], g.hid[2], CL};
    if (r.bad) return -1;
    VFI_DO(run_features(r, pyr[0], hs, wsz, 0, feat, fcs));
    const float* f3 = feat[3];
    float *tok = r.buf("tok_a", 1, 2 * h8 + 1, w8, CL), *tok2 = r.buf("tok_b", 1, 2 * h8 + 1, w8, CL);
    if (r.bad) return -1;
    VFI_DO(run_fusion(r, m->lf, feat[1], g.hid[1], g.hid[1], feat[2], g.hid[2], g.hid[2], cat_l, CL, h8, w8, tok));
    const float *src0 = pyr[0], *src1 = pyr[0] + (size_t)Hp * Wp * 8;      // what the last synthesis step warps
    if (mode) {
        float* g5 = r.buf("gl_out5", 1, h16, w16, 8);
        if (r.bad) return -1;
        VFI_DO(run_global(r, feat[2], f3, CL, h16, w16, g5));
        if (mode == 2) {
            // multiscale_global_motion_ensemble (network_lite.py:556-597): level 0 is g5 (the reference recomputes the same features from the
            // same input); levels 1 and 2 run the feature extractor and the global branch on pyr[1] / pyr[2], the x0.5 images it feeds them.
            // The shifted block of a level whose map pads to the previous level's layout is masked with that level's pad regions, as the
            // reference's cached mask makes it (attention.py:279-305; tests/atm_ensemble_restated.py: mask_level).
            float* lev[3] = {g5, nullptr, nullptr};
            int lab = 0;      // the level whose map the shifted block's pad labels come from
            for (int k = 1; k <= 2; ++k) {
                const int hk = hs[4 + k], wk = wsz[4 + k];
                if (round_up(hk, 12) != round_up(hs[3 + k], 12) || round_up(wk, 12) != round_up(wsz[3 + k], 12)) lab = k;
                static const char *fn[2][4] = {{"e1_fe_f0", "e1_fe_f1", "e1_fe_f2", "e1_fe_f3"}, {"e2_fe_f0", "e2_fe_f1", "e2_fe_f2", "e2_fe_f3"}};
                float* ef[4];
                for (int i = 0; i < 4; ++i) ef[i] = r.buf(fn[k - 1][i], 2, hs[k + i], wsz[k + i], g.hid[i]);
                lev[k] = r.buf("ens_out5", 1, hk, wk, 8);
                if (r.bad) return -1;
                VFI_DO(run_features(r, pyr[k], hs, wsz, k, ef, g.hid));
                VFI_DO(run_global(r, ef[2], ef[3], g.hid[3], hk, wk, lev[k], hs[4 + lab], wsz[4 + lab]));
            }
            float *part = r.buf("ens_partial", 1, 1, 1, (int)vfi_atm_alignment_scratch_floats(Hp, Wp)), *sel = r.buf("ens_sel5", 1, h16, w16, 8);
            if (r.bad) return -1;
            for (int k = 0; k < 3; ++k) VFI_DO(vfi_atm_alignment_loss(pyr[0], 8, Hp, Wp, lev[k], 8, hs[4 + k], wsz[4 + k], part, m->ens_rec + 4 + k, st));
            VFI_DO(vfi_atm_select_flow(m->ens_rec + 4, lev[0], lev[1], lev[2], 8, h16, w16, sel, 8, m->ens_rec, st));
            m->ens_stream = st, m->ens_ran = true;
            g5 = sel;      // channels 0..3: the winner's flows; the global-level mask logit is not read
        }
        // the global flows, x2 per level up to full resolution; the tokens and every pyramid level are warped by them
        float* fl[4];
        const char* fl_names[4] = {"gl_fl0", "gl_fl1", "gl_fl2", "gl_fl3"};
        for (int i = 0; i < 4; ++i) fl[i] = r.buf(fl_names[i], 1, hs[i], wsz[i], 4);
        float* wp[4];
        const char* wp_names[4] = {"wimg0", "wimg1", "wimg2", "wimg3"};
        for (int i = 0; i < 4; ++i) wp[i] = r.buf(wp_names[i], 2, hs[i], wsz[i], 8);
        if (r.bad) return -1;
        VFI_DO(vfi_resize_bilinear_ac(g5, 8, fl[3], 4, 1, h16, w16, h8, w8, 4, 2.0f, st));
        const size_t p8 = (size_t)h8 * w8;
        VFI_DO(vfi_flow_sample(tok, CL, fl[3], 4, tok2, CL, 1, h8, w8, CL, st));
        VFI_DO(vfi_flow_sample(tok + p8 * CL, CL, fl[3] + 2, 4, tok2 + p8 * CL, CL, 1, h8, w8, CL, st));
        float* t = tok;
        tok = tok2, tok2 = t;
        for (int i = 3; i >= 0; --i) {
            const size_t px = (size_t)hs[i] * wsz[i];
            VFI_DO(vfi_flow_sample(pyr[i], 8, fl[i], 4, wp[i], 8, 1, hs[i], wsz[i], 3, st));
            VFI_DO(vfi_flow_sample(pyr[i] + px * 8, 8, fl[i] + 2, 4, wp[i] + px * 8, 8, 1, hs[i], wsz[i], 3, st));
            if (i) VFI_DO(vfi_resize_bilinear_ac(fl[i], 4, fl[i - 1], 4, 1, hs[i], wsz[i], hs[i - 1], wsz[i - 1], 4, 2.0f, st));
        }
        src0 = wp[0], src1 = wp[0] + (size_t)Hp * Wp * 8;
    }
    // local motion, feature enhancement
    float* o5 = r.buf("lo_out5", 1, h8, w8, 8);
    if (r.bad) return -1;
    VFI_DO(run_motion(r, m->loc, m->lh, tok, tok2, h8, w8, CL, g.local_head, 8, o5));
    VFI_DO(run_block(r, m->enh[0], tok, tok2, h8, w8, CL, 8, 0, false, nullptr, 0));
    VFI_DO(run_block(r, m->enh[1], tok2, tok, h8, w8, CL, 8, 4, false, nullptr, 0));
    // (warped frame 0 tokens | warped frame 1 tokens | the 5 motion channels), then the three up-sampling levels
    const int c0cs = r8(2 * CL + kMotion);
    float* fcat = r.buf("up_in", 1, h8, w8, c0cs);
    if (r.bad) return -1;
    {
        const size_t p8 = (size_t)h8 * w8;
        VFI_DO(vfi_flow_sample(tok, CL, o5, 8, fcat, c0cs, 1, h8, w8, CL, st));
        VFI_DO(vfi_flow_sample(tok + p8 * CL, CL, o5 + 2, 8, fcat + CL, c0cs, 1, h8, w8, CL, st));
        VFI_DO(r.copy(o5, 8, fcat + 2 * CL, c0cs, (long)p8, kMotion));
    }
    float* R = r.buf("ref_in", 1, Hp, Wp, rcs);      // (feat local_c / 4 + 5 | im0 | warped 0 | im1 | warped 1 | I_t)
    float* lvl[3] = {nullptr, nullptr, R};
    int lcs[3] = {0, 0, rcs};
    {
        const float* x = fcat;
        int xcs = c0cs;
        const char *pn[3] = {"up_pre0", "up_pre1", "up_pre2"}, *dn[3] = {"up_d0", "up_d1", "up_d2"}, *cn[3] = {"up_c0", "up_c1", "up_c2"}, *on[2] = {"up_o0", "up_o1"};
        for (int i = 0; i < 3; ++i) {
            const Up& U = m->up[i];
            const int h = hs[3 - i], w = wsz[3 - i], ccs = r8(U.c);
            if (U.pre) {
                float* p = r.buf(pn[i], 1, h, w, r8(U.cin));
                if (r.bad) return -1;
                VFI_DO(r.copy(x, xcs, p, r8(U.cin), (long)h * w, U.cin, U.pre));
                x = p, xcs = r8(U.cin);
            }
            float *d = r.buf(dn[i], 1, 2 * h, 2 * w, ccs), *c = r.buf(cn[i], 1, 2 * h, 2 * w, ccs);
            if (i < 2) lvl[i] = r.buf(on[i], 1, 2 * h, 2 * w, ccs), lcs[i] = ccs;
            if (r.bad) return -1;
            VFI_DO(r.deconv(U.de, U.c, x, xcs, h, w, d, ccs));
            VFI_DO(r.conv(U.c1, d, ccs, 2 * h, 2 * w, c, ccs, 1, 3));
            VFI_DO(r.conv(U.c2, c, ccs, 2 * h, 2 * w, lvl[i], lcs[i], 1, 0));
            x = lvl[i], xcs = lcs[i];
        }
    }
    const int fc = CL / 4 + kMotion;      // 61 / 101
    VFI_DO(vfi_atm_blend_warps(src0, src1, 8, pyr[0], pyr[0] + (size_t)Hp * Wp * 8, 8, R + fc - kMotion, rcs, R + fc, rcs, Hp, Wp, st));
    // residual refinement (network_lite.py:409-423), hidden width hd; concat buffers: c6 = (u0 | r0), c2 = (r1 | skip 1/2), c3 = (r2 | skip 1/4),
    // c4 = (u2 | r2), c5 = (u1 | r1)
    const int h2 = hs[1], w2 = wsz[1], h4 = hs[2], w4 = wsz[2];
    const int hd = g.ref_hid, s2 = hd + CL / 2, s3 = 2 * hd + CL;      // the channel strides of c2 and c3
    float *c6 = r.buf("rf_c6", 1, Hp, Wp, 2 * hd), *c2 = r.buf("rf_c2", 1, h2, w2, s2), *c3 = r.buf("rf_c3", 1, h4, w4, s3), *c4 = r.buf("rf_c4", 1, h4, w4, 4 * hd);
    float *c5 = r.buf("rf_c5", 1, h2, w2, 2 * hd), *d2 = r.buf("rf_d2", 1, h4, w4, 2 * hd), *d3a = r.buf("rf_d3a", 1, h8, w8, 4 * hd), *d3b = r.buf("rf_d3b", 1, h8, w8, 4 * hd);
    float *u2 = r.buf("rf_u2", 1, h4, w4, 2 * hd), *u1 = r.buf("rf_u1", 1, h2, w2, 2 * hd), *rh = r.buf("rf_h", 1, Hp, Wp, hd), *res = r.buf("rf_res", 1, Hp, Wp, 8);
    if (r.bad) return -1;
    VFI_DO(r.conv(m->proj, R, rcs, Hp, Wp, c6 + hd, 2 * hd, 1, 3));
    VFI_DO(r.conv(m->down1, c6 + hd, 2 * hd, Hp, Wp, c2, s2, 1, 3));
    VFI_DO(r.copy(lvl[1], lcs[1], c2 + hd, s2, (long)h2 * w2, CL / 2));
    VFI_DO(r.conv(m->down2[0], c2, s2, h2, w2, d2, 2 * hd, 1, 3));
    VFI_DO(r.conv(m->down2[1], d2, 2 * hd, h4, w4, c3, s3, 1, 3));
    VFI_DO(r.copy(lvl[0], lcs[0], c3 + 2 * hd, s3, (long)h4 * w4, CL));
    VFI_DO(r.copy(c3, s3, c4 + 2 * hd, 4 * hd, (long)h4 * w4, 2 * hd));
    VFI_DO(r.copy(c2, s2, c5 + hd, 2 * hd, (long)h2 * w2, hd));
    VFI_DO(r.conv(m->down3[0], c3, s3, h4, w4, d3a, 4 * hd, 1, 3));
    VFI_DO(r.conv(m->down3[1], d3a, 4 * hd, h8, w8, d3b, 4 * hd, 1, 3));
    VFI_DO(r.conv(m->down3[2], d3b, 4 * hd, h8, w8, d3a, 4 * hd, 1, 3));
    VFI_DO(r.deconv(m->up1d, 2 * hd, d3a, 4 * hd, h8, w8, u2, 2 * hd));
    VFI_DO(r.conv(m->up1c, u2, 2 * hd, h4, w4, c4, 4 * hd, 1, 3));
    VFI_DO(r.deconv(m->up2d, 2 * hd, c4, 4 * hd, h4, w4, u1, 2 * hd));
    VFI_DO(r.conv(m->up2c, u1, 2 * hd, h2, w2, c5, 2 * hd, 1, 3));
    VFI_DO(r.deconv(m->up3d, hd, c5, 2 * hd, h2, w2, c6, 2 * hd));
    VFI_DO(r.conv(m->rh[0], c6, 2 * hd, Hp, Wp, rh, hd, 1, 3));
    VFI_DO(r.conv(m->rh[1], rh, hd, Hp, Wp, res, 8, 1, 3));
    return vfi_atm_refine_out(R + fc + 12, rcs, res, 8, out, Hp, Wp, top, left, H, W, st);
}

int atm_pad64(int n) { return n + (((n / 64) + 1) * 64 - n) % 64; }

}  // namespace

extern "C" {

int64_t vfi_atm_max_padded_pixels(void) { return max_padded_pixels(kCfg[0].px_floats); }

int64_t vfi_atm_large_max_padded_pixels(int variant) { return variant == 0 || variant == 1 ? max_padded_pixels_large(kCfg[variant].px_floats) : 0; }

int64_t vfi_atm_object_max_padded_pixels(const vfi_atm_t* m) {
    return !m ? 0 : (m->large ? max_padded_pixels_large(kCfg[m->variant].px_floats) : max_padded_pixels(kCfg[m->variant].px_floats));
}

int vfi_atm_set_large_frames(vfi_atm_t* m, int on) {
    VFI_REQUIRE(m, "vfi_atm_set_large_frames: null object");
    m->large = on != 0;
    return 0;
}

vfi_atm_t* vfi_atm_create(const float* const* tensors, const int64_t* numels, int n_tensors) { return vfi_atm_create_variant(tensors, numels, n_tensors, 0); }

vfi_atm_t* vfi_atm_create_variant(const float* const* tensors, const int64_t* numels, int n_tensors, int variant) {
    const bool known = variant == 0 || variant == 1;
    if (!tensors || !numels || !known || n_tensors != kTensors) {
        set_error("vfi_atm_create: expected the %d weight tensors of %s in atm_spec.weight_shapes() order (variant 0 = ATM-lite, 1 = ATM-base), got %d "
                  "(variant %d)", kTensors, known ? kCfg[variant].name : "ATM-?", n_tensors, variant);
        return nullptr;
    }
    const Cfg& g = kCfg[variant];
    const int CL = g.local_c, CG = g.global_c;
    vfi_atm* m = new vfi_atm();
    m->variant = variant;
    // both variants have 232 tensors: the per-tensor element counts are what tells a file of the other model
    TensorCursor cur(tensors, numels, n_tensors, variant ? "vfi_atm_create (ATM-base)" : "vfi_atm_create (ATM-lite)");
    std::vector<float> tmp, tb, tp;
    // Conv2d(cin, cout, k, stride, padding k / 2) with bias [+ PReLU]
    auto conv = [&](int cout, int cin, int k, int stride, bool prelu, bool bias = true) { return m->read_layer(cur, 0, cout, cin, k, stride, bias, prelu); };
    // Conv2d(c, c, 3, stride s, dilation d, padding d) as a 1x1 layer over the gathered taps: input channel t c + ci
    auto tapconv = [&](int c) -> vfi_conv_t* {
        const float* w = cur.take((int64_t)c * c * 9);
        const float* b = cur.take(c);
        if (!cur.ok()) return nullptr;
        tmp.assign((size_t)c * 9 * c, 0.f);
        for (int co = 0; co < c; ++co)
            for (int ci = 0; ci < c; ++ci)
                for (int t = 0; t < 9; ++t) tmp[(size_t)co * 9 * c + t * c + ci] = w[((size_t)co * c + ci) * 9 + t];
        return m->add_layer(vfi_conv_create_ex(0, tmp.data(), b, c, 9 * c, 1, 1, 0, nullptr, 9 * c, nullptr));
    };
    // ConvTranspose2d(cin, c, 2, 2, 0) + PReLU(c) as a 1x1 layer with 4 c outputs: output channel t c + co, t = 2 ky + kx
    auto deconv = [&](int cin, int c) -> vfi_conv_t* {
        const float* w = cur.take((int64_t)cin * c * 4);
        const float* b = cur.take(c);
        const float* p = cur.take(c);
        if (!cur.ok()) return nullptr;
        tmp.assign((size_t)4 * c * cin, 0.f), tb.resize(4 * c), tp.resize(4 * c);
        for (int t = 0; t < 4; ++t)
            for (int co = 0; co < c; ++co) {
                tb[t * c + co] = b[co], tp[t * c + co] = p[co];
                for (int ci = 0; ci < cin; ++ci) tmp[((size_t)t * c + co) * cin + ci] = w[((size_t)ci * c + co) * 4 + t];
            }
        return m->add_layer(vfi_conv_create_ex(0, tmp.data(), tb.data(), 4 * c, cin, 1, 1, 0, nullptr, r8(cin), tp.data()));
    };
    auto vec = [&](int n) -> float* {
        const float* p = cur.take(n);
        return p ? m->upload(p, n) : nullptr;
    };
    auto fusion = [&](Fusion& F, int c0, int c1, int C) {
        F.l[0] = tapconv(c1), F.l[1] = tapconv(c0), F.l[2] = tapconv(c0);
        F.proj = conv(C, C, 1, 1, false);
        F.nw = vec(C), F.nb = vec(C);
    };
    auto mlp = [&](Block& B, int C) {
        B.n2w = vec(C), B.n2b = vec(C);
        const int M = g.mlp_ratio * C;
        B.fc1 = conv(M, C, 1, 1, false);
        const float* w = cur.take((int64_t)M * 9);
        if (w) {
            tmp.assign((size_t)9 * M, 0.f);
            for (int c = 0; c < M; ++c)
                for (int t = 0; t < 9; ++t) tmp[(size_t)t * M + c] = w[(size_t)c * 9 + t];
            B.dww = m->upload(tmp.data(), tmp.size());
        }
        B.dwb = vec(M);
        B.fc2 = conv(C, M, 1, 1, false);
    };
    auto atmformer = [&](Block& B, int C) {
        B.n1w = vec(C), B.n1b = vec(C);
        B.q = conv(C, C, 1, 1, false, false);
        B.kv = conv(2 * C, C, 1, 1, false, false);
        B.proj = conv(C, C, 1, 1, false);
        B.m0w = vec(kHeads / 2 * kHeads), B.m0b = vec(kHeads / 2), B.m2w = vec(kHeads / 2), B.m2b = vec(1);
        mlp(B, C);
    };
    auto head = [&](Head& Hd, int C, int Ch) {
        Hd.c[0] = conv(Ch, 2 * C + kHeads, 3, 1, true);
        Hd.c[1] = conv(Ch, Ch, 3, 1, true);
        Hd.c[2] = conv(kMotion, Ch, 1, 1, false);
    };
    int prev = 3;
    for (int i = 0; i < 4; ++i) {
        m->fe[i][0] = conv(g.hid[i], prev, 3, i ? 2 : 1, true);
        m->fe[i][1] = conv(g.hid[i], g.hid[i], 3, 1, true);
        prev = g.hid[i];
    }
    fusion(m->lf, g.hid[1], g.hid[2], CL);
    for (int k = 0; k < 2; ++k) {
        Block& B = m->enh[k];
        B.n1w = vec(CL), B.n1b = vec(CL);
        B.qkv = conv(3 * CL, CL, 1, 1, false, false);
        B.proj = conv(CL, CL, 1, 1, false);
        mlp(B, CL);
    }
    for (int k = 0; k < 2; ++k) atmformer(m->loc[k], CL);
    head(m->lh, CL, g.local_head);
    m->last[0] = conv(g.last, g.hid[3], 3, 2, true);
    m->last[1] = conv(g.last, g.last, 3, 1, true);
    fusion(m->gf, g.hid[2], g.hid[3], CG);
    for (int k = 0; k < 2; ++k) atmformer(m->glo[k], CG);
    head(m->gh, CG, g.global_head);
    int cin = 2 * CL + kMotion;
    for (int i = 0; i < 3; ++i) {
        Up& U = m->up[i];
        U.cin = cin, U.c = (CL >> i) + kMotion;
        if (i) U.pre = vec(cin);
        U.de = deconv(cin, U.c);
        U.c1 = conv(U.c, U.c, 3, 1, true);
        U.c2 = conv(U.c, U.c, 3, 1, false);
        cin = U.c;
    }
    const int hid = g.ref_hid;
    m->proj = conv(hid, CL / 4 + kMotion + 15, 3, 1, true);
    m->down1 = conv(hid, hid, 3, 2, true);
    m->down2[0] = conv(2 * hid, CL / 2 + hid, 3, 2, true);
    m->down2[1] = conv(2 * hid, 2 * hid, 3, 1, true);
    m->down3[0] = conv(4 * hid, CL + 2 * hid, 3, 2, true);
    m->down3[1] = conv(4 * hid, 4 * hid, 3, 1, true);
    m->down3[2] = conv(4 * hid, 4 * hid, 3, 1, true);
    m->up1d = deconv(4 * hid, 2 * hid);
    m->up1c = conv(2 * hid, 2 * hid, 3, 1, true);
    m->up2d = deconv(4 * hid, 2 * hid);
    m->up2c = conv(hid, 2 * hid, 3, 1, true);
    m->up3d = deconv(2 * hid, hid);
    m->rh[0] = conv(hid, 2 * hid, 3, 1, true);
    m->rh[1] = conv(3, hid, 3, 1, true);
    m->ens_rec = m->upload(nullptr, 8);
    if (!cur.finish() || m->failed) {
        vfi_atm_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_atm_destroy(vfi_atm_t* m) { delete m; }

int vfi_atm_release_workspace(vfi_atm_t* m) {
    VFI_REQUIRE(m, "vfi_atm_release_workspace: null object");
    return m->ws.release();
}

int64_t vfi_atm_workspace_bytes(const vfi_atm_t* m) { return m ? m->ws.bytes() : 0; }

namespace {

// the size guard and the workspace key of the two entry points; `who` names the caller in the refusal
int atm_enter(vfi_atm_t* m, const char* who, int H, int W) {
    const Cfg& g = kCfg[m->variant];
    return m->enter(who, g.name, H, W, atm_pad64(H), atm_pad64(W), g.px_floats, false, m->large);
}

}  // namespace

int vfi_atm_forward(vfi_atm_t* m, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, int global_motion, float* out_dev, void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && out_dev && C >= 3 && H > 0 && W > 0 && (global_motion == 0 || global_motion == 1),
                "vfi_atm_forward: bad arguments (global_motion %d: 0 off, 1 on; the multi-scale ensemble is vfi_atm_forward_ensemble's)", global_motion);
    if (const int rc = atm_enter(m, "vfi_atm_forward", H, W)) return rc;
    return atm_forward(m, frame0_dev, frame1_dev, C, H, W, global_motion, out_dev, (hipStream_t)stream);
}

int vfi_atm_forward_ensemble(vfi_atm_t* m, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float* out_dev, void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && out_dev && C >= 3 && H > 0 && W > 0, "vfi_atm_forward_ensemble: bad arguments");
    if (const int rc = atm_enter(m, "vfi_atm_forward_ensemble", H, W)) return rc;
    return atm_forward(m, frame0_dev, frame1_dev, C, H, W, 2, out_dev, (hipStream_t)stream);
}

#ifdef VFI_TEST_TAPS      // include/vfi_hip_test_atm.h: only in libvfi_hip_test.so
int vfi_atm_ensemble_record(vfi_atm_t* m, float* losses, int* level) {
    VFI_REQUIRE(m && losses && level, "vfi_atm_ensemble_record: bad arguments");
    VFI_REQUIRE(m->ens_ran, "vfi_atm_ensemble_record: no ensemble forward has run on this object");
    float rec[4];
    VFI_CHECK_HIP(hipStreamSynchronize(m->ens_stream));
    VFI_CHECK_HIP(hipMemcpy(rec, m->ens_rec, sizeof(rec), hipMemcpyDeviceToHost));
    losses[0] = rec[0], losses[1] = rec[1], losses[2] = rec[2], *level = (int)rec[3];
    return 0;
}
#endif  // VFI_TEST_TAPS

}  // extern "C"
