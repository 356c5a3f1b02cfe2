// AMT (vfi_models/amt/amt_arch.py AMT_S / AMT_L / AMT_G): the kernels the network needs beyond the shared layer objects, and the network object
// (vfi_amt_create / _forward / ..., at the end of the file) that runs one frame pair at n timesteps over them.
//
//   amt_pool2 / amt_lookup   the bidirectional correlation lookup WITHOUT the all-pairs volume (BidirCorrBlock, :1076-1141)
//   conv7x7                  7x7 stride-1 zero-padded convolution for thin layers (convf1, AMT-L's comb_block)
//   amt_warps / amt_out      multi_flow_combine around comb_block (:869-902), clamp and un-pad
//   amt_mean_* / amt_center  mean_ over the padded pair (deterministic), its subtraction; the pad itself is net_object.h's pad_frame_pair
//   amt_upsample_lrelu       leaky_relu(bilinear x2 / x4 up-sampling) in one pass: AMT-G's update*_high blocks after their commuted convc1
//   amt_add / amt_warp       residual sums, channel-window and stride-2 copies; amt_arch.warp of a feature window (rife_warp.h's taps)
//
// Built with -ffp-contract=off (csrc/build.py): coordinates are coord + flow * scale as two roundings, as torch computes them; the dot
// products and convolutions ask for their fmas by name.
#include <cstring>

#include "../../include/vfi_hip.h"
#include "../../include/vfi_hip_test_amt.h"
#include "bilinear_src.h"
#include "net_object.h"
#include "rife_warp.h"
#include "vfi_common.h"

namespace vfi {
namespace {

constexpr int kLevels = 4, kRadius = 3, kWin = 2 * kRadius + 1, kNb = kWin + 1;   // 7x7 taps from an 8x8 integer neighbourhood
constexpr int kMaxD = 256;

// out [hin/2][win/2][D] = avg_pool2d(in [hin][win][D], 2, stride 2): odd rows / columns at the end are dropped
__global__ void amt_pool2_kernel(const float* __restrict__ in, float* __restrict__ out, int hin, int win, int D4) {
    const int ho = hin >> 1, wo = win >> 1;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)ho * wo * D4) return;
    const int d = (int)(idx % D4);
    const long p = idx / D4;
    const int x = (int)(p % wo), y = (int)(p / wo);
    const float4* r0 = (const float4*)in + ((size_t)(2 * y) * win + 2 * x) * D4 + d;
    const float4* r1 = r0 + (size_t)win * D4;
    const float4 a = r0[0], b = r0[D4], c = r1[0], e = r1[D4];
    float4 o;
    o.x = ((a.x + b.x) + (c.x + e.x)) * 0.25f;
    o.y = ((a.y + b.y) + (c.y + e.y)) * 0.25f;
    o.z = ((a.z + b.z) + (c.z + e.z)) * 0.25f;
    o.w = ((a.w + b.w) + (c.w + e.w)) * 0.25f;
    ((float4*)out)[idx] = o;
}

// One workgroup per query pixel q, one wave per pyramid level.  The level's 8x8 integer neighbourhood around floor(c(q) / 2^lvl) needs 64
// dot products <fq[q], ft_lvl[p]> over D channels.  Eight lanes share a position: lane `sub` of the eight takes the float4 slices sub,
// sub + 8, ... of the target vector, so the eight read one contiguous 128-byte piece per load, and a wave's load covers eight neighbouring
// positions of one neighbourhood row (D contiguous floats each, the row 8 D contiguous floats): a load touches about eight cache lines,
// where one lane per position touched 64 and the kernel ran at the L1's line rate.  The query vector is staged in LDS (eight distinct
// 16-byte reads per wave, broadcast over the positions); the eight partial sums meet in three xor-shuffles.  Positions outside the map
// contribute 0 (grid_sample's zero padding).  The 256 dots go through LDS; 196 lanes then blend their four neighbours with
// the level's pair of fractions, which all 49 taps share because the taps are one pixel apart, and store the query's 196 channels
// contiguously.
__global__ __launch_bounds__(256) void amt_lookup_kernel(const float* __restrict__ fq, const float* __restrict__ ft0,
                                                         const float* __restrict__ ftp, const float* __restrict__ flow, int flow_cs,
                                                         float scale, float inv_sqrt_d, int h, int w, int D, float* __restrict__ out,
                                                         int out_cs) {
    __shared__ __attribute__((aligned(16))) float q_s[kMaxD];
    __shared__ float g_s[kLevels][kNb][kNb + 1];
    const int tid = threadIdx.x;
    const int qi = blockIdx.x;
    const int qx = qi % w, qy = qi / w;
    for (int i = tid; i < D; i += 256) q_s[i] = fq[(size_t)qi * D + i];
    const float* fl = flow + (size_t)qi * flow_cs;
    const float cx = (float)qx + fl[0] * scale, cy = (float)qy + fl[1] * scale;      // two roundings each (no contraction)
    {
        const int lvl = tid >> 6, gx = (tid >> 3) & 7, sub = tid & 7;
        const int hl = h >> lvl, wl = w >> lvl, D4 = D >> 2;
        const float s = 1.0f / (float)(1 << lvl);
        // far-away and non-finite coordinates are brought next to the map before the conversion: every position is then outside it
        const int x0 = (int)fminf(fmaxf(floorf(cx * s), -16.f), (float)(wl + 16));
        const int y0 = (int)fminf(fmaxf(floorf(cy * s), -16.f), (float)(hl + 16));
        const int px = x0 - kRadius + gx;
        size_t base = 0;      // floats in front of level lvl in the pooled buffer (levels 1..3)
        for (int l = 1; l < lvl; ++l) base += (size_t)(h >> l) * (w >> l) * D;
        const float* t = lvl == 0 ? ft0 : ftp + base;
        const float4* qv = (const float4*)q_s;
        __syncthreads();
        // the eight rows of the neighbourhood advance together, so eight loads are in flight per lane; rows and columns outside the map read
        // the clamped position instead (always inside the map) and are zeroed afterwards
        const bool okx = px >= 0 && px < wl;
        const float4* tv[kNb];
        float4 a[kNb];
#pragma unroll
        for (int gy = 0; gy < kNb; ++gy) {
            const int py = min(max(y0 - kRadius + gy, 0), hl - 1);
            tv[gy] = (const float4*)(t + ((size_t)py * wl + min(max(px, 0), wl - 1)) * D);
            a[gy] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int d = sub; d < D4; d += 8) {
            const float4 q = qv[d];
#pragma unroll
            for (int gy = 0; gy < kNb; ++gy) {
                const float4 v = tv[gy][d];
                a[gy].x = fmaf(v.x, q.x, a[gy].x);
                a[gy].y = fmaf(v.y, q.y, a[gy].y);
                a[gy].z = fmaf(v.z, q.z, a[gy].z);
                a[gy].w = fmaf(v.w, q.w, a[gy].w);
            }
        }
#pragma unroll
        for (int gy = 0; gy < kNb; ++gy) {
            const int py = y0 - kRadius + gy;
            float acc = (okx && py >= 0 && py < hl) ? (a[gy].x + a[gy].y) + (a[gy].z + a[gy].w) : 0.f;
            acc += __shfl_xor(acc, 1);
            acc += __shfl_xor(acc, 2);
            acc += __shfl_xor(acc, 4);
            if (sub == 0) g_s[lvl][gy][gx] = acc * inv_sqrt_d;
        }
    }
    __syncthreads();
    if (tid < kLevels * kWin * kWin) {
        const int lvl = tid / (kWin * kWin), k = tid % (kWin * kWin);
        const int a = k / kWin, b = k % kWin;      // a moves x, b moves y: the reference adds its (dy, dx) deltas to (x, y) coordinates
        const float s = 1.0f / (float)(1 << lvl);
        const float cxl = cx * s, cyl = cy * s;
        const float fx = cxl - floorf(cxl), fy = cyl - floorf(cyl);      // exact
        const float ex = 1.0f - fx, ey = 1.0f - fy;
        const float v = ey * ex * g_s[lvl][b][a] + ey * fx * g_s[lvl][b][a + 1] + fy * ex * g_s[lvl][b + 1][a] + fy * fx * g_s[lvl][b + 1][a + 1];
        out[(size_t)qi * out_cs + tid] = v;
    }
}

// 7x7, stride 1, zero padding 3.  A workgroup owns 16x16 output pixels and CO output channels; the 22x22 input patch goes through LDS four
// input channels at a time as one float4 per pixel; the 4 x CO weights of a tap are contiguous at a wave-uniform address ([7][7][Cin4][CoutP]
// zero-padded pack), so they arrive through the scalar cache and feed the fmas as scalar operands: one 16-byte LDS read per 4 CO fmas.
template <int CO>
__global__ __launch_bounds__(256) void conv7x7_kernel(const float* __restrict__ in, int in_cs, const float* __restrict__ wp,
                                                      const float* __restrict__ bias, const float* __restrict__ prelu, float slope,
                                                      int act, float* __restrict__ out, int out_cs, int H, int W, int Cin, int Cout,
                                                      int CoutP, int zblocks) {
    __shared__ float4 tile[22][23];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n = blockIdx.z / zblocks, co0 = (blockIdx.z % zblocks) * CO;
    const int bx = blockIdx.x * 16, by = blockIdx.y * 16;
    const int Cin4 = (Cin + 3) & ~3;
    const float* img = in + (size_t)n * H * W * in_cs;
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = 0.f;
    for (int ci0 = 0; ci0 < Cin; ci0 += 4) {
        __syncthreads();
        for (int i = tid; i < 22 * 22; i += 256) {
            const int ly = i / 22, lx = i % 22;
            const int gy = by + ly - 3, gx = bx + lx - 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float* p = img + ((size_t)gy * W + gx) * in_cs + ci0;
                v.x = p[0];
                if (ci0 + 1 < Cin) v.y = p[1];
                if (ci0 + 2 < Cin) v.z = p[2];
                if (ci0 + 3 < Cin) v.w = p[3];
            }
            tile[ly][lx] = v;
        }
        __syncthreads();
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float4 v = tile[ty + ky][tx + kx];
                const float* wt = wp + ((size_t)(ky * 7 + kx) * Cin4 + ci0) * CoutP + co0;
#pragma unroll
                for (int j = 0; j < CO; ++j) {
                    float a = acc[j];
                    a = fmaf(v.x, wt[j], a);
                    a = fmaf(v.y, wt[CoutP + j], a);
                    a = fmaf(v.z, wt[2 * CoutP + j], a);
                    a = fmaf(v.w, wt[3 * CoutP + j], a);
                    acc[j] = a;
                }
            }
        }
    }
    const int X = bx + tx, Y = by + ty;
    if (X >= W || Y >= H) return;
    float* o = out + ((size_t)n * H * W + (size_t)Y * W + X) * out_cs;
#pragma unroll
    for (int j = 0; j < CO; ++j) {
        const int co = co0 + j;
        if (co < Cout) {
            float v = acc[j] + (bias ? bias[co] : 0.f);
            if (act == 1) v = v > 0.f ? v : v * slope;
            else if (act == 3) v = v > 0.f ? v : v * prelu[co];
            o[co] = v;
        }
    }
}

// multi_flow_combine up to comb_block's input: warps[.., 3 i + c] = sigmoid(mask_i) * warp(img0, flow0_i)[c] + (1 - sigmoid(mask_i)) *
// warp(img1, flow1_i)[c] + mean + res_i[c]; fin channels: flow0 (2 n) | flow1 (2 n) | mask logits (n) | res (3 n)
__global__ void amt_warps_kernel(const float* __restrict__ img0, const float* __restrict__ img1, int img_cs, const float* __restrict__ fin,
                                 int fin_cs, const float* __restrict__ mean, int nf, float* __restrict__ out, int out_cs, int Hp, int Wp) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)Hp * Wp) return;
    const int X = (int)(idx % Wp), Y = (int)(idx / Wp);
    const WarpGeo g = make_warp_geo(Wp, Hp);
    const float* f = fin + (size_t)idx * fin_cs;
    float* o = out + (size_t)idx * out_cs;
    const float mean_v = mean[0];
    for (int i = 0; i < nf; ++i) {
        const float m = 1.0f / (1.0f + expf(-f[4 * nf + i])), om = 1.0f - m;
        float wv[2][3];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const Tap4 t = warp_taps(g, X, Y, f[2 * nf * k + 2 * i], f[2 * nf * k + 2 * i + 1]);
            const float* im = k ? img1 : img0;
            const float *a = im + (size_t)t.o00 * img_cs, *b = im + (size_t)t.o01 * img_cs, *c = im + (size_t)t.o10 * img_cs,
                        *d = im + (size_t)t.o11 * img_cs;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) wv[k][ch] = a[ch] * t.nw + b[ch] * t.ne + c[ch] * t.sw + d[ch] * t.se;
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[3 * i + ch] = ((m * wv[0][ch] + om * wv[1][ch]) + mean_v) + f[5 * nf + 3 * i + ch];
    }
}

// out [H,W,3] = clamp(mean over the n flows of warps + comb, 0, 1) cropped at (top, left)
__global__ void amt_out_kernel(const float* __restrict__ warps, int warps_cs, const float* __restrict__ comb, int comb_cs, int nf,
                               float* __restrict__ out, int Wp, int top, int left, int H, int W) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int X = (int)(idx % W), Y = (int)(idx / W);
    const size_t p = (size_t)(Y + top) * Wp + (X + left);
    const float* wr = warps + p * warps_cs;
    const float* cb = comb + p * comb_cs;
    const float cnt = (float)nf;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float s = wr[ch];
        for (int i = 1; i < nf; ++i) s += wr[3 * i + ch];
        out[(size_t)idx * 3 + ch] = fminf(fmaxf(s / cnt + cb[ch], 0.f), 1.f);
    }
}

// mean_ over the three colour channels of both padded frames (:1206), deterministic: kMeanSlots fixed slots in double, summed in order
constexpr int kMeanSlots = 256;
__global__ __launch_bounds__(256) void amt_mean_partial_kernel(const float* __restrict__ img, long pixels, double* __restrict__ part) {
    __shared__ double s[256];
    double a = 0.0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long)kMeanSlots * 256) {
        const float* q = img + (size_t)p * 8;
        a += (double)q[0] + (double)q[1] + (double)q[2];
    }
    s[threadIdx.x] = a;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) s[threadIdx.x] += s[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}
__global__ void amt_mean_final_kernel(const double* __restrict__ part, long pixels, float* __restrict__ mean) {
    double a = 0.0;
    for (int i = 0; i < kMeanSlots; ++i) a += part[i];
    mean[0] = (float)(a / (3.0 * (double)pixels));
}
__global__ void amt_center_kernel(float* __restrict__ img, long pixels, const float* __restrict__ mean) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pixels) return;
    const float m = mean[0];
    float* q = img + (size_t)idx * 8;
    q[0] -= m, q[1] -= m, q[2] -= m;
}

// out[y, x, 0..C) = a[y * step, x * step, 0..C) + b[y, x, 0..C): channel-window copy (b null), stride-2 sub-sampling in front of a 1x1
// stride-2 layer, and the residual sums `flow + dflow`, `ft + dft`.  reps > 1: out[.., r * C + c] += b[.., c] for r < reps (a = out), the
// up-sampled flow added to each of the num_flows flows (:1262-1263)
__global__ void amt_add_kernel(const float* a, int a_cs, int a_w, int step, const float* __restrict__ b, int b_cs, float* out, int out_cs, int h, int w, int C, int reps) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)h * w) return;
    const int x = (int)(idx % w), y = (int)(idx / w);
    const float* pa = a + ((size_t)(y * step) * a_w + (size_t)x * step) * a_cs;
    const float* pb = b ? b + (size_t)idx * b_cs : nullptr;
    float* po = out + (size_t)idx * out_cs;
    for (int r = 0; r < reps; ++r)
        for (int c = 0; c < C; ++c) po[r * C + c] = pb ? pa[r * C + c] + pb[c] : pa[r * C + c];
}

// amt_arch.warp (:26-34) of a C-channel window by a 2-channel flow window: the shared warp_taps (border, align_corners=True)
__global__ void amt_warp_kernel(const float* __restrict__ in, int in_cs, const float* __restrict__ flow, int flow_cs, float* __restrict__ out,
                                int out_cs, int H, int W, int C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const WarpGeo g = make_warp_geo(W, H);
    const float* f = flow + (size_t)idx * flow_cs;
    const Tap4 t = warp_taps(g, (int)(idx % W), (int)(idx / W), f[0], f[1]);
    const float *a = in + (size_t)t.o00 * in_cs, *b = in + (size_t)t.o01 * in_cs, *c = in + (size_t)t.o10 * in_cs, *d = in + (size_t)t.o11 * in_cs;
    float* o = out + (size_t)idx * out_cs;
    for (int ch = 0; ch < C; ++ch) o[ch] = a[ch] * t.nw + b[ch] * t.ne + c[ch] * t.sw + d[ch] * t.se;
}

// out[n, Y, X, 0..C) = leaky_relu(F.interpolate(in, scale_factor=s, mode="bilinear", align_corners=False), slope): one thread per output
// pixel and group of V channels (V = 4: float4 loads and stores; V = 1 where a stride or a window offset is not 16-byte aligned), the
// channel groups of a pixel on neighbouring lanes, so the four taps are read and the result is written as contiguous runs.  Taps and blend
// are torch's (and resize_ratio_kernel's): bil_src with ratio 1 / s, rows blended first.  Each output element is written once.
template <int V>
__global__ void amt_upsample_lrelu_kernel(const float* __restrict__ in, int in_cs, float* __restrict__ out, int out_cs, int N, int h, int w,
                                          int C, int s, float ratio, float slope) {
    const int CV = C / V, Ho = h * s, Wo = w * s;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * Ho * Wo * CV) return;
    const int cg = (int)(idx % CV);
    const long p = idx / CV;
    const int X = (int)(p % Wo), Y = (int)((p / Wo) % Ho), n = (int)(p / ((long)Wo * Ho));
    const BilS by = bil_src(Y, ratio, h), bx = bil_src(X, ratio, w);
    const float* b = in + (size_t)n * h * w * in_cs + (size_t)cg * V;
    const float *p00 = b + ((size_t)by.i0 * w + bx.i0) * in_cs, *p01 = b + ((size_t)by.i0 * w + bx.i1) * in_cs;
    const float *p10 = b + ((size_t)by.i1 * w + bx.i0) * in_cs, *p11 = b + ((size_t)by.i1 * w + bx.i1) * in_cs;
    float* o = out + (size_t)p * out_cs + (size_t)cg * V;
    alignas(16) float a[V], bb[V], c[V], d[V], r[V];
    if (V == 4) {
        *(float4*)a = *(const float4*)p00, *(float4*)bb = *(const float4*)p01, *(float4*)c = *(const float4*)p10, *(float4*)d = *(const float4*)p11;
    } else {
        a[0] = p00[0], bb[0] = p01[0], c[0] = p10[0], d[0] = p11[0];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const float v = by.w0 * (bx.w0 * a[k] + bx.w1 * bb[k]) + by.w1 * (bx.w0 * c[k] + bx.w1 * d[k]);      // no contraction: five roundings
        r[k] = v > 0.f ? v : v * slope;
    }
    if (V == 4) *(float4*)o = *(const float4*)r;
    else o[0] = r[0];
}

}  // namespace
}  // namespace vfi

using namespace vfi;

extern "C" {

int vfi_amt_pool_features(const float* f_dev, int h, int w, int D, float* pooled_dev, void* stream) {
    VFI_REQUIRE(f_dev && pooled_dev && D > 0 && D % 4 == 0 && aligned16(f_dev) && aligned16(pooled_dev),
                "vfi_amt_pool_features: bad arguments (D = %d must be a multiple of 4, buffers 16-byte aligned)", D);
    VFI_REQUIRE(h >= 16 && w >= 16 && (long)h * w * D < (1L << 31),
                "vfi_amt_pool_features: a %dx%d feature map: both sides must be at least 16 (the reference is all-NaN when the coarsest "
                "correlation level is one pixel wide) and the map below 2^31 elements", h, w);
    TraceScope ts("amt_pool2", (hipStream_t)stream);
    const float* src = f_dev;
    float* dst = pooled_dev;
    for (int l = 0; l < kLevels - 1; ++l) {
        const int hin = h >> l, win = w >> l;
        const long n = (long)(hin >> 1) * (win >> 1) * (D / 4);
        hipLaunchKernelGGL(amt_pool2_kernel, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, hin, win, D / 4);
        src = dst;
        dst += (size_t)(hin >> 1) * (win >> 1) * D;
    }
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_amt_corr_lookup(const float* fq_dev, const float* ft_dev, const float* ft_pooled_dev, const float* flow_dev, int flow_cs, float scale,
                        int h, int w, int D, float* out_dev, int out_cs, void* stream) {
    VFI_REQUIRE(fq_dev && ft_dev && ft_pooled_dev && flow_dev && out_dev && flow_cs >= 2 && out_cs >= kLevels * kWin * kWin,
                "vfi_amt_corr_lookup: bad arguments");
    VFI_REQUIRE(D > 0 && D % 4 == 0 && D <= kMaxD && aligned16(ft_dev) && aligned16(ft_pooled_dev),
                "vfi_amt_corr_lookup: D = %d must be a multiple of 4, at most %d, and the target maps 16-byte aligned", D, kMaxD);
    VFI_REQUIRE(h >= 16 && w >= 16 && (long)h * w * D < (1L << 31) && (long)h * w * out_cs < (1L << 31) && (long)h * w * flow_cs < (1L << 31),
                "vfi_amt_corr_lookup: a %dx%d feature map: both sides must be at least 16 (the reference is all-NaN when the coarsest "
                "correlation level is one pixel wide) and every tensor below 2^31 elements", h, w);
    TraceScope ts("amt_lookup", (hipStream_t)stream);
    hipLaunchKernelGGL(amt_lookup_kernel, dim3(h * w), dim3(256), 0, (hipStream_t)stream, fq_dev, ft_dev, ft_pooled_dev, flow_dev, flow_cs,
                       scale, (float)(1.0 / sqrt((double)(float)D)), h, w, D, out_dev, out_cs);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_conv7x7(const float* in_dev, int in_cs, const float* w_dev, const float* bias_dev, const float* prelu_dev, float slope, int act,
                int Cin, int Cout, float* out_dev, int out_cs, int N, int H, int W, void* stream) {
    // Cout: a workgroup owns 16 output channels whatever Cout is (blockIdx.z walks the groups), so registers and LDS do not depend on it; a
    // wider layer re-stages the input patch once per group of 16, which is what bounds the layers this direct form is meant for.  96 was
    // the widest layer served (AMT-L's convf1); AMT-G's convf1 is 4 -> 128: eight groups over one staged float4 per pixel.
    VFI_REQUIRE(in_dev && w_dev && out_dev && N > 0 && H > 0 && W > 0 && Cin > 0 && Cin <= 96 && Cout > 0 && Cout <= 128 && in_cs >= Cin &&
                    out_cs >= Cout,
                "vfi_conv7x7: bad arguments (Cin %d at most 96, Cout %d at most 128, strides %d / %d at least the channel counts)", Cin, Cout,
                in_cs, out_cs);
    VFI_REQUIRE(act == 0 || act == 1 || (act == 3 && prelu_dev), "vfi_conv7x7: act %d (0 none, 1 leaky relu, 3 PReLU with slopes)", act);
    VFI_REQUIRE((long)N * H * W * in_cs < (1L << 31) * 4 && (long)N * H * W < (1L << 31) && aligned16(w_dev),
                "vfi_conv7x7: %d x %dx%d pixels are beyond the kernel's index arithmetic, or the weights are not 16-byte aligned", N, H, W);
    const int co = Cout <= 4 ? 4 : 16, CoutP = round_up(Cout, co), zb = CoutP / co;
    VFI_REQUIRE((long)N * zb <= 65535, "vfi_conv7x7: N = %d is too large a batch", N);
    TraceScope ts("conv7x7", (hipStream_t)stream);
    const dim3 grid(cdiv(W, 16), cdiv(H, 16), N * zb);
    if (co == 4)
        hipLaunchKernelGGL(conv7x7_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, w_dev, bias_dev, prelu_dev, slope, act,
                           out_dev, out_cs, H, W, Cin, Cout, CoutP, zb);
    else
        hipLaunchKernelGGL(conv7x7_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, w_dev, bias_dev, prelu_dev, slope, act,
                           out_dev, out_cs, H, W, Cin, Cout, CoutP, zb);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_amt_upsample_lrelu(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int h, int w, int C, int scale, float slope,
                           void* stream) {
    VFI_REQUIRE(in_dev && out_dev && N > 0 && h > 0 && w > 0 && C > 0 && in_cs >= C && out_cs >= C && (scale == 2 || scale == 4),
                "vfi_amt_upsample_lrelu: bad arguments (scale %d must be 2 or 4, strides %d / %d at least C = %d)", scale, in_cs, out_cs, C);
    const long total = (long)N * h * scale * w * scale * C;
    VFI_REQUIRE((long)h * scale < (1L << 22) && (long)w * scale < (1L << 22) && total / 256 < (1L << 31) - 1,
                "vfi_amt_upsample_lrelu: %d x %dx%d x %d channels at scale %d is beyond the kernel's index arithmetic", N, h, w, C, scale);
    TraceScope ts("amt_upsample", (hipStream_t)stream);
    const float ratio = 1.0f / (float)scale;
    if (C % 4 == 0 && in_cs % 4 == 0 && out_cs % 4 == 0 && aligned16(in_dev) && aligned16(out_dev))
        hipLaunchKernelGGL(amt_upsample_lrelu_kernel<4>, dim3(nblk(total / 4, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, out_dev,
                           out_cs, N, h, w, C, scale, ratio, slope);
    else
        hipLaunchKernelGGL(amt_upsample_lrelu_kernel<1>, dim3(nblk(total, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, out_dev, out_cs,
                           N, h, w, C, scale, ratio, slope);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_amt_combine_warps(const float* img0_dev, const float* img1_dev, int img_cs, const float* fin_dev, int fin_cs, const float* mean_dev,
                          int num_flows, float* out_dev, int out_cs, int Hp, int Wp, void* stream) {
    VFI_REQUIRE(img0_dev && img1_dev && fin_dev && mean_dev && out_dev && img_cs >= 3 && num_flows >= 1 && fin_cs >= 8 * num_flows &&
                    out_cs >= 3 * num_flows && Hp > 1 && Wp > 1,
                "vfi_amt_combine_warps: bad arguments");
    VFI_REQUIRE((long)Hp * Wp * fin_cs < (1L << 31) && (long)Hp * Wp * out_cs < (1L << 31),
                "vfi_amt_combine_warps: a %dx%d frame is beyond the kernel's index arithmetic", Hp, Wp);
    TraceScope ts("amt_warps", (hipStream_t)stream);
    hipLaunchKernelGGL(amt_warps_kernel, dim3(nblk((long)Hp * Wp, 256)), dim3(256), 0, (hipStream_t)stream, img0_dev, img1_dev, img_cs, fin_dev,
                       fin_cs, mean_dev, num_flows, out_dev, out_cs, Hp, Wp);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_amt_combine_out(const float* warps_dev, int warps_cs, const float* comb_dev, int comb_cs, int num_flows, float* out_dev, int Hp,
                        int Wp, int pad_top, int pad_left, int H, int W, void* stream) {
    VFI_REQUIRE(warps_dev && comb_dev && out_dev && num_flows >= 1 && warps_cs >= 3 * num_flows && comb_cs >= 3 && H > 0 && W > 0 &&
                    pad_top >= 0 && pad_left >= 0 && pad_top + H <= Hp && pad_left + W <= Wp,
                "vfi_amt_combine_out: bad arguments (the %dx%d crop at (%d, %d) must lie inside %dx%d)", H, W, pad_top, pad_left, Hp, Wp);
    VFI_REQUIRE((long)Hp * Wp * warps_cs < (1L << 31) * 4, "vfi_amt_combine_out: a %dx%d frame is beyond the kernel's index arithmetic", Hp, Wp);
    TraceScope ts("amt_out", (hipStream_t)stream);
    hipLaunchKernelGGL(amt_out_kernel, dim3(nblk((long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, warps_dev, warps_cs, comb_dev, comb_cs,
                       num_flows, out_dev, Wp, pad_top, pad_left, H, W);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- the network object: AMT-S / AMT-L / AMT-G on csrc/net_object.h ------------------------------------------------------------------------

namespace {

// enc / enc_stride: the feature encoder's stages of two blocks each (AMT-G's LargeEncoder has a fourth, stride-1 stage, layer3_2);
// n_upd: update4, update3[_low], update2[_low], then AMT-G's update3_high, update2_high; px_floats: the widest activation in floats per
// padded pixel, which bounds the frame size (vfi_amt_forward)
struct Cfg {
    int ch[4], skip, nf, D, comb_k, hid, fd, cd, cd2, fc, e1, n_enc, enc[4], enc_stride[4], n_upd, px_floats, n_tensors;
    const char* name;
};
// (amt.py's MAX_PADDED_PIXELS_G is derived from the same 88; tests/test_gpu_amt_g.py asserts that the two limits agree.)
// AMT-G's widest buffer is decoder1's ResBlock at half resolution: r8(3 * 84) + 8 + r8(84) = 352 channels = 88 floats per padded pixel
// (gru.0's input in update2_high, r8(188 + 4 + 84) = 280 channels, is 70).  AMT-S / AMT-L keep their 64.  The limit is signed (every object
// as created) or, for AMT-G after vfi_amt_set_large_frames, unsigned: every layer that meets an image of 2 GiB or more then has a
// large-image form (docs/design/amt.md "4K").
const Cfg kCfg[3] = {{{20, 32, 44, 56}, 20, 3, 84, 3, 76, 20, 64, 0, 68, 32, 3, {32, 64, 96}, {1, 2, 2}, 3, 64, 213, "AMT-S"},
                     {{48, 64, 72, 128}, 48, 5, 128, 7, 128, 48, 256, 160, 124, 64, 3, {64, 72, 128}, {1, 2, 2}, 3, 64, 207, "AMT-L"},
                     {{84, 96, 112, 128}, 84, 5, 128, 7, 192, 64, 256, 192, 188, 64, 4, {64, 112, 160, 160}, {1, 2, 2, 1}, 5, 88, 259, "AMT-G"}};

struct Conv7 {      // a vfi_conv7x7 layer: packed weights, bias, PReLU slopes (nullable) on the device
    float *w = nullptr, *b = nullptr, *pr = nullptr;
    int cin = 0, cout = 0;
};
struct Stem {       // a vfi_conv7x7s2_prelu layer: its output channels padded to 64, or AMT-G's 84 as they are
    float *w = nullptr, *b = nullptr, *slope = nullptr;
    int cout = 64;
};
struct EncBlk {
    vfi_conv_t *c1 = nullptr, *c2 = nullptr, *c3 = nullptr, *ds = nullptr;
    int cin = 0, c = 0, stride = 1;
};
struct Dec {
    vfi_conv_t *c0 = nullptr, *rb[5] = {}, *up = nullptr;      // convrelu, the ResBlock's conv1..conv5, ConvTranspose2d
    int cin = 0, c = 0, cout = 0;
};
struct Upd {
    vfi_conv_t *c1 = nullptr, *c2 = nullptr, *f2 = nullptr, *cv = nullptr, *g0 = nullptr, *g2 = nullptr, *fh0 = nullptr, *fh2 = nullptr, *wh0 = nullptr,
               *wh2 = nullptr;
    Conv7 f1;
};

}  // namespace

struct vfi_amt : PaddedNet {
    int variant = 0;      // 0 AMT-S, 1 AMT-L, 2 AMT-G
    bool large = false;   // vfi_amt_set_large_frames on an AMT-G object: padded frames up to max_padded_pixels_large(px_floats) are served
    Stem fe_stem, py_stem;
    EncBlk blk[8];
    vfi_conv_t* fe_out = nullptr;
    vfi_conv_t *py0[4] = {}, *py1[4] = {};
    Dec dec[4];           // decoder4, 3, 2, 1
    Upd upd[5];           // update4, 3[_low], 2[_low]; AMT-G: update3_high, update2_high
    vfi_conv_t *cb0 = nullptr, *cb2 = nullptr;
    Conv7 cb7[2];
};

namespace {

struct Run : NetRun<vfi_amt> {      // act 1 is LeakyReLU(0.1): amt_forward sets `leaky`
    // out = a (sub-sampled by step) [+ b]
    int add(const float* a, int a_cs, int a_w, int step, const float* b, int b_cs, float* out, int out_cs, int h, int w, int C, int reps = 1) {
        hipLaunchKernelGGL(amt_add_kernel, dim3(nblk((long)h * w, 256)), dim3(256), 0, st, a, a_cs, a_w, step, b, b_cs, out, out_cs, h, w, C, reps);
        VFI_CHECK_HIP(hipGetLastError());
        return 0;
    }
    int copy(const float* a, int a_cs, float* out, int out_cs, int h, int w, int C) { return add(a, a_cs, w, 1, nullptr, 0, out, out_cs, h, w, C); }
    int warp(const float* in, int in_cs, const float* flow, int flow_cs, float* out, int out_cs, int h, int w, int C) {
        hipLaunchKernelGGL(amt_warp_kernel, dim3(nblk((long)h * w, 256)), dim3(256), 0, st, in, in_cs, flow, flow_cs, out, out_cs, h, w, C);
        VFI_CHECK_HIP(hipGetLastError());
        return 0;
    }
    int resize(const float* in, int ics, int hi, int wi, float* out, int ocs, int ho, int wo, int C, float ratio, float mul) {
        return vfi_resize_bilinear_ratio(in, ics, out, ocs, 1, hi, wi, ho, wo, C, ratio, ratio, mul, st);
    }
    // InstanceNorm2d over N = 2 frames: out = relu2(relu1(norm(x)) + add).  out may be x: the apply kernel reads and writes one element per
    // thread at the same position and declares neither pointer __restrict__ (gmfss_bodies.h: instnorm_apply_body)
    int norm(const float* x, int cs, int C, long HW, int relu1, const float* add_, int add_cs, int relu2, float* out, int ocs) {
        const int cmax = m->variant == 2 ? 160 : 128;      // the widest normalised layer
        float* stats = buf("stats", 1, 1, 1, 2 * cmax * 2);
        float* nws = buf("norm_ws", 1, 1, 1, 2 * 64 * cmax * 2 * 2);
        if (bad) return -1;
        if (vfi_instnorm_stats(x, cs, C, 2, HW, stats, (double*)nws, (int64_t)64 * 2 * C * 2 * sizeof(double), st)) return -1;
        return vfi_instnorm_apply(x, cs, stats, C, 2, HW, relu1, add_, add_cs, relu2, out, ocs, st);
    }
};

// a decoder's convblock (:824-857): convrelu, ResBlock with side channels (:762-799), ConvTranspose2d.  The ResBlock's side-channel
// layers read the last `skip` channels of x1 / x3 as a window and write behind the main channels (offset off); conv3 / conv5 were created
// with a channel map over that layout, so no cat is ever made.
int run_decoder(Run& r, const Dec& d, int skip, const float* din, int din_cs, int h, int w, float* out, int out_cs) {
    const int c8 = r8(d.c), off = c8 + 8, xcs = off + r8(skip), so = d.c - skip;
    float *r0 = r.buf("dec_r0", 1, h, w, c8), *x1 = r.buf("dec_x1", 1, h, w, xcs), *x3 = r.buf("dec_x3", 1, h, w, xcs), *r5 = r.buf("dec_r5", 1, h, w, c8);
    if (r.bad) return -1;
    VFI_DO(r.conv(d.c0, din, din_cs, h, w, r0, c8, 1, 3));
    VFI_DO(r.conv(d.rb[0], r0, c8, h, w, x1, xcs, 1, 3));
    VFI_DO(r.conv(d.rb[1], x1 + so, xcs, h, w, x1 + off, xcs, 1, 3));
    VFI_DO(r.conv(d.rb[2], x1, xcs, h, w, x3, xcs, 1, 3));
    VFI_DO(r.conv(d.rb[3], x3 + so, xcs, h, w, x3 + off, xcs, 1, 3));
    VFI_DO(r.conv(d.rb[4], x3, xcs, h, w, r5, c8, 1, 3, r0, c8));
    return r.conv(d.up, r5, c8, h, w, out, out_cs, 1, 0);
}

// an update block from convf1 on (:1060-1068), at the h x w of its buffers: convf1 / convf2 of the flow window, `conv` over (cor | flo) into the
// front of inp (whose flow and net windows the caller has filled), gru, feat_head -> dn, flow_head -> df
int update_tail(Run& r, const Cfg& g, const Upd& U, const float* flow, int flow_cs, int ch, int h, int w, float* inp, int inp_cs, float* cf, int cf_cs,
                float* fa, float* h1, float* h2, float* h3, float* dn, float* df) {
    const int hcs = r8(g.hid), cdo = g.cd2 ? g.cd2 : g.cd;
    VFI_DO(vfi_conv7x7(flow, flow_cs, U.f1.w, U.f1.b, nullptr, 0.1f, 1, 4, 2 * g.fd, fa, 2 * g.fd, 1, h, w, r.st));
    VFI_DO(r.conv(U.f2, fa, 2 * g.fd, h, w, cf + cdo, cf_cs, 1, 1));
    // (writes channels 0 .. fc of inp, directly in front of the flow window: the layer objects store exactly Cout channels, never Cout
    // rounded up, see the `co < a.Cout` guards of conv_mfma*.hip / conv_wino.hip)
    VFI_DO(r.conv(U.cv, cf, cf_cs, h, w, inp, inp_cs, 1, 1));
    VFI_DO(r.conv(U.g0, inp, inp_cs, h, w, h1, hcs, 1, 1));
    VFI_DO(r.conv(U.g2, h1, hcs, h, w, h2, hcs, 1, 0));
    VFI_DO(r.conv(U.fh0, h2, hcs, h, w, h1, hcs, 1, 1));
    VFI_DO(r.conv(U.fh2, h1, hcs, h, w, dn, r8(ch), 1, 0));
    VFI_DO(r.conv(U.wh0, h2, hcs, h, w, h3, hcs, 1, 1));
    return r.conv(U.wh2, h3, hcs, h, w, df, 8, 1, 0);
}

int amt_forward(vfi_amt* m, const float* f0, const float* f1, int C, int H, int W, const float* ts, int n_t, float* out, hipStream_t st) {
    const Cfg& g = kCfg[m->variant];
    const bool basic = m->variant >= 1, G = m->variant == 2;      // basic: the BasicUpdateBlock family, AMT-L and AMT-G, which share a forward; G: the 84-channel stem and the high blocks
    const int Hp = m->Hp, Wp = m->Wp, top = (Hp - H) / 2, left = (Wp - W) / 2;
    const long P = (long)Hp * Wp;
    const int h8 = Hp / 8, w8 = Wp / 8, D = g.D;
    Run r{{m, st, 0.1f}};
    // ---- once per pair ----
    float* img = r.buf("img", 2, Hp, Wp, 8);
    float* mean = r.buf("mean", 1, 1, 1, 4 + 2 * kMeanSlots);
    if (r.bad) return -1;
    double* part = (double*)(mean + 4);
    VFI_DO(pad_frame_pair(f0, f1, C, H, W, img, Hp, Wp, top, left, true, st));      // InputPadder(dims, 16) (:194-211): centred, replicate
    hipLaunchKernelGGL(amt_mean_partial_kernel, dim3(kMeanSlots), dim3(256), 0, st, (const float*)img, 2 * P, part);
    hipLaunchKernelGGL(amt_mean_final_kernel, dim3(1), dim3(1), 0, st, (const double*)part, 2 * P, mean);
    hipLaunchKernelGGL(amt_center_kernel, dim3(nblk(2 * P, 256)), dim3(256), 0, st, img, 2 * P, (const float*)mean);
    VFI_CHECK_HIP(hipGetLastError());
    // feature encoder (SmallEncoder / BasicEncoder / LargeEncoder, norm_fn = instance) over both frames
    float* fmap = r.buf("fmap", 2, h8, w8, D);
    {
        int h = Hp / 2, w = Wp / 2;
        float* e1 = r.buf("fe_e1", 2, h, w, 64);
        if (r.bad) return -1;
        VFI_DO(vfi_conv7x7s2_prelu(img, 8, m->fe_stem.w, m->fe_stem.b, m->fe_stem.slope, 64, e1, 64, 2, Hp, Wp, st));
        VFI_DO(r.norm(e1, 64, g.e1, (long)h * w, 1, nullptr, 0, 0, e1, 64));
        const float* x = e1;
        int xcs = 64;
        for (int k = 0; k < 2 * g.n_enc; ++k) {
            const EncBlk& B = m->blk[k];
            const int ho = h / B.stride, wo = w / B.stride, c = B.c;
            float* y3 = r.buf("fe_y3", 2, ho, wo, c);
            if (!basic) {
                const int c4 = c / 4;
                float *y1 = r.buf("fe_y1", 2, h, w, c4), *y2 = r.buf("fe_y2", 2, ho, wo, c4);
                if (r.bad) return -1;
                VFI_DO(r.conv(B.c1, x, xcs, h, w, y1, c4, 2, 0));
                VFI_DO(r.norm(y1, c4, c4, (long)h * w, 1, nullptr, 0, 0, y1, c4));
                VFI_DO(r.conv(B.c2, y1, c4, h, w, y2, c4, 2, 0));
                VFI_DO(r.norm(y2, c4, c4, (long)ho * wo, 1, nullptr, 0, 0, y2, c4));
                VFI_DO(r.conv(B.c3, y2, c4, ho, wo, y3, c, 2, 0));
            } else {
                float* y1 = r.buf("fe_y1", 2, ho, wo, c);
                if (r.bad) return -1;
                VFI_DO(r.conv(B.c1, x, xcs, h, w, y1, c, 2, 0));
                VFI_DO(r.norm(y1, c, c, (long)ho * wo, 1, nullptr, 0, 0, y1, c));
                VFI_DO(r.conv(B.c2, y1, c, ho, wo, y3, c, 2, 0));
            }
            const float* res = x;
            int res_cs = xcs;
            if (B.ds) {      // Conv2d(cin, c, 1, stride 2) + norm: the two frames sub-sampled as one image of 2 ho rows
                float *sub = r.buf("fe_sub", 2, ho, wo, B.cin), *dsn = r.buf("fe_ds", 2, ho, wo, c);
                if (r.bad) return -1;
                VFI_DO(r.add(x, xcs, w, 2, nullptr, 0, sub, B.cin, 2 * ho, wo, B.cin));
                VFI_DO(r.conv(B.ds, sub, B.cin, ho, wo, dsn, c, 2, 0));
                VFI_DO(r.norm(dsn, c, c, (long)ho * wo, 0, nullptr, 0, 0, dsn, c));
                res = dsn, res_cs = c;
            }
            float* xn = r.buf(k % 2 ? "fe_xb" : "fe_xa", 2, ho, wo, c);
            if (r.bad) return -1;
            VFI_DO(r.norm(y3, c, c, (long)ho * wo, 1, res, res_cs, 1, xn, c));
            x = xn, xcs = c, h = ho, w = wo;
        }
        VFI_DO(r.conv(m->fe_out, x, xcs, h8, w8, fmap, D, 2, 0));
    }
    const float *fm0 = fmap, *fm1 = fmap + (size_t)h8 * w8 * D;
    size_t npool = 0;
    for (int l = 1; l < kLevels; ++l) npool += (size_t)(h8 >> l) * (w8 >> l);
    float* pool = r.buf("pool", 2, 1, 1, (int)(npool * D));
    if (r.bad) return -1;
    float *pool0 = pool, *pool1 = pool + npool * D;
    VFI_DO(vfi_amt_pool_features(fm0, h8, w8, D, pool0, st));
    VFI_DO(vfi_amt_pool_features(fm1, h8, w8, D, pool1, st));
    // pyramid encoder over both frames
    float* pyr[4];
    int pcs[4];
    {
        const float* x = img;
        int xcs = 8, h = Hp, w = Wp;
        for (int i = 0; i < 4; ++i) {
            pcs[i] = (basic && !G && i == 0) ? 64 : r8(g.ch[i]);      // AMT-L's stem writes its 64 padded channels, AMT-G's its own 84
            float* a = r.buf("py_a", 2, h / 2, w / 2, pcs[i]);
            pyr[i] = r.buf("py_p", 2, h / 2, w / 2, pcs[i]);
            if (r.bad) return -1;
            if (basic && i == 0) VFI_DO(vfi_conv7x7s2_prelu(img, 8, m->py_stem.w, m->py_stem.b, m->py_stem.slope, m->py_stem.cout, a, pcs[0], 2, Hp, Wp, st));
            else VFI_DO(r.conv(m->py0[i], x, xcs, h, w, a, pcs[i], 2, 3));
            h /= 2, w /= 2;
            VFI_DO(r.conv(m->py1[i], a, pcs[i], h, w, pyr[i], pcs[i], 2, 3));
            x = pyr[i], xcs = pcs[i];
        }
    }
    const int h16 = Hp / 16, w16 = Wp / 16, c3 = g.ch[3], din4_cs = r8(2 * c3 + 1);
    float* din4 = r.buf("din4", 1, h16, w16, din4_cs);
    if (r.bad) return -1;
    VFI_DO(r.copy(pyr[3], pcs[3], din4, din4_cs, h16, w16, c3));
    VFI_DO(r.copy(pyr[3] + (size_t)h16 * w16 * pcs[3], pcs[3], din4 + c3, din4_cs, h16, w16, c3));
    // ---- per timestep ----
    const int hcs = r8(g.hid), cdo = g.cd2 ? g.cd2 : g.cd, cf_cs = r8(cdo + g.fd);
    for (int ti = 0; ti < n_t; ++ti) {
        const float embt = ts[ti];
        const float s1 = 1.0f / embt, s0 = 1.0f / (1.0f - embt);
        VFI_DO(vfi_fill_items(din4 + 2 * c3, din4_cs, 1, 1, (int64_t)h16 * w16, &embt, st));
        int ocs = r8(g.ch[2] + 4);
        float* o = r.buf("dec_out", 1, h8, w8, ocs);
        if (r.bad) return -1;
        VFI_DO(run_decoder(r, m->dec[0], g.skip, din4, din4_cs, h16, w16, o, ocs));
        float *fl = o, *ft = o + 4;      // (flow0, flow1) and the hidden feature of the current level
        int fcs = ocs;
        for (int s = 0; s < 3; ++s) {
            const int lvl = 2 - s, down = 1 << s, h = h8 * down, w = w8 * down, ch = g.ch[lvl];
            const Upd& U = m->upd[s];
            // the flows at 1/8 resolution (:1190-1203)
            const float* fd = fl;
            int fd_cs = fcs;
            if (down != 1) {
                float* t = r.buf("flow_d", 1, h8, w8, 4);
                if (r.bad) return -1;
                VFI_DO(r.resize(fl, fcs, h, w, t, 4, h8, w8, 4, (float)down, 1.0f / (float)down));
                fd = t, fd_cs = 4;
            }
            float* corr = r.buf("corr", 1, h8, w8, 2 * kLevels * kWin * kWin);
            const int inp_cs = r8(g.fc + 4 + ch);
            float *inp = r.buf("upd_in", 1, h8, w8, inp_cs), *cf = r.buf("upd_cf", 1, h8, w8, cf_cs), *fa = r.buf("upd_f1", 1, h8, w8, 2 * g.fd);
            float *h1 = r.buf("upd_h1", 1, h8, w8, hcs), *h2 = r.buf("upd_h2", 1, h8, w8, hcs), *h3 = r.buf("upd_h3", 1, h8, w8, hcs);
            float *dn = r.buf("upd_dn", 1, h8, w8, r8(ch)), *df = r.buf("upd_df", 1, h8, w8, 8);
            if (r.bad) return -1;
            VFI_DO(vfi_amt_corr_lookup(fm0, fm1, pool1, fd + 2, fd_cs, s1, h8, w8, D, corr, 392, st));
            VFI_DO(vfi_amt_corr_lookup(fm1, fm0, pool0, fd, fd_cs, s0, h8, w8, D, corr + 196, 392, st));
            // the update block (:969-1073) at 1/8 resolution
            if (down != 1) VFI_DO(r.resize(ft, fcs, h, w, inp + g.fc + 4, inp_cs, h8, w8, ch, (float)down, 1.0f));
            else VFI_DO(r.copy(ft, fcs, inp + g.fc + 4, inp_cs, h8, w8, ch));
            VFI_DO(r.copy(fd, fd_cs, inp + g.fc, inp_cs, h8, w8, 4));
            if (basic) {
                float* c1 = r.buf("upd_c1", 1, h8, w8, g.cd);
                if (r.bad) return -1;
                VFI_DO(r.conv(U.c1, corr, 392, h8, w8, c1, g.cd, 1, 1));
                VFI_DO(r.conv(U.c2, c1, g.cd, h8, w8, cf, cf_cs, 1, 1));
            } else {
                VFI_DO(r.conv(U.c1, corr, 392, h8, w8, cf, cf_cs, 1, 1));
            }
            VFI_DO(update_tail(r, g, U, fd, fd_cs, ch, h8, w8, inp, inp_cs, cf, cf_cs, fa, h1, h2, h3, dn, df));
            const float *dnu = dn, *dfu = df;
            int dnu_cs = r8(ch), dfu_cs = 8;
            if (down != 1) {
                float *a = r.buf("upd_dnu", 1, h, w, r8(ch)), *b = r.buf("upd_dfu", 1, h, w, 4);
                if (r.bad) return -1;
                VFI_DO(r.resize(dn, r8(ch), h8, w8, a, r8(ch), h, w, ch, 1.0f / (float)down, 1.0f));
                VFI_DO(r.resize(df, 8, h8, w8, b, 4, h, w, 4, 1.0f / (float)down, (float)down));
                dnu = a, dfu = b, dfu_cs = 4;
            }
            // the next decoder's input: ft + dft | warp(f0_lvl, flow0) | warp(f1_lvl, flow1) | flow0 + dflow0 | flow1 + dflow1
            const int din_cs = r8(3 * ch + 4);
            float* din = r.buf("dec_in", 1, h, w, din_cs);
            const Dec& dc = m->dec[s + 1];
            ocs = r8(dc.cout);
            float *on = r.buf("dec_out", 1, 2 * h, 2 * w, ocs), *up = r.buf("flow_up", 1, 2 * h, 2 * w, 4);
            if (r.bad) return -1;
            VFI_DO(r.add(ft, fcs, w, 1, dnu, dnu_cs, din, din_cs, h, w, ch));
            VFI_DO(r.add(fl, fcs, w, 1, dfu, dfu_cs, din + 3 * ch, din_cs, h, w, 4));
            if (G && down != 1) {
                // update3_high / update2_high (:1537-1543, :1558-1564) at this level's own resolution, on the sums just written (ft + dft,
                // the four flow channels) and on the SAME lookup output.  The reference resizes the 392 lookup channels and then applies
                // convc1 (1x1); convc1 is linear and per pixel and the bilinear weights sum to 1, so convc1 runs on the 1/8 map (bias, no
                // activation) and its 256 channels are resized, with the LeakyReLU in the same pass: the resized lookup output never exists
                const Upd& UH = m->upd[s + 2];
                TraceScope high("amt_high_blocks", st);      // an outer scope: everything the two high blocks launch (tools/amt_bench.py)
                float *c1lo = r.buf("updh_c1lo", 1, h8, w8, g.cd), *c1 = r.buf("updh_c1", 1, h, w, g.cd);
                float *inph = r.buf("upd_in", 1, h, w, inp_cs), *cfh = r.buf("upd_cf", 1, h, w, cf_cs), *fah = r.buf("upd_f1", 1, h, w, 2 * g.fd);
                float *h1h = r.buf("upd_h1", 1, h, w, hcs), *h2h = r.buf("upd_h2", 1, h, w, hcs), *h3h = r.buf("upd_h3", 1, h, w, hcs);
                float *dnh = r.buf("upd_dn", 1, h, w, r8(ch)), *dfh = r.buf("upd_df", 1, h, w, 8);
                if (r.bad) return -1;
                VFI_DO(r.conv(UH.c1, corr, 392, h8, w8, c1lo, g.cd, 1, 0));
                VFI_DO(vfi_amt_upsample_lrelu(c1lo, g.cd, c1, g.cd, 1, h8, w8, g.cd, down, 0.1f, st));
                VFI_DO(r.conv(UH.c2, c1, g.cd, h, w, cfh, cf_cs, 1, 1));
                VFI_DO(r.copy(din, din_cs, inph + g.fc + 4, inp_cs, h, w, ch));
                VFI_DO(r.copy(din + 3 * ch, din_cs, inph + g.fc, inp_cs, h, w, 4));
                VFI_DO(update_tail(r, g, UH, din + 3 * ch, din_cs, ch, h, w, inph, inp_cs, cfh, cf_cs, fah, h1h, h2h, h3h, dnh, dfh));
                VFI_DO(r.add(din, din_cs, w, 1, dnh, r8(ch), din, din_cs, h, w, ch));
                VFI_DO(r.add(din + 3 * ch, din_cs, w, 1, dfh, 8, din + 3 * ch, din_cs, h, w, 4));
            }
            VFI_DO(r.warp(pyr[lvl], pcs[lvl], din + 3 * ch, din_cs, din + ch, din_cs, h, w, ch));
            VFI_DO(r.warp(pyr[lvl] + (size_t)h * w * pcs[lvl], pcs[lvl], din + 3 * ch + 2, din_cs, din + 2 * ch, din_cs, h, w, ch));
            VFI_DO(run_decoder(r, dc, g.skip, din, din_cs, h, w, on, ocs));
            VFI_DO(r.resize(din + 3 * ch, din_cs, h, w, up, 4, 2 * h, 2 * w, 4, 0.5f, 2.0f));
            if (s < 2) {
                VFI_DO(r.add(on, ocs, 2 * w, 1, up, 4, on, ocs, 2 * h, 2 * w, 4));
            } else {      // the num_flows flows of each direction take the up-sampled flow of theirs (:1262-1263)
                VFI_DO(r.add(on, ocs, 2 * w, 1, up, 4, on, ocs, 2 * h, 2 * w, 2, g.nf));
                VFI_DO(r.add(on + 2 * g.nf, ocs, 2 * w, 1, up + 2, 4, on + 2 * g.nf, ocs, 2 * h, 2 * w, 2, g.nf));
            }
            fl = on, ft = on + 4, fcs = ocs;
        }
        // multi_flow_combine (:869-902), clamp, un-pad
        const int wr_cs = r8(3 * g.nf), mid_cs = r8(6 * g.nf);
        float *wr = r.buf("comb_in", 1, Hp, Wp, wr_cs), *mid = r.buf("comb_mid", 1, Hp, Wp, mid_cs), *cb = r.buf("comb_out", 1, Hp, Wp, 8);
        if (r.bad) return -1;
        VFI_DO(vfi_amt_combine_warps(img, img + (size_t)P * 8, 8, fl, fcs, mean, g.nf, wr, wr_cs, Hp, Wp, st));
        if (basic) {
            VFI_DO(vfi_conv7x7(wr, wr_cs, m->cb7[0].w, m->cb7[0].b, m->cb7[0].pr, 0.f, 3, 3 * g.nf, 6 * g.nf, mid, mid_cs, 1, Hp, Wp, st));
            VFI_DO(vfi_conv7x7(mid, mid_cs, m->cb7[1].w, m->cb7[1].b, nullptr, 0.f, 0, 6 * g.nf, 3, cb, 8, 1, Hp, Wp, st));
        } else {
            VFI_DO(r.conv(m->cb0, wr, wr_cs, Hp, Wp, mid, mid_cs, 1, 3));
            VFI_DO(r.conv(m->cb2, mid, mid_cs, Hp, Wp, cb, 8, 1, 0));
        }
        VFI_DO(vfi_amt_combine_out(wr, wr_cs, cb, 8, g.nf, out + (size_t)ti * H * W * 3, Hp, Wp, top, left, H, W, st));
    }
    return 0;
}

int amt_pad(int n) { return n + (((n / 16) + 1) * 16 - n) % 16; }

}  // namespace

extern "C" {

vfi_amt_t* vfi_amt_create(const float* const* tensors, const int64_t* numels, int n_tensors, int variant) {
    const bool known = variant >= 0 && variant <= 2;
    const int want = known ? kCfg[variant].n_tensors : 0;
    if (!tensors || !numels || !known || n_tensors != want) {
        set_error("vfi_amt_create: expected the %d state_dict tensors of %s in amt_spec.amt_shapes() order (variant 0 = S, 1 = L, 2 = G), got %d "
                  "(variant %d)", want, known ? kCfg[variant].name : "AMT-?", n_tensors, variant);
        return nullptr;
    }
    vfi_amt* m = new vfi_amt();
    m->variant = variant;
    const Cfg& g = kCfg[variant];
    const bool basic = variant >= 1, G = variant == 2;
    TensorCursor cur(tensors, numels, n_tensors, "vfi_amt_create");
    // Conv2d (kind 0) / ConvTranspose2d (kind 1) with bias, then the PReLU slopes where the layer has them
    auto layer = [&](int kind, int cout, int cin, int k, int stride, bool prelu, const int* map = nullptr, int cin_phys = 0) {
        return m->read_layer(cur, kind, cout, cin, k, stride, true, prelu, map, cin_phys);
    };
    std::vector<float> tmp;
    // Conv2d(3, cout, 7, 2, 3) [+ PReLU] for vfi_conv7x7s2_prelu: [7][7][3][P], P = 64 with the missing output channels zero, or AMT-G's 84
    // as they are (the two widths the kernel is instantiated for); slope 1 = no activation
    auto stem = [&](Stem& s, int cout, bool prelu) {
        const float* w = cur.take((int64_t)cout * 3 * 49);
        const float* b = cur.take(cout);
        const float* p = prelu ? cur.take(cout) : nullptr;
        if (!cur.ok()) return;
        const int P = cout <= 64 ? 64 : 84;
        tmp.assign((size_t)49 * 3 * P, 0.f);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < 3; ++ci)
                for (int t = 0; t < 49; ++t) tmp[((size_t)t * 3 + ci) * P + co] = w[((size_t)co * 3 + ci) * 49 + t];
        s.w = m->upload(tmp.data(), tmp.size());
        tmp.assign(P, 0.f);
        memcpy(tmp.data(), b, cout * sizeof(float));
        s.b = m->upload(tmp.data(), P);
        tmp.assign(P, 1.f);
        if (p) memcpy(tmp.data(), p, cout * sizeof(float));
        s.slope = m->upload(tmp.data(), P);
        s.cout = P;
    };
    // Conv2d(cin, cout, 7, 1, 3) [+ PReLU] for vfi_conv7x7: [7][7][Cin4][CoutP]
    auto conv7 = [&](Conv7& c, int cout, int cin, bool prelu) {
        const float* w = cur.take((int64_t)cout * cin * 49);
        const float* b = cur.take(cout);
        const float* p = prelu ? cur.take(cout) : nullptr;
        if (!cur.ok()) return;
        const int cin4 = (cin + 3) & ~3, co = cout <= 4 ? 4 : 16, coutp = round_up(cout, co);
        tmp.assign((size_t)49 * cin4 * coutp, 0.f);
        for (int o = 0; o < cout; ++o)
            for (int i = 0; i < cin; ++i)
                for (int t = 0; t < 49; ++t) tmp[((size_t)t * cin4 + i) * coutp + o] = w[((size_t)o * cin + i) * 49 + t];
        c.w = m->upload(tmp.data(), tmp.size());
        c.b = m->upload(b, cout);
        if (p) c.pr = m->upload(p, cout);
        c.cin = cin, c.cout = cout;
    };
    // feature encoder
    stem(m->fe_stem, g.e1, false);
    int cin = g.e1;
    for (int i = 0; i < g.n_enc; ++i) {
        const int c = g.enc[i];
        for (int b = 0; b < 2; ++b) {
            EncBlk& B = m->blk[2 * i + b];
            B.cin = b == 0 ? cin : c, B.c = c, B.stride = b == 0 ? g.enc_stride[i] : 1;
            if (!basic) {
                B.c1 = layer(0, c / 4, B.cin, 1, 1, false);
                B.c2 = layer(0, c / 4, c / 4, 3, B.stride, false);
                B.c3 = layer(0, c, c / 4, 1, 1, false);
            } else {
                B.c1 = layer(0, c, B.cin, 3, B.stride, false);
                B.c2 = layer(0, c, c, 3, 1, false);
            }
            if (B.stride == 2) B.ds = layer(0, c, B.cin, 1, 1, false);
        }
        cin = c;
    }
    m->fe_out = layer(0, g.D, cin, 1, 1, false);
    // pyramid encoder
    int prev = 3;
    for (int i = 0; i < 4; ++i) {
        if (basic && i == 0) stem(m->py_stem, g.ch[0], true);
        else m->py0[i] = layer(0, g.ch[i], prev, 3, 2, true, nullptr, (basic && !G && i == 1) ? 64 : 0);
        m->py1[i] = layer(0, g.ch[i], g.ch[i], 3, 1, true, nullptr, (basic && !G && i == 0) ? 64 : 0);
        prev = g.ch[i];
    }
    // decoders
    const int dcin[4] = {2 * g.ch[3] + 1, 3 * g.ch[2] + 4, 3 * g.ch[1] + 4, 3 * g.ch[0] + 4};
    const int dc[4] = {2 * g.ch[3], 3 * g.ch[2], 3 * g.ch[1], 3 * g.ch[0]};
    const int dco[4] = {g.ch[2] + 4, g.ch[1] + 4, g.ch[0] + 4, 8 * g.nf};
    std::vector<int> map;
    for (int k = 0; k < 4; ++k) {
        Dec& d = m->dec[k];
        d.cin = dcin[k], d.c = dc[k], d.cout = dco[k];
        const int c = d.c, off = r8(c) + 8, xcs = off + r8(g.skip);
        map.resize(c);
        for (int i = 0; i < c; ++i) map[i] = i < c - g.skip ? i : off + i - (c - g.skip);
        d.c0 = layer(0, c, d.cin, 3, 1, true);
        d.rb[0] = layer(0, c, c, 3, 1, true);
        d.rb[1] = layer(0, g.skip, g.skip, 3, 1, true);
        d.rb[2] = layer(0, c, c, 3, 1, true, map.data(), xcs);
        d.rb[3] = layer(0, g.skip, g.skip, 3, 1, true);
        d.rb[4] = layer(0, c, c, 3, 1, true, map.data(), xcs);      // conv5, then the block's PReLU over x + conv5(...)
        d.up = layer(1, d.cout, c, 4, 2, false);
    }
    // update blocks
    for (int k = 0; k < g.n_upd; ++k) {      // update4, update3[_low], update2[_low], then AMT-G's update3_high, update2_high
        Upd& U = m->upd[k];
        const int cdim = g.ch[k < 3 ? 2 - k : 4 - k], cdo = g.cd2 ? g.cd2 : g.cd;
        U.c1 = layer(0, g.cd, 392, 1, 1, false);
        if (g.cd2) U.c2 = layer(0, g.cd2, g.cd, 3, 1, false);
        conv7(U.f1, 2 * g.fd, 4, false);
        U.f2 = layer(0, g.fd, 2 * g.fd, 3, 1, false);
        U.cv = layer(0, g.fc, cdo + g.fd, 3, 1, false);
        U.g0 = layer(0, g.hid, g.fc + 4 + cdim, 3, 1, false);
        U.g2 = layer(0, g.hid, g.hid, 3, 1, false);
        U.fh0 = layer(0, g.hid, g.hid, 3, 1, false);
        U.fh2 = layer(0, cdim, g.hid, 3, 1, false);
        U.wh0 = layer(0, g.hid, g.hid, 3, 1, false);
        U.wh2 = layer(0, 4, g.hid, 3, 1, false);
    }
    if (basic) {
        conv7(m->cb7[0], 6 * g.nf, 3 * g.nf, true);
        conv7(m->cb7[1], 3, 6 * g.nf, false);
    } else {
        m->cb0 = layer(0, 6 * g.nf, 3 * g.nf, 3, 1, true);
        m->cb2 = layer(0, 3, 6 * g.nf, 3, 1, false);
    }
    if (!cur.finish() || m->failed) {
        vfi_amt_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_amt_destroy(vfi_amt_t* m) { delete m; }

int vfi_amt_release_workspace(vfi_amt_t* m) {
    VFI_REQUIRE(m, "vfi_amt_release_workspace: null object");
    return m->ws.release();
}

int64_t vfi_amt_workspace_bytes(const vfi_amt_t* m) { return m ? m->ws.bytes() : 0; }

// AMT-S / AMT-L: px_floats = 64 is a bound on the frame, not on a buffer (their widest buffers stay below 2 GiB at 2^23 - 1 pixels, where the
// 2^23 comes from the kernels' pixel arithmetic), so the switch has nothing to raise and changes nothing for them.
int64_t vfi_amt_large_max_padded_pixels(int variant) {
    if (variant < 0 || variant > 2) return 0;
    return variant == 2 ? max_padded_pixels_large(kCfg[2].px_floats) : max_padded_pixels(kCfg[variant].px_floats);
}

int64_t vfi_amt_object_max_padded_pixels(const vfi_amt_t* m) {
    return !m ? 0 : (m->large ? max_padded_pixels_large(kCfg[m->variant].px_floats) : max_padded_pixels(kCfg[m->variant].px_floats));
}

// AMT-G: every layer object gets the one permission the forward needs beyond the forms a layer takes on its own (decoder1's rb[4] is
// residual + PReLU on a 2.92 GB input at 2160x3840), and the entry guard takes the 4 GiB bound.  AMT-S / AMT-L: nothing is set.
int vfi_amt_set_large_frames(vfi_amt_t* m, int on) {
    VFI_REQUIRE(m, "vfi_amt_set_large_frames: null object");
    if (m->variant != 2) return 0;
    for (vfi_conv_t* L : m->layers)
        if (vfi_conv_allow_large_res_prelu(L, on != 0)) return -1;
    m->large = on != 0;
    return 0;
}

#ifdef VFI_TEST_TAPS      // include/vfi_hip_test_amt.h: only in libvfi_hip_test.so.  The launches are Run::add's and Run::warp's.
int vfi_test_amt_add(const float* a, int a_cs, int a_w, int step, const float* b, int b_cs, float* out, int out_cs, int h, int w, int C, int reps,
                     void* stream) {
    VFI_REQUIRE(a && out && h > 0 && w > 0 && C > 0 && reps >= 1 && step >= 1 && a_w >= (w - 1) * step + 1 && a_cs >= reps * C && out_cs >= reps * C &&
                    (!b || b_cs >= C),
                "vfi_test_amt_add: bad arguments");
    Run r{{nullptr, (hipStream_t)stream, 0.1f}};
    return r.add(a, a_cs, a_w, step, b, b_cs, out, out_cs, h, w, C, reps);
}

int vfi_test_amt_warp(const float* in, int in_cs, const float* flow, int flow_cs, float* out, int out_cs, int H, int W, int C, void* stream) {
    VFI_REQUIRE(in && flow && out && H > 1 && W > 1 && C > 0 && in_cs >= C && out_cs >= C && flow_cs >= 2, "vfi_test_amt_warp: bad arguments");
    Run r{{nullptr, (hipStream_t)stream, 0.1f}};
    return r.warp(in, in_cs, flow, flow_cs, out, out_cs, H, W, C);
}
#endif

int vfi_amt_forward(vfi_amt_t* m, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, const float* ts_host, int n_t, float* out_dev,
                    void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && ts_host && out_dev && C >= 3 && H > 0 && W > 0 && n_t > 0, "vfi_amt_forward: bad arguments");
    for (int i = 0; i < n_t; ++i)
        VFI_REQUIRE(ts_host[i] > 0.f && ts_host[i] < 1.f, "vfi_amt_forward: timestep %d is %g, outside (0, 1)", i, (double)ts_host[i]);
    const int Hp = amt_pad(H), Wp = amt_pad(W);
    VFI_REQUIRE(Hp >= 128 && Wp >= 128,
                "vfi_amt_forward: a %dx%d frame (padded %dx%d): AMT needs padded sides of at least 128 pixels (below, the coarsest correlation level is "
                "one pixel wide and the reference is all-NaN)", H, W, Hp, Wp);
    const Cfg& g = kCfg[m->variant];      // px_floats: the variant's widest activation, floats per padded pixel
    if (const int rc = m->enter("vfi_amt_forward", g.name, H, W, Hp, Wp, g.px_floats, false, m->large)) return rc;
    return amt_forward(m, frame0_dev, frame1_dev, C, H, W, ts_host, n_t, out_dev, (hipStream_t)stream);
}

}  // extern "C"
