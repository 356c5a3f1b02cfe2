// XVFI (vfi_models/xvfi/xvfi_arch.py XVFInet / VFInet / RefineUNet, inference path): the kernels the network needs beyond the shared layer
// objects, and the network object (vfi_xvfi_create / _forward / ..., at the end of the file) that runs one frame pair at one timestep.
//
//   xvfi_bicubic_down   F.interpolate(x, 1 / l, 'bicubic', align_corners=False) for l = 2, 4, 8, ...: a fixed separable 4-tap filter (:156)
//   xvfi_bwarp          bwarp (:240-268): grid_sample(bilinear, zeros, align_corners=True) times the `mask < 0.999 -> 0` gate
//   xvfi_cfr            Complementary Flow Reversal (:183-198): both z_fwarp splats (:320-415) as a deterministic gather, the numerators,
//                       norm_l and the masked division
//   xvfi_assemble       level 0 (:213-221): the x scale flow upscale, both image warps, pixel_shuffle of the four feature maps: the
//                       RefineUNet's input in one pass
//   xvfi_blend_out      the occlusion blend plus residual (:222-226) and the crop
//   xvfi_same              whether the object's cached pair is the pair it is given (the node's zero pad is net_object.h's pad_frame_pair)
//
// Built with -ffp-contract=off (csrc/build.py): a splat target is the single fp32 product t * flow, and the warps' grid coordinates round
// as torch rounds them.
#include <climits>
#include <cstdio>
#include <cstring>

#include "../../include/vfi_hip.h"
#include "bilinear_src.h"
#include "net_object.h"
#include "vfi_common.h"

namespace vfi {
namespace {

// torch's upsample_bicubic2d with A = -0.75 at the half-pixel phase every output of an even 1 / l reduction has: cubic_convolution2(1.5),
// cubic_convolution1(0.5), cubic_convolution1(0.5), cubic_convolution2(1.5) = -3/32, 19/32, 19/32, -3/32; source rows l i + l / 2 - 2 ...
// l i + l / 2 + 1, clamped to the image.  One thread per output element.
__global__ void xvfi_bicubic_kernel(const float* __restrict__ in, int in_cs, float* __restrict__ out, int out_cs, int N, int H, int W, int C, int l) {
    const int Ho = H / l, Wo = W / l;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * Ho * Wo * C) return;
    const int c = (int)(idx % C);
    const long p = idx / C;
    const int X = (int)(p % Wo), Y = (int)((p / Wo) % Ho), n = (int)(p / ((long)Wo * Ho));
    const float k[4] = {-0.09375f, 0.59375f, 0.59375f, -0.09375f};
    const float* b = in + (size_t)n * H * W * in_cs + c;
    const int y0 = l * Y + l / 2 - 2, x0 = l * X + l / 2 - 2;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = min(max(y0 + i, 0), H - 1);
        float row = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int xx = min(max(x0 + j, 0), W - 1);
            row += k[j] * b[((size_t)yy * W + xx) * in_cs];
        }
        acc += k[i] * row;
    }
    out[(size_t)p * out_cs + c] = acc;
}

// The four taps of bwarp at pixel (x, y) with flow (fx, fy): the reference normalises (2 (x + fx) / max(W - 1, 1) - 1) and grid_sample
// (align_corners=True) un-normalises (((g + 1) / 2) (W - 1)), both in fp32; taps outside the image have offset -1 and weight 0 (zeros
// padding); gate = 0 where the all-ones image sampled the same way is below 0.999 (:260-266), else 1.  A non-finite or far-away position
// has no tap inside and gate 0; it is told before any conversion to an integer.
struct BwTap {
    long off[4];
    float w[4];
    float gate;
};
__device__ inline BwTap bw_taps(int x, int y, float fx, float fy, int H, int W) {
    const float dx = (float)max(W - 1, 1), dy = (float)max(H - 1, 1);
    const float gx = 2.0f * ((float)x + fx) / dx - 1.0f, gy = 2.0f * ((float)y + fy) / dy - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    BwTap t;
    t.gate = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) t.off[k] = -1, t.w[k] = 0.f;
    if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) return t;      // (NaN fails every comparison)
    const float x0f = floorf(ix), y0f = floorf(iy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float ex = (x0f + 1.0f) - ix, wx = ix - x0f, ey = (y0f + 1.0f) - iy, wy = iy - y0f;
    const float w4[4] = {ex * ey, wx * ey, ex * wy, wx * wy};      // nw, ne, sw, se
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
            t.off[k] = (long)yy * W + xx;
            t.w[k] = w4[k];
            m += w4[k];
        }
    }
    t.gate = m < 0.999f ? 0.f : 1.f;
    return t;
}
__device__ inline float bw_sample(const BwTap& t, const float* __restrict__ img, int cs, int c) {
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (t.off[k] >= 0) r += img[(size_t)t.off[k] * cs + c] * t.w[k];
    return r * t.gate;
}

// out[n, y, x, 0..C) = bwarp(in[n or n ^ 1], flow[n]); image n of in / flow / out starts n * {in, flow, out}_ns floats after image 0, so that
// the two directions of a pair can be two channel windows of one tensor.  One thread per pixel and group of four channels (C % 4 == 0:
// float4 accesses) or per pixel (any C).
template <bool VEC>
__global__ void xvfi_bwarp_kernel(const float* __restrict__ in, int in_cs, long in_ns, int in_swap, const float* __restrict__ flow, int flow_cs, long flow_ns,
                                  float* __restrict__ out, int out_cs, long out_ns, int N, int H, int W, int C) {
    const int CQ = VEC ? C / 4 : 1;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)N * H * W * CQ) return;
    const int q = (int)(idx % CQ);
    const long pp = idx / CQ;
    const long p = pp % ((long)H * W);
    const int n = (int)(pp / ((long)H * W));
    const int x = (int)(p % W), y = (int)(p / W);
    const float* f = flow + (size_t)n * flow_ns + (size_t)p * flow_cs;
    const BwTap t = bw_taps(x, y, f[0], f[1], H, W);
    const float* b = in + (size_t)(in_swap ? (n ^ 1) : n) * in_ns;
    float* o = out + (size_t)n * out_ns + (size_t)p * out_cs;
    if (VEC) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t.off[k] >= 0) {
                const float4 v = *(const float4*)(b + (size_t)t.off[k] * in_cs + q * 4);
                r.x += v.x * t.w[k], r.y += v.y * t.w[k], r.z += v.z * t.w[k], r.w += v.w * t.w[k];
            }
        r.x *= t.gate, r.y *= t.gate, r.z *= t.gate, r.w *= t.gate;
        *(float4*)(o + q * 4) = r;
    } else {
        for (int c = 0; c < C; ++c) o[c] = bw_sample(t, b, in_cs, c);
    }
}

// ---- Complementary Flow Reversal ---------------------------------------------------------------------------------------------------------
// z_fwarp(img = flow, flo = s flow, z) (:320-366) for direction d (0: flow_01 with s = t, 1: flow_10 with s = 1 - t): source (sr, sc) splats
// flow[sr, sc] with weight (sigmoid(z) + 1e-5) exp(-((ty - (Fy + a))^2 + (tx - (Fx + b))^2)) onto the cells (sr + Fy + a, sc + Fx + b), a, b
// in {0, 1}, where ty = s fy, tx = s fx (one fp32 product each), Fy = floor(ty), Fx = floor(tx).  A source whose four cells all lie
// outside the image, or whose target is not finite, contributes nothing: it is told on the floats, before any conversion.
struct CfrSrc {
    int Fy, Fx;      // valid only when ok
    float ty, tx;
    bool ok;
};
__device__ inline CfrSrc cfr_src(float fx, float fy, float s, int sr, int sc, int h, int w) {
    CfrSrc r;
    r.ty = s * fy, r.tx = s * fx;
    const float Fy = floorf(r.ty), Fx = floorf(r.tx);
    // sr + Fy in [-1, h - 1] and sc + Fx in [-1, w - 1]: at least one of the four cells is inside (NaN fails)
    r.ok = Fy >= (float)(-1 - sr) && Fy <= (float)(h - 1 - sr) && Fx >= (float)(-1 - sc) && Fx <= (float)(w - 1 - sc);
    r.Fy = r.ok ? (int)Fy : 0, r.Fx = r.ok ? (int)Fx : 0;
    return r;
}

// bounds[d * 4 + 0..3] = (min Fy, max Fy, min Fx, max Fx) over the contributing sources of direction d (min > max: none).  One workgroup;
// integer minima and maxima, so the order of the reduction is immaterial.
__global__ __launch_bounds__(1024) void xvfi_cfr_bounds_kernel(const float* __restrict__ flow, int flow_cs, float t, int h, int w, int* __restrict__ bounds) {
    __shared__ int red[8][1024];
    int b[8] = {INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN, INT_MAX, INT_MIN};
    const float s2[2] = {t, 1.0f - t};
    for (long p = threadIdx.x; p < (long)h * w; p += 1024) {
        const int sr = (int)(p / w), sc = (int)(p % w);
        const float* f = flow + (size_t)p * flow_cs;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const CfrSrc s = cfr_src(f[2 * d], f[2 * d + 1], s2[d], sr, sc, h, w);
            if (s.ok) {
                b[4 * d] = min(b[4 * d], s.Fy), b[4 * d + 1] = max(b[4 * d + 1], s.Fy);
                b[4 * d + 2] = min(b[4 * d + 2], s.Fx), b[4 * d + 3] = max(b[4 * d + 3], s.Fx);
            }
        }
    }
    for (int k = 0; k < 8; ++k) red[k][threadIdx.x] = b[k];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 8; ++k) {
                const int a = red[k][threadIdx.x], c = red[k][threadIdx.x + o];
                red[k][threadIdx.x] = (k & 1) ? max(a, c) : min(a, c);
            }
        __syncthreads();
    }
    if (threadIdx.x < 8) bounds[threadIdx.x] = red[threadIdx.x][0];
}

// One thread per target cell (r, c).  The sources that can reach it lie in sr in [r - maxFy - 1, r - minFy], sc in [c - maxFx - 1, c - minFx]
// (xvfi_cfr_bounds_kernel): they are visited in row-major order and each adds at most one of its four corners, so the sums have one fixed
// order and the same inputs give the same bits.  Then the numerators of Eq. (1) / (2), norm_l and the masked division (:192-198).
__global__ void xvfi_cfr_kernel(const float* __restrict__ flow, int flow_cs, const float* __restrict__ z, int z_cs, float t, const int* __restrict__ bounds,
                                float* __restrict__ out, int out_cs, int h, int w) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)h * w) return;
    const int r = (int)(idx / w), c = (int)(idx % w);
    const float omt = 1.0f - t;
    const float s2[2] = {t, omt};
    float img[2][2], nrm[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        float ax = 0.f, ay = 0.f, an = 0.f;
        const int minFy = bounds[4 * d], maxFy = bounds[4 * d + 1], minFx = bounds[4 * d + 2], maxFx = bounds[4 * d + 3];
        if (minFy <= maxFy && minFx <= maxFx) {
            const int r0 = max(r - maxFy - 1, 0), r1 = min(r - minFy, h - 1), c0 = max(c - maxFx - 1, 0), c1 = min(c - minFx, w - 1);
            for (int sr = r0; sr <= r1; ++sr)
                for (int sc = c0; sc <= c1; ++sc) {
                    const size_t sp = (size_t)sr * w + sc;
                    const float fx = flow[sp * flow_cs + 2 * d], fy = flow[sp * flow_cs + 2 * d + 1];
                    const CfrSrc s = cfr_src(fx, fy, s2[d], sr, sc, h, w);
                    if (!s.ok) continue;
                    const int a = r - sr - s.Fy, b = c - sc - s.Fx;
                    if (a < 0 || a > 1 || b < 0 || b > 1) continue;
                    const float zz = 1.0f / (1.0f + expf(-z[sp * z_cs + d])) + 1e-5f;
                    const float ey = s.ty - (float)(s.Fy + a), ex = s.tx - (float)(s.Fx + b);
                    const float wgt = zz * expf(-(ey * ey + ex * ex));
                    ax += fx * wgt, ay += fy * wgt, an += wgt;
                }
        }
        img[d][0] = ax, img[d][1] = ay, nrm[d] = an;
    }
    const float norm = omt * nrm[0] + t * nrm[1];
    float* o = out + (size_t)idx * out_cs;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float ff = img[0][k], fb = img[1][k];
        float f0 = (-omt) * (t * ff) + t * (t * fb);
        float f1 = omt * (omt * ff) - t * (omt * fb);
        if (norm > 0.f) f0 = f0 / norm, f1 = f1 / norm;
        o[k] = f0, o[2 + k] = f1;
    }
}

// The RefineUNet's input at full resolution, one thread per pixel (Y, X) of Hp x Wp (:213-221):
//   channels 0 .. cps           pixel_shuffle(cat(feat0, feat1, warped0, warped1), s): channel c from channel c s^2 + (Y % s) s + X % s of the cat
//   cps + 0 .. 5                frame 0, frame 1
//   cps + 6 .. 11               bwarp(frame 0, flow_t0), bwarp(frame 1, flow_t1)
//   cps + 12 .. 15              flow_t0, flow_t1 = s * F.interpolate(flow, scale_factor=s, 'bilinear', align_corners=False)
// feat [2,h,w,feat_cs] (64 channels used), warped [2,h,w,warped_cs], fr [h,w,fr_cs] (4 channels), img [2,Hp,Wp,img_cs]; cps = 256 / s^2.
__global__ void xvfi_assemble_kernel(const float* __restrict__ feat, int feat_cs, const float* __restrict__ warped, int warped_cs, const float* __restrict__ fr,
                                     int fr_cs, const float* __restrict__ img, int img_cs, float* __restrict__ out, int out_cs, int h, int w, int s) {
    const int Hp = h * s, Wp = w * s, cps = 256 / (s * s);
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)Hp * Wp) return;
    const int X = (int)(idx % Wp), Y = (int)(idx / Wp);
    float* o = out + (size_t)idx * out_cs;
    const size_t lp = (size_t)(Y / s) * w + X / s, hw = (size_t)h * w;
    const int sub = (Y % s) * s + X % s;
    for (int c = 0; c < cps; ++c) {
        const int ch = c * s * s + sub, m = ch >> 6, cc = ch & 63;
        o[c] = m < 2 ? feat[((size_t)m * hw + lp) * feat_cs + cc] : warped[((size_t)(m - 2) * hw + lp) * warped_cs + cc];
    }
    const float ratio = 1.0f / (float)s;
    const BilS by = bil_src(Y, ratio, h), bx = bil_src(X, ratio, w);
    const float *p00 = fr + ((size_t)by.i0 * w + bx.i0) * fr_cs, *p01 = fr + ((size_t)by.i0 * w + bx.i1) * fr_cs;
    const float *p10 = fr + ((size_t)by.i1 * w + bx.i0) * fr_cs, *p11 = fr + ((size_t)by.i1 * w + bx.i1) * fr_cs;
    float fl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) fl[k] = (float)s * (by.w0 * (bx.w0 * p00[k] + bx.w1 * p01[k]) + by.w1 * (bx.w0 * p10[k] + bx.w1 * p11[k]));
    const float *i0 = img, *i1 = img + (size_t)Hp * Wp * img_cs;
    const BwTap t0 = bw_taps(X, Y, fl[0], fl[1], Hp, Wp), t1 = bw_taps(X, Y, fl[2], fl[3], Hp, Wp);
    float* q = o + cps;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q[k] = i0[(size_t)idx * img_cs + k];
        q[3 + k] = i1[(size_t)idx * img_cs + k];
        q[6 + k] = bw_sample(t0, i0, img_cs, k);
        q[9 + k] = bw_sample(t1, i1, img_cs, k);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) q[12 + k] = fl[k];
}

// out [H,W,3] = ((1 - t) occ0 w0 + t occ1 w1) / ((1 - t) occ0 + t occ1) + res, occ0 = sigmoid(ro[0]), occ1 = 1 - occ0, res = ro[1..3]; w0 / w1:
// the warped frames, three channels each at w_dev / w_dev + 3 (:222-226); the H x W crop of the padded Hp x Wp result, not clamped
__global__ void xvfi_blend_kernel(const float* __restrict__ ro, int ro_cs, const float* __restrict__ wimg, int w_cs, float t, float* __restrict__ out, int Wp,
                                  int H, int W) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int X = (int)(idx % W), Y = (int)(idx / W);
    const size_t p = (size_t)Y * Wp + X;
    const float* r = ro + p * ro_cs;
    const float* wv = wimg + p * w_cs;
    const float omt = 1.0f - t;
    const float occ0 = 1.0f / (1.0f + expf(-r[0])), occ1 = 1.0f - occ0;
    const float a = omt * occ0, b = t * occ1, den = a + b;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)idx * 3 + k] = (a * wv[k] + b * wv[3 + k]) / den + r[1 + k];
}

// *differs |= 1 where a frame's bits are not the padded copy's: whether the features the object holds are this pair's (bit compare, so
// that a NaN pixel equals itself)
__global__ void xvfi_same_kernel(const float* __restrict__ f0, const float* __restrict__ f1, int C, int H, int W, const float* __restrict__ img, int Hp, int Wp,
                                 int* __restrict__ differs) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int X = (int)(idx % W), Y = (int)(idx / W);
    const unsigned* s = (const unsigned*)((blockIdx.y ? f1 : f0) + (size_t)idx * C);
    const unsigned* o = (const unsigned*)(img + ((size_t)blockIdx.y * Hp * Wp + (size_t)Y * Wp + X) * 8);
    if (s[0] != o[0] || s[1] != o[1] || s[2] != o[2]) atomicOr(differs, 1);
}

}  // namespace
}  // namespace vfi

using namespace vfi;

extern "C" {

int vfi_xvfi_bicubic_down(const float* in_dev, int in_cs, float* out_dev, int out_cs, int N, int H, int W, int C, int l, void* stream) {
    VFI_REQUIRE(in_dev && out_dev && N > 0 && C > 0 && in_cs >= C && out_cs >= C, "vfi_xvfi_bicubic_down: bad arguments");
    VFI_REQUIRE(l >= 2 && (l & (l - 1)) == 0 && H >= l && W >= l && H % l == 0 && W % l == 0,
                "vfi_xvfi_bicubic_down: l = %d must be a power of two >= 2 that divides %dx%d", l, H, W);
    const long total = (long)N * (H / l) * (W / l) * C;
    VFI_REQUIRE(total / 256 < 0x7fffffffL, "vfi_xvfi_bicubic_down: %d x %dx%d x %d is beyond the kernel's index arithmetic", N, H, W, C);
    TraceScope ts("xvfi_bicubic", (hipStream_t)stream);
    hipLaunchKernelGGL(xvfi_bicubic_kernel, dim3(nblk(total, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, out_dev, out_cs, N, H, W, C, l);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_xvfi_bwarp(const float* in_dev, int in_cs, int64_t in_ns, int in_swap, const float* flow_dev, int flow_cs, int64_t flow_ns, float* out_dev,
                   int out_cs, int64_t out_ns, int N, int H, int W, int C, void* stream) {
    VFI_REQUIRE(in_dev && flow_dev && out_dev && N > 0 && H > 0 && W > 0 && C > 0 && in_cs >= C && out_cs >= C && flow_cs >= 2 && in_ns >= 0 &&
                    flow_ns >= 0 && out_ns >= 0,
                "vfi_xvfi_bwarp: bad arguments");
    VFI_REQUIRE(!in_swap || N % 2 == 0, "vfi_xvfi_bwarp: the partner-image swap needs an even batch (N = %d)", N);
    VFI_REQUIRE((long)H * W < 0x7fffffffL && (long)N * H * W * C / 256 < 0x7fffffffL, "vfi_xvfi_bwarp: %d x %dx%d x %d is beyond the kernel's index arithmetic",
                N, H, W, C);
    TraceScope ts("xvfi_bwarp", (hipStream_t)stream);
    const bool vec = C % 4 == 0 && in_cs % 4 == 0 && out_cs % 4 == 0 && in_ns % 4 == 0 && out_ns % 4 == 0 && aligned16(in_dev) && aligned16(out_dev);
    if (vec)
        hipLaunchKernelGGL(xvfi_bwarp_kernel<true>, dim3(nblk((long)N * H * W * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, (long)in_ns,
                           in_swap, flow_dev, flow_cs, (long)flow_ns, out_dev, out_cs, (long)out_ns, N, H, W, C);
    else
        hipLaunchKernelGGL(xvfi_bwarp_kernel<false>, dim3(nblk((long)N * H * W, 256)), dim3(256), 0, (hipStream_t)stream, in_dev, in_cs, (long)in_ns, in_swap,
                           flow_dev, flow_cs, (long)flow_ns, out_dev, out_cs, (long)out_ns, N, H, W, C);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_xvfi_cfr(const float* flow_dev, int flow_cs, const float* z_dev, int z_cs, float t, float* out_dev, int out_cs, void* scratch_dev, int h, int w,
                 void* stream) {
    VFI_REQUIRE(flow_dev && z_dev && out_dev && scratch_dev && flow_cs >= 4 && z_cs >= 2 && out_cs >= 4 && h > 0 && w > 0, "vfi_xvfi_cfr: bad arguments");
    VFI_REQUIRE(t >= 0.f && t <= 1.f, "vfi_xvfi_cfr: t = %g outside [0, 1]", (double)t);
    VFI_REQUIRE((long)h * w * flow_cs < 0x7fffffffL && (long)h * w * out_cs < 0x7fffffffL, "vfi_xvfi_cfr: a %dx%d map is beyond the kernel's index arithmetic", h, w);
    TraceScope ts("xvfi_cfr", (hipStream_t)stream);
    hipLaunchKernelGGL(xvfi_cfr_bounds_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, flow_dev, flow_cs, t, h, w, (int*)scratch_dev);
    hipLaunchKernelGGL(xvfi_cfr_kernel, dim3(nblk((long)h * w, 64)), dim3(64), 0, (hipStream_t)stream, flow_dev, flow_cs, z_dev, z_cs, t, (const int*)scratch_dev,
                       out_dev, out_cs, h, w);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_xvfi_assemble(const float* feat_dev, int feat_cs, const float* warped_dev, int warped_cs, const float* flow_dev, int flow_cs, const float* img_dev,
                      int img_cs, float* out_dev, int out_cs, int h, int w, int scale, void* stream) {
    VFI_REQUIRE(feat_dev && warped_dev && flow_dev && img_dev && out_dev && h > 0 && w > 0 && (scale == 2 || scale == 4), "vfi_xvfi_assemble: bad arguments (scale 2 or 4)");
    VFI_REQUIRE(feat_cs >= 64 && warped_cs >= 64 && flow_cs >= 4 && img_cs >= 3 && out_cs >= 256 / (scale * scale) + 16,
                "vfi_xvfi_assemble: strides too small (features 64, flows 4, frames 3, output %d channels)", 256 / (scale * scale) + 16);
    VFI_REQUIRE((long)h * scale * w * scale * out_cs < (1L << 31) && (long)h * w * feat_cs < (1L << 30),
                "vfi_xvfi_assemble: a %dx%d map at scale %d is beyond the kernel's index arithmetic", h, w, scale);
    TraceScope ts("xvfi_assemble", (hipStream_t)stream);
    hipLaunchKernelGGL(xvfi_assemble_kernel, dim3(nblk((long)h * scale * w * scale, 256)), dim3(256), 0, (hipStream_t)stream, feat_dev, feat_cs, warped_dev,
                       warped_cs, flow_dev, flow_cs, img_dev, img_cs, out_dev, out_cs, h, w, scale);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_xvfi_blend_out(const float* refine_dev, int refine_cs, const float* warped_dev, int warped_cs, float t, float* out_dev, int Hp, int Wp, int H, int W,
                       void* stream) {
    VFI_REQUIRE(refine_dev && warped_dev && out_dev && refine_cs >= 4 && warped_cs >= 6 && H > 0 && W > 0 && H <= Hp && W <= Wp, "vfi_xvfi_blend_out: bad arguments");
    VFI_REQUIRE((long)Hp * Wp * warped_cs < (1L << 31) * 4, "vfi_xvfi_blend_out: a %dx%d frame is beyond the kernel's index arithmetic", Hp, Wp);
    TraceScope ts("xvfi_blend", (hipStream_t)stream);
    hipLaunchKernelGGL(xvfi_blend_kernel, dim3(nblk((long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, refine_dev, refine_cs, warped_dev, warped_cs, t, out_dev,
                       Wp, H, W);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---- the network object on csrc/net_object.h -------------------------------------------------------------------------------------------------

namespace {

constexpr int NF = 64;
constexpr int kMaxLevels = 8;
// the widest per-image buffer, floats per padded pixel: the RefineUNet's input at scale 2 (64 shuffled channels + 16); the layers index
// an image with 32 bits of bytes, signed (the limit of every object as created) or unsigned (after vfi_xvfi_set_large_frames)
constexpr int kPxFloats = 80;

struct Tower {      // Conv2d(4, 2, 1), Conv2d(4, 2, 1), up 2 + 3x3, up 2 + 3x3, 3x3: conv_flow_bottom / conv_flow2 / conv_flow3 after its 1x1
    vfi_conv_t *d1 = nullptr, *d2 = nullptr, *u1 = nullptr, *u2 = nullptr, *o = nullptr;
};

}  // namespace

struct vfi_xvfi : PaddedNet {
    int scale = 2, S = 1, nds = 1;      // module_scale_factor, S_tst, log2(scale)
    vfi_conv_t *cc = nullptr, *ext_ds = nullptr, *ext_c = nullptr, *rb[4] = {}, *ctx_ds = nullptr;
    Tower bottom, flow2, flow3;
    vfi_conv_t *flow1 = nullptr, *flow3_in = nullptr;
    vfi_conv_t *enc1 = nullptr, *enc2 = nullptr, *enc3 = nullptr, *dec0 = nullptr, *dec1 = nullptr, *dec2 = nullptr, *dec3 = nullptr;
    int H = 0, W = 0;            // the frame size is part of the workspace key too: the kept pair is compared against the padded copy
    bool large = false;          // vfi_xvfi_set_large_frames: padded frames up to max_padded_pixels_large(kPxFloats) are served
    bool have_pair = false;      // the workspace holds the features, the level flows and flow_l_tmp of the pair whose padded copy is "img"
    int* flag_host = nullptr;    // pinned: xvfi_same_kernel's verdict
};

namespace {

struct Run : NetRun<vfi_xvfi> {      // conv's act: 0 none, 1 ReLU
    int copy(const float* a, int a_cs, float* out, int out_cs, long px, int C) { return vfi_axpby(a, a_cs, nullptr, 0, out, out_cs, px, C, 1.f, 0.f, st); }
    int up2(const float* in, int ics, int h, int w, float* out, int ocs, int C) { return vfi_upsample_nearest(in, ics, out, ocs, 1, h, w, 2 * h, 2 * w, C, st); }
};

// in [h,w,ics] -> out [h,w,8] (+ res); h, w multiples of 4.  UpsamplingNearest2d(2) is the nearest resize in front of its 3x3 layer, not fused.
int run_tower(Run& r, const Tower& T, const float* in, int ics, int h, int w, float* out, const float* res = nullptr, int rcs = 0) {
    float *t1 = r.buf("tw_t1", 1, h / 2, w / 2, 2 * NF), *t2 = r.buf("tw_t2", 1, h / 4, w / 4, 4 * NF), *u1 = r.buf("tw_u1", 1, h / 2, w / 2, 4 * NF);
    float *t3 = r.buf("tw_t3", 1, h / 2, w / 2, 2 * NF), *u2 = r.buf("tw_u2", 1, h, w, 2 * NF), *t4 = r.buf("tw_t4", 1, h, w, NF);
    if (r.bad) return -1;
    VFI_DO(r.conv(T.d1, in, ics, h, w, t1, 2 * NF, 1, 1));
    VFI_DO(r.conv(T.d2, t1, 2 * NF, h / 2, w / 2, t2, 4 * NF, 1, 1));
    VFI_DO(r.up2(t2, 4 * NF, h / 4, w / 4, u1, 4 * NF, 4 * NF));
    VFI_DO(r.conv(T.u1, u1, 4 * NF, h / 2, w / 2, t3, 2 * NF, 1, 1));
    VFI_DO(r.up2(t3, 2 * NF, h / 2, w / 2, u2, 2 * NF, 2 * NF));
    VFI_DO(r.conv(T.u2, u2, 2 * NF, h, w, t4, NF, 1, 1));
    return r.conv(T.o, t4, NF, h, w, out, 8, 1, 0, res, rcs);
}

const char* lname(const char* base, int l, char (&buf)[24]) {
    snprintf(buf, sizeof(buf), "%s%d", base, l);
    return buf;
}

// once per pair: the zero pad, the features of both frames at every level (XVFInet.forward :53-58), the flows of levels S .. 1 and level
// 0's flow_l_tmp / flow_l (VFInet.forward :165-178): none of it depends on t
int xvfi_prepare(vfi_xvfi* m, const float* f0, const float* f1, int C, hipStream_t st) {
    Run r{{m, st}};
    const int Hp = m->Hp, Wp = m->Wp, s = m->scale, h0 = Hp / s, w0 = Wp / s;
    char nb[24];
    float* img = r.buf("img", 2, Hp, Wp, 8);
    if (r.bad) return -1;
    VFI_DO(pad_frame_pair(f0, f1, C, m->H, m->W, img, Hp, Wp, 0, 0, false, st));      // F.pad(frames, (0, Wp - W, 0, Hp - H)): zeros
    // channel_converter, rec_ext_ds x log2(scale), the 3x3 layer, RResBlock2D_3D: Conv3d layers with temporal kernel 1 = a batch of two frames
    float* F[kMaxLevels];
    {
        float* x = r.buf("fe_cc", 2, Hp, Wp, NF);
        if (r.bad) return -1;
        VFI_DO(r.conv(m->cc, img, 8, Hp, Wp, x, NF, 2, 1));
        int h = Hp, w = Wp;
        for (int i = 0; i < m->nds; ++i) {
            float* y = r.buf(lname("fe_ds", i, nb), 2, h / 2, w / 2, NF);
            if (r.bad) return -1;
            VFI_DO(r.conv(m->ext_ds, x, NF, h, w, y, NF, 2, 1));
            x = y, h /= 2, w /= 2;
        }
        float *x0 = r.buf("fe_x0", 2, h, w, NF), *t1 = r.buf("fe_t1", 2, h, w, NF), *y1 = r.buf("fe_y1", 2, h, w, NF), *y2 = r.buf("fe_y2", 2, h, w, NF);
        F[0] = r.buf("feat0", 2, h, w, 2 * NF);
        if (r.bad) return -1;
        VFI_DO(r.conv(m->ext_c, x, NF, h, w, x0, NF, 2, 0));
        VFI_DO(r.conv(m->rb[0], x0, NF, h, w, t1, NF, 2, 1));
        VFI_DO(r.conv(m->rb[1], t1, NF, h, w, y1, NF, 2, 0, x0, NF));
        VFI_DO(r.conv(m->rb[2], y1, NF, h, w, t1, NF, 2, 1));
        VFI_DO(r.conv(m->rb[3], t1, NF, h, w, y2, NF, 2, 0, y1, NF));
        VFI_DO(vfi_axpby(y2, NF, x0, NF, F[0], 2 * NF, 2L * h * w, NF, 1.f, 1.f, st));
        for (int l = 1; l <= m->S; ++l) {
            F[l] = r.buf(lname("feat", l, nb), 2, h0 >> l, w0 >> l, 2 * NF);
            if (r.bad) return -1;
            VFI_DO(r.conv(m->ctx_ds, F[l - 1], 2 * NF, h0 >> (l - 1), w0 >> (l - 1), F[l], 2 * NF, 2, 0));
        }
    }
    // the recursion: flow_l [h,w,4] per level in "flow<l>", level 0's flow_l_tmp (6 channels) in "tmp0"
    const float* prev = nullptr;
    for (int l = m->S; l >= 0; --l) {
        const int h = h0 >> l, w = w0 >> l;
        const size_t hw = (size_t)h * w;
        float *tmp = r.buf(lname("tmp", l, nb), 1, h, w, 8), *fl = r.buf(lname("flow", l, nb), 1, h, w, 4);
        if (r.bad) return -1;
        if (!prev) {
            float* B = r.buf(lname("cat", l, nb), 1, h, w, 2 * NF);
            if (r.bad) return -1;
            VFI_DO(r.copy(F[l], 2 * NF, B, 2 * NF, (long)hw, NF));
            VFI_DO(r.copy(F[l] + hw * 2 * NF, 2 * NF, B + NF, 2 * NF, (long)hw, NF));
            VFI_DO(run_tower(r, m->bottom, B, 2 * NF, h, w, tmp));
            VFI_DO(r.copy(tmp, 8, fl, 4, (long)hw, 4));
        } else {
            const int gcs = 2 * NF + 8;
            float *G = r.buf(lname("cf", l, nb), 1, h, w, gcs), *CF = r.buf(lname("cf1_", l, nb), 2, h, w, NF);
            if (r.bad) return -1;
            float* up = G + 2 * NF;      // up_flow_l_prev: channels 128..131 of conv_flow2's input
            VFI_DO(vfi_resize_bilinear(prev, 4, up, gcs, 1, h / 2, w / 2, h, w, 4, 2.0f, st));
            // warped_feat1 = bwarp(feat1, up[:, :2]) beside feat0, warped_feat0 = bwarp(feat0, up[:, 2:]) beside feat1: conv_flow1's two inputs
            VFI_DO(vfi_xvfi_bwarp(F[l], 2 * NF, (int64_t)hw * 2 * NF, 1, up, gcs, 2, F[l] + NF, 2 * NF, (int64_t)hw * 2 * NF, 2, h, w, NF, st));
            VFI_DO(r.conv(m->flow1, F[l], 2 * NF, h, w, CF, NF, 2, 0));
            VFI_DO(r.copy(CF, NF, G, gcs, (long)hw, NF));
            VFI_DO(r.copy(CF + hw * NF, NF, G + NF, gcs, (long)hw, NF));
            VFI_DO(run_tower(r, m->flow2, G, gcs, h, w, tmp));
            VFI_DO(vfi_axpby(tmp, 8, up, gcs, fl, 4, (long)hw, 4, 1.f, 1.f, st));
        }
        prev = fl;
    }
    // conv_flow3's input: feat0 | warped0 | warped1 | feat1 | flow_t0 | flow_t1 (260 of 264 channels); the features are the pair's
    float* R = r.buf("refine_in", 1, h0, w0, 4 * NF + 8);
    if (r.bad) return -1;
    const size_t hw0 = (size_t)h0 * w0;
    VFI_DO(r.copy(F[0], 2 * NF, R, 4 * NF + 8, (long)hw0, NF));
    VFI_DO(r.copy(F[0] + hw0 * 2 * NF, 2 * NF, R + 3 * NF, 4 * NF + 8, (long)hw0, NF));
    return 0;
}

// per timestep: level 0 from the CFR on (VFInet.forward :183-226)
int xvfi_render(vfi_xvfi* m, float t, float* out, hipStream_t st) {
    Run r{{m, st}};
    const int Hp = m->Hp, Wp = m->Wp, s = m->scale, h = Hp / s, w = Wp / s, rcs = 4 * NF + 8;
    const size_t hw = (size_t)h * w;
    const int cps = 256 / (s * s), ucs = cps + 16;
    float *img = r.buf("img", 2, Hp, Wp, 8), *F0 = r.buf("feat0", 2, h, w, 2 * NF), *tmp = r.buf("tmp0", 1, h, w, 8), *fl = r.buf("flow0", 1, h, w, 4);
    float *R = r.buf("refine_in", 1, h, w, rcs), *bounds = r.buf("cfr_bounds", 1, 1, 1, 8), *c1 = r.buf("f3_in", 1, h, w, NF), *FR = r.buf("flow_refined", 1, h, w, 8);
    float *WF = r.buf("warped", 2, h, w, NF), *U = r.buf("unet_in", 1, Hp, Wp, ucs);
    float *D2 = r.buf("unet_d2", 1, Hp / 2, Wp / 2, 3 * NF), *D1 = r.buf("unet_d1", 1, Hp / 4, Wp / 4, 6 * NF), *E3 = r.buf("unet_e3", 1, Hp / 8, Wp / 8, 4 * NF);
    float *T0 = r.buf("unet_t0", 1, Hp / 8, Wp / 8, 4 * NF), *T1 = r.buf("unet_t1", 1, Hp / 4, Wp / 4, 2 * NF), *T2 = r.buf("unet_t2", 1, Hp / 2, Wp / 2, NF);
    float *T3 = r.buf("unet_t3", 1, Hp, Wp, NF), *RO = r.buf("unet_out", 1, Hp, Wp, 8);
    if (r.bad) return -1;
    VFI_DO(vfi_xvfi_cfr(fl, 4, tmp + 4, 8, t, R + 4 * NF, rcs, bounds, h, w, st));
    // warped0 = bwarp(feat0, flow_t0) -> channels 64.., warped1 = bwarp(feat1, flow_t1) -> channels 128..
    VFI_DO(vfi_xvfi_bwarp(F0, 2 * NF, (int64_t)hw * 2 * NF, 0, R + 4 * NF, rcs, 2, R + NF, rcs, NF, 2, h, w, NF, st));
    VFI_DO(r.conv(m->flow3_in, R, rcs, h, w, c1, NF, 1, 1));
    VFI_DO(run_tower(r, m->flow3, c1, NF, h, w, FR, R + 4 * NF, rcs));
    VFI_DO(vfi_xvfi_bwarp(F0, 2 * NF, (int64_t)hw * 2 * NF, 0, FR, 8, 2, WF, NF, (int64_t)hw * NF, 2, h, w, NF, st));
    VFI_DO(vfi_xvfi_assemble(F0, 2 * NF, WF, NF, FR, 8, img, 8, U, ucs, h, w, s, st));
    // RefineUNet (:436-453): the two concats are channel windows of D1 / D2 (decoder output first, encoder map behind)
    VFI_DO(r.conv(m->enc1, U, ucs, Hp, Wp, D2 + 2 * NF, 3 * NF, 1, 1));
    VFI_DO(r.conv(m->enc2, D2 + 2 * NF, 3 * NF, Hp / 2, Wp / 2, D1 + 4 * NF, 6 * NF, 1, 1));
    VFI_DO(r.conv(m->enc3, D1 + 4 * NF, 6 * NF, Hp / 4, Wp / 4, E3, 4 * NF, 1, 1));
    VFI_DO(r.conv(m->dec0, E3, 4 * NF, Hp / 8, Wp / 8, T0, 4 * NF, 1, 1));
    VFI_DO(r.up2(T0, 4 * NF, Hp / 8, Wp / 8, D1, 6 * NF, 4 * NF));
    VFI_DO(r.conv(m->dec1, D1, 6 * NF, Hp / 4, Wp / 4, T1, 2 * NF, 1, 1));
    VFI_DO(r.up2(T1, 2 * NF, Hp / 4, Wp / 4, D2, 3 * NF, 2 * NF));
    VFI_DO(r.conv(m->dec2, D2, 3 * NF, Hp / 2, Wp / 2, T2, NF, 1, 1));
    VFI_DO(r.up2(T2, NF, Hp / 2, Wp / 2, T3, NF, NF));
    VFI_DO(r.conv(m->dec3, T3, NF, Hp, Wp, RO, 8, 1, 0));
    return vfi_xvfi_blend_out(RO, 8, U + cps + 6, ucs, t, out, Hp, Wp, m->H, m->W, st);
}

int round_to(int n, int d) { return n + (d - n % d) % d; }

}  // namespace

extern "C" {

int64_t vfi_xvfi_max_padded_pixels(void) { return max_padded_pixels(kPxFloats); }
int64_t vfi_xvfi_large_max_padded_pixels(void) { return max_padded_pixels_large(kPxFloats); }
int64_t vfi_xvfi_object_max_padded_pixels(const vfi_xvfi_t* m) { return !m ? 0 : (m->large ? max_padded_pixels_large(kPxFloats) : max_padded_pixels(kPxFloats)); }

int vfi_xvfi_set_large_frames(vfi_xvfi_t* m, int on) {
    VFI_REQUIRE(m, "vfi_xvfi_set_large_frames: null object");
    m->large = on != 0;
    return 0;
}

vfi_xvfi_t* vfi_xvfi_create(const float* const* tensors, const int64_t* numels, int n_tensors, int scale, int S_tst) {
    const bool known = (scale == 2 || scale == 4) && S_tst >= 0 && S_tst < kMaxLevels;
    const int want = scale == 4 ? 74 : 72;
    if (!tensors || !numels || !known || n_tensors != want) {
        set_error("vfi_xvfi_create: expected the %d state_dict tensors of XVFInet in xvfi_spec.xvfi_shapes() order for module_scale_factor %d (2 or 4) and "
                  "0 <= S_tst < %d, got %d tensors, S_tst %d", want, scale, kMaxLevels, n_tensors, S_tst);
        return nullptr;
    }
    vfi_xvfi* m = new vfi_xvfi();
    m->scale = scale, m->S = S_tst, m->nds = scale == 4 ? 2 : 1;
    TensorCursor cur(tensors, numels, n_tensors, "vfi_xvfi_create");
    auto layer = [&](int cout, int cin, int k, int stride) { return m->read_layer(cur, 0, cout, cin, k, stride, true, false); };
    // an aliased tensor of the state dict (one module registered twice): its numel is checked, its values are xvfi_spec's to compare
    auto alias = [&](int cout, int cin) {
        cur.take((int64_t)cout * cin * 9);
        cur.take(cout);
    };
    auto tower = [&](Tower& T, int cin, int cout) {
        T.d1 = layer(2 * NF, cin, 4, 2);
        T.d2 = layer(4 * NF, 2 * NF, 4, 2);
        T.u1 = layer(2 * NF, 4 * NF, 3, 1);
        T.u2 = layer(NF, 2 * NF, 3, 1);
        T.o = layer(cout, NF, 3, 1);
    };
    // vfinet.*
    tower(m->bottom, 2 * NF, 6);
    m->flow1 = layer(NF, 2 * NF, 3, 1);
    tower(m->flow2, 2 * NF + 4, 6);
    m->flow3_in = layer(NF, 4 * NF + 4, 1, 1);
    tower(m->flow3, NF, 4);
    alias(NF, NF);      // refine_unet.conv1 / conv2: in the state dict, not in the forward
    alias(NF, NF);
    const int cps = 256 / (scale * scale);
    m->enc1 = layer(NF, cps + 16, 4, 2);
    m->enc2 = layer(2 * NF, NF, 4, 2);
    m->enc3 = layer(4 * NF, 2 * NF, 4, 2);
    m->dec0 = layer(4 * NF, 4 * NF, 3, 1);
    m->dec1 = layer(2 * NF, 6 * NF, 3, 1);
    m->dec2 = layer(NF, 3 * NF, 3, 1);
    m->dec3 = layer(4, NF, 3, 1);
    // channel_converter.0, rec_ext_ds, rec_ext_ds_module.{0.0, 1[, 3]} (aliases), the 3x3 layer, the residual blocks, rec_ctx_ds
    m->cc = layer(NF, 3, 3, 1);
    m->ext_ds = layer(NF, NF, 3, 2);
    const float* w = cur.take((int64_t)NF * 3 * 9);      // rec_ext_ds_module.0.0 = channel_converter.0
    (void)w;
    cur.take(NF);
    for (int i = 0; i < m->nds; ++i) alias(NF, NF);
    m->ext_c = layer(NF, NF, 3, 1);
    for (int i = 0; i < 4; ++i) m->rb[i] = layer(NF, NF, 3, 1);
    m->ctx_ds = layer(NF, NF, 3, 2);
    if (cur.finish() && !m->failed && hipHostMalloc((void**)&m->flag_host, sizeof(int), hipHostMallocDefault) != hipSuccess) {
        set_error("vfi_xvfi_create: pinned host allocation failed");
        m->failed = true;
    }
    if (!cur.finish() || m->failed) {
        vfi_xvfi_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_xvfi_destroy(vfi_xvfi_t* m) {
    if (!m) return;
    if (m->flag_host) (void)hipHostFree(m->flag_host);
    delete m;
}

int vfi_xvfi_release_workspace(vfi_xvfi_t* m) {
    VFI_REQUIRE(m, "vfi_xvfi_release_workspace: null object");
    m->have_pair = false;
    return m->ws.release();
}

int64_t vfi_xvfi_workspace_bytes(const vfi_xvfi_t* m) { return m ? m->ws.bytes() : 0; }

int vfi_xvfi_forward(vfi_xvfi_t* m, const float* frame0_dev, const float* frame1_dev, int C, int H, int W, float t, float* out_dev, void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && out_dev && C >= 3 && H > 0 && W > 0, "vfi_xvfi_forward: bad arguments");
    VFI_REQUIRE(t >= 0.f && t <= 1.f, "vfi_xvfi_forward: timestep %g outside [0, 1]", (double)t);
    const int divide = (1 << m->S) * m->scale * 4;
    const int Hp = round_to(H, divide), Wp = round_to(W, divide);
    hipStream_t st = (hipStream_t)stream;
    const int rc = m->enter("vfi_xvfi_forward", "XVFI", H, W, Hp, Wp, kPxFloats, m->H != H || m->W != W, m->large);
    if (!m->ws.live()) m->have_pair = false;      // released just now, by the caller, or by a failed allocation
    if (rc) return rc;
    m->H = H, m->W = W;
    if (m->have_pair) {
        // the features, level flows and flow_l_tmp are kept while t varies: they are this pair's when both frames equal the padded copy bit
        // for bit (one pass over the frames and one stream synchronisation, against a third of the network)
        Run r{{m, st}};
        float *img = r.buf("img", 2, Hp, Wp, 8), *flag = r.buf("same_flag", 1, 1, 1, 4);
        if (r.bad) return -1;
        VFI_CHECK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
        hipLaunchKernelGGL(xvfi_same_kernel, dim3(nblk((long)H * W, 256), 2), dim3(256), 0, st, frame0_dev, frame1_dev, C, H, W, (const float*)img, Hp, Wp, (int*)flag);
        VFI_CHECK_HIP(hipGetLastError());
        VFI_CHECK_HIP(hipMemcpyAsync(m->flag_host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
        VFI_CHECK_HIP(hipStreamSynchronize(st));
        if (*m->flag_host) m->have_pair = false;
    }
    if (!m->have_pair) {
        if (xvfi_prepare(m, frame0_dev, frame1_dev, C, st)) {
            m->have_pair = false;
            return -1;
        }
        m->have_pair = true;
    }
    if (xvfi_render(m, t, out_dev, st)) {
        m->have_pair = false;
        return -1;
    }
    return 0;
}

int vfi_xvfi_level0_flow(vfi_xvfi_t* m, float* out_dev, void* stream) {
    VFI_REQUIRE(m && out_dev, "vfi_xvfi_level0_flow: bad arguments");
    VFI_REQUIRE(m->have_pair && m->ws.live(), "vfi_xvfi_level0_flow: no forward has run since the workspace was released");
    Run r{{m, (hipStream_t)stream}};
    const int h = m->Hp / m->scale, w = m->Wp / m->scale;
    float* tmp = r.buf("tmp0", 1, h, w, 8);
    if (r.bad) return -1;
    return vfi_axpby(tmp, 8, nullptr, 0, out_dev, 6, (int64_t)h * w, 6, 1.f, 0.f, stream);
}

}  // extern "C"
