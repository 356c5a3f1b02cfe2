// FLAVR (vfi_models/flavr/flavr_arch.py UNet_3D_3D("unet_18", n_inputs=4, n_outputs, joinType="concat", upmode="transpose"),
// resnet_3D.py) as a C-side object: vfi_flavr_create / _forward / _destroy — weights packed once, workspace owned, the ~230 launches of a
// four-frame window issued by one call.  The node's InputPadder(16) and the window mean are inside the call.
//
// Layout.  Every temporal stride of the network is 1, so T stays 4 from the stem to the last up-convolution.  A feature map with C
// channels is kept as [H, W, 6, C]: the four time slices in slices 1..4 between two border slices that are zeroed when the workspace is
// made and never written.  A 3x3x3 convolution with temporal padding 1 is then, for output time t, a 2D 3x3 convolution over the
// CONTIGUOUS channel window of 3 C that starts at slice t — so the 16 encoder convolutions and the two decoder Conv_3d layers are layer
// objects of vfi_conv_create_ex (weights [Cout, Cin, 3, 3, 3] repacked to [Cout, 3 Cin (dt-major), 3, 3]) and run on the library's
// Winograd / direct MFMA kernels, one launch per time slice.  The three ConvTranspose3d((3,4,4), (1,2,2), (1,1,1)) layers are kind-1
// (4x4, stride 2, pad 1) objects over the same window with the temporal taps flipped (window slice j holds input time t - 1 + j, which
// a transposed convolution weighs with tap 2 - j).  The joinTensors concats are channel windows: the decoder writes its half of a
// [H, W, 6, Ca + Cb] buffer, the encoder's output is copied into the other half.
//
// New kernels (below): frame-in (replicate pad to a multiple of 16, deterministic window mean, time-interleaved [Hp, Wp, 4, 4]), the stem
// (Conv3d(3, 64, (3,7,7), (1,2,2), (1,3,3)) + ReLU), the sub-sampling in front of the 1x1x1 downsample convolutions, SEGating (mean over
// (T, H, W), C x C 1x1 with bias, sigmoid) with the scale fused into what follows it — relu(x y + residual) in a BasicBlock,
// lrelu_0.2(x y) written into the concat half in the decoder — and frame-out (ReflectionPad2d(3) + 7x7 convolution to the three channels
// of output 0, + window mean, crop; no clamp).  Every reduction sums fixed slots in a fixed order: no float atomics.
//
// Windows of a call run one after another through the same launches as a call with one window, so a window's result does not depend on
// its batch mates; the workspace is sized for one window.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/vfi_hip.h"
#include "net_object.h"
#include "vfi_common.h"

using namespace vfi;

namespace {

constexpr int T = 4;                     // frames of a window = time slices of every feature map
constexpr int TS = T + 2;                // slices of a bordered feature map
constexpr int SUM_SLOTS = 256;           // frame-in: workgroups of the mean's first pass
constexpr int GATE_SLOTS = 1024;         // SEGating: at most this many workgroups in the mean's first pass

unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

// ---- frame-in ----------------------------------------------------------------------------------------------------------------------
struct Frames4 {
    const float* f[T];
};

// slots[b][c] = sum over workgroup b's padded pixels (all four frames) of channel c; pixel i of the 4 Hp Wp belongs to thread i % (256 G)
__global__ __launch_bounds__(256) void flavr_sum_kernel(Frames4 fr, int C, int H, int W, int Hp, int Wp, int pt, int pl, float* __restrict__ slots) {
    __shared__ float red[256][3];
    const long n = (long)T * Hp * Wp;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int f = (int)(i / ((long)Hp * Wp));
        const long p = i - (long)f * Hp * Wp;
        const int y = (int)(p / Wp), x = (int)(p - (long)y * Wp);
        const int sy = min(max(y - pt, 0), H - 1), sx = min(max(x - pl, 0), W - 1);
        const float* q = fr.f[f] + ((long)sy * W + sx) * C;
        s0 += q[0], s1 += q[1], s2 += q[2];
    }
    red[threadIdx.x][0] = s0, red[threadIdx.x][1] = s1, red[threadIdx.x][2] = s2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int c = 0; c < 3; ++c) red[threadIdx.x][c] += red[threadIdx.x + h][c];
        __syncthreads();
    }
    if (threadIdx.x < 3) slots[blockIdx.x * 4 + threadIdx.x] = red[0][threadIdx.x];
}

__global__ void flavr_mean_kernel(const float* __restrict__ slots, int G, double count, float* __restrict__ mean) {
    if (threadIdx.x >= 4) return;
    double s = 0.0;
    if (threadIdx.x < 3)
        for (int g = 0; g < G; ++g) s += (double)slots[g * 4 + threadIdx.x];
    mean[threadIdx.x] = (float)(s / count);
}

// out[y, x, t, 0..3] = (frame_t[clamped y - pt, x - pl, 0..2] - mean, 0)
__global__ __launch_bounds__(256) void flavr_center_kernel(Frames4 fr, int C, int H, int W, int Hp, int Wp, int pt, int pl, const float* __restrict__ mean,
                                                           float4* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Hp * Wp * T) return;
    const int t = (int)(i & 3);
    const long p = i >> 2;
    const int y = (int)(p / Wp), x = (int)(p - (long)y * Wp);
    const int sy = min(max(y - pt, 0), H - 1), sx = min(max(x - pl, 0), W - 1);
    const float* q = fr.f[t] + ((long)sy * W + sx) * C;
    out[i] = make_float4(q[0] - mean[0], q[1] - mean[1], q[2] - mean[2], 0.f);
}

int frame_in_launch(const float* const* frames, int C, int H, int W, int Hp, int Wp, float* out, float* mean, float* slots, hipStream_t st) {
    Frames4 fr;
    for (int t = 0; t < T; ++t) fr.f[t] = frames[t];
    const int pt = (Hp - H) / 2, pl = (Wp - W) / 2;
    TraceScope ts("flavr_frame_in", st);
    flavr_sum_kernel<<<SUM_SLOTS, 256, 0, st>>>(fr, C, H, W, Hp, Wp, pt, pl, slots);
    flavr_mean_kernel<<<1, 64, 0, st>>>(slots, SUM_SLOTS, (double)T * Hp * Wp, mean);
    flavr_center_kernel<<<blocks((long)Hp * Wp * T), 256, 0, st>>>(fr, C, H, W, Hp, Wp, pt, pl, mean, (float4*)out);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- stem --------------------------------------------------------------------------------------------------------------------------
// Conv3d(3, 64, (3,7,7), stride (1,2,2), padding (1,3,3)) + ReLU on x [Hp, Wp, 4, 4].  A workgroup owns 16 x 16 output pixels of one time
// slice and 16 of the 64 output channels (a thread: one pixel, 16 accumulators); the 37 x 37 input patch of each of the (up to) three
// temporal taps goes through LDS as float4 (r, g, b, 0).  Weights are repacked to [chunk][dt][ky][kx][ci][16]: the 48 weights of a tap
// position are contiguous and their address is wave-uniform, so they arrive through the scalar cache and feed the FMAs as scalar operands.
constexpr int ST_TILE = 16, ST_PATCH = 2 * ST_TILE + 5, ST_WFLOATS = 64 * 3 * 3 * 49;

__global__ void flavr_stem_pack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;      // packed index
    if (i >= ST_WFLOATS) return;
    const int k = i % 16, ci = (i / 16) % 3, pos = (i / 48) % 49, dt = (i / (48 * 49)) % 3, chunk = i / (48 * 49 * 3);
    wp[i] = w[(((chunk * 16 + k) * 3 + ci) * 3 + dt) * 49 + pos];
}

__global__ __launch_bounds__(256) void flavr_stem_kernel(const float4* __restrict__ x, int Hp, int Wp, int Ho, int Wo, const float* __restrict__ wp,
                                                         const float* __restrict__ bias, float* __restrict__ out, long out_cs) {
    __shared__ float4 patch[ST_PATCH * ST_PATCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int t = blockIdx.z >> 2, chunk = blockIdx.z & 3;
    const int ox0 = blockIdx.x * ST_TILE, oy0 = blockIdx.y * ST_TILE;
    float acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = bias ? bias[chunk * 16 + k] : 0.f;
    for (int dt = 0; dt < 3; ++dt) {
        const int tsrc = t + dt - 1;
        if (tsrc < 0 || tsrc >= T) continue;      // temporal zero padding (uniform)
        __syncthreads();
        for (int i = tid; i < ST_PATCH * ST_PATCH; i += 256) {
            const int r = i / ST_PATCH, c = i - r * ST_PATCH;
            const int gy = 2 * oy0 - 3 + r, gx = 2 * ox0 - 3 + c;
            patch[i] = (gy >= 0 && gy < Hp && gx >= 0 && gx < Wp) ? x[((long)gy * Wp + gx) * T + tsrc] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        const float* __restrict__ w = wp + (size_t)((chunk * 3 + dt) * 49) * 48;
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float4 v = patch[(2 * ty + ky) * ST_PATCH + 2 * tx + kx];
                const float* __restrict__ w48 = w + (ky * 7 + kx) * 48;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    acc[k] = fmaf(v.x, w48[k], acc[k]);
                    acc[k] = fmaf(v.y, w48[16 + k], acc[k]);
                    acc[k] = fmaf(v.z, w48[32 + k], acc[k]);
                }
            }
        }
    }
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;
    float4* o = (float4*)(out + ((long)oy * Wo + ox) * out_cs + t * 64 + chunk * 16);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = make_float4(fmaxf(acc[4 * k], 0.f), fmaxf(acc[4 * k + 1], 0.f), fmaxf(acc[4 * k + 2], 0.f), fmaxf(acc[4 * k + 3], 0.f));
}

int stem_launch(const float* x, int Hp, int Wp, const float* wp, const float* bias, float* out, long out_cs, hipStream_t st) {
    const int Ho = (Hp + 1) / 2, Wo = (Wp + 1) / 2;
    TraceScope ts("flavr_stem", st);
    flavr_stem_kernel<<<dim3(cdiv(Wo, ST_TILE), cdiv(Ho, ST_TILE), T * 4), 256, 0, st>>>((const float4*)x, Hp, Wp, Ho, Wo, wp, bias, out, out_cs);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- slice movement ----------------------------------------------------------------------------------------------------------------
// dst[(y, x), t, c] = src[(sy * y, sx * x), t, c] for the four time slices; element (p, t, c) of a tensor sits at base + p * ps + t * ss + c
// (ps = pixel stride, ss = slice stride, floats; C % 4 == 0).  step 1 = the copy of an encoder output into its concat half, step 2 = the
// spatial sub-sampling in front of a Conv3d(k=1, stride (1,2,2)).
__global__ __launch_bounds__(256) void flavr_slices_kernel(const float* __restrict__ src, long s_ps, long s_ss, int Ws, int step, float* __restrict__ dst,
                                                           long d_ps, long d_ss, int h, int w, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)h * w * T * C4) return;
    const int q = (int)(i % C4);
    const long pt = i / C4;
    const int t = (int)(pt & 3);
    const long p = pt >> 2;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    *(float4*)(dst + p * d_ps + t * d_ss + 4 * q) = *(const float4*)(src + ((long)y * step * Ws + (long)x * step) * s_ps + t * s_ss + 4 * q);
}

int slices_launch(const float* src, long s_ps, long s_ss, int Ws, int step, float* dst, long d_ps, long d_ss, int h, int w, int C, hipStream_t st) {
    TraceScope ts(step == 1 ? "flavr_copy_slices" : "flavr_subsample", st);
    flavr_slices_kernel<<<blocks((long)h * w * T * (C / 4)), 256, 0, st>>>(src, s_ps, s_ss, Ws, step, dst, d_ps, d_ss, h, w, C / 4);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- SEGating ----------------------------------------------------------------------------------------------------------------------
// pass 1: slots[b][c] = sum over workgroup b's pixel range and the four slices of x[., ., c]; a thread owns a channel quad and every
// rows-th pixel of the range, the rows are then summed in order by row 0
__global__ __launch_bounds__(256) void flavr_gate_sum_kernel(const float* __restrict__ x, long ps, long ss, long P, long chunk, int C4, float* __restrict__ slots) {
    __shared__ float4 red[256];
    const int rows = 256 / C4, tid = threadIdx.x;
    const int r = tid / C4, q = tid - r * C4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) {
        const long p1 = min(P, (long)(blockIdx.x + 1) * chunk);
        for (long p = (long)blockIdx.x * chunk + r; p < p1; p += rows) {
            const float* b = x + p * ps + 4 * q;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const float4 v = *(const float4*)(b + t * ss);
                s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
            }
        }
    }
    red[tid] = s;
    __syncthreads();
    if (r == 0) {
        for (int k = 1; k < rows; ++k) {
            const float4 v = red[k * C4 + q];
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        *(float4*)(slots + (long)blockIdx.x * 4 * C4 + 4 * q) = s;
    }
}

// pass 2: mean[c] = (sum_b slots[b][c]) / count (in double, slot order), y[co] = sigmoid(b[co] + sum_ci w[co][ci] mean[ci]): a wave per output
// channel, lanes over ci, butterfly sum (the same order on every run)
__global__ __launch_bounds__(256) void flavr_gate_fc_kernel(const float* __restrict__ slots, int G, double count, int C, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ y) {
    __shared__ float mean[1024];
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)slots[(long)g * C + c];
        mean[c] = (float)(s / count);
    }
    __syncthreads();
    const int co = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (co >= C) return;
    float d = 0.f;
    for (int ci = lane; ci < C; ci += 64) d = fmaf(w[(long)co * C + ci], mean[ci], d);
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    if (lane == 0) y[co] = 1.f / (1.f + expf(-(d + b[co])));
}

// pass 3: out = relu(x y + res) (MODE 0, BasicBlock) or lrelu_0.2(x y) (MODE 1, decoder); out may alias x
template <int MODE>
__global__ __launch_bounds__(256) void flavr_gate_apply_kernel(const float* x, long x_ps, long x_ss, const float* res, long r_ps, long r_ss,
                                                               const float* __restrict__ y, float* out, long o_ps, long o_ss, long P, int C4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * T * C4) return;
    const int q = (int)(i % C4);
    const long pt = i / C4;
    const int t = (int)(pt & 3);
    const long p = pt >> 2;
    const float4 v = *(const float4*)(x + p * x_ps + t * x_ss + 4 * q);
    const float4 g = *(const float4*)(y + 4 * q);
    float4 o;
    if (MODE == 0) {
        const float4 rr = *(const float4*)(res + p * r_ps + t * r_ss + 4 * q);
        o = make_float4(fmaxf(fmaf(v.x, g.x, rr.x), 0.f), fmaxf(fmaf(v.y, g.y, rr.y), 0.f), fmaxf(fmaf(v.z, g.z, rr.z), 0.f), fmaxf(fmaf(v.w, g.w, rr.w), 0.f));
    } else {
        auto lr = [](float a) { return a > 0.f ? a : 0.2f * a; };
        o = make_float4(lr(v.x * g.x), lr(v.y * g.y), lr(v.z * g.z), lr(v.w * g.w));
    }
    *(float4*)(out + p * o_ps + t * o_ss + 4 * q) = o;
}

int gate_slots(long P) { return (int)std::min<long>(GATE_SLOTS, std::max<long>(1, (P + 63) / 64)); }

int gate_launch(const float* x, long x_ps, long x_ss, const float* res, long r_ps, long r_ss, float* out, long o_ps, long o_ss, long P, int C,
                const float* w, const float* b, int mode, float* ws, hipStream_t st) {
    const int G = gate_slots(P), C4 = C / 4;
    const long chunk = (P + G - 1) / G;
    float* slots = ws;
    float* y = ws + (size_t)GATE_SLOTS * C;
    TraceScope ts(mode ? "flavr_gate_lrelu" : "flavr_gate_res_relu", st);
    flavr_gate_sum_kernel<<<G, 256, 0, st>>>(x, x_ps, x_ss, P, chunk, C4, slots);
    flavr_gate_fc_kernel<<<cdiv(C, 4), 256, 0, st>>>(slots, G, (double)P * T, C, w, b, y);
    if (mode == 0)
        flavr_gate_apply_kernel<0><<<blocks(P * T * C4), 256, 0, st>>>(x, x_ps, x_ss, res, r_ps, r_ss, y, out, o_ps, o_ss, P, C4);
    else
        flavr_gate_apply_kernel<1><<<blocks(P * T * C4), 256, 0, st>>>(x, x_ps, x_ss, nullptr, 0, 0, y, out, o_ps, o_ss, P, C4);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- frame-out ---------------------------------------------------------------------------------------------------------------------
// out[y, x, c] = b[c] + mean[c] + sum_{ky, kx, ci} feat[reflect(y + pt + ky - 3), reflect(x + pl + kx - 3), ci] w[c][ci][ky][kx], c = 0..2, for the
// H x W crop at (pt, pl) of feat [Hp, Wp, 64].  A workgroup owns 16 x 16 output pixels; the 22 x 22 patch goes through LDS 16 channels at
// a time as four planes of float4 (neighbouring pixels in neighbouring LDS words); weights repacked to [ky][kx][ci][4] arrive as scalars.
constexpr int FO_TILE = 16, FO_PATCH = FO_TILE + 6, FO_WFLOATS = 49 * 64 * 4;

__global__ void flavr_out_pack_kernel(const float* __restrict__ w, float* __restrict__ wp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= FO_WFLOATS) return;
    const int c = i & 3, ci = (i >> 2) & 63, pos = i >> 8;
    wp[i] = c < 3 ? w[(c * 64 + ci) * 49 + pos] : 0.f;
}

__global__ __launch_bounds__(256) void flavr_out_kernel(const float4* __restrict__ feat, int Hp, int Wp, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, const float* __restrict__ mean, int pt, int pl, int H, int W,
                                                        float* __restrict__ out) {
    __shared__ float4 patch[4][FO_PATCH * FO_PATCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = blockIdx.x * FO_TILE, y0 = blockIdx.y * FO_TILE;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int chunk = 0; chunk < 4; ++chunk) {
        __syncthreads();
        for (int i = tid; i < 4 * FO_PATCH * FO_PATCH; i += 256) {
            const int q = i & 3, pix = i >> 2;
            const int r = pix / FO_PATCH, c = pix - r * FO_PATCH;
            const int gy = pad_index(y0 + pt - 3 + r, Hp, 2), gx = pad_index(x0 + pl - 3 + c, Wp, 2);
            patch[q][pix] = feat[((long)gy * Wp + gx) * 16 + chunk * 4 + q];
        }
        __syncthreads();
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float* __restrict__ w = wp + ((ky * 7 + kx) * 64 + chunk * 16) * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 v = patch[q][(ty + ky) * FO_PATCH + tx + kx];
                    const float* __restrict__ wq = w + q * 16;
                    a0 = fmaf(v.x, wq[0], a0), a1 = fmaf(v.x, wq[1], a1), a2 = fmaf(v.x, wq[2], a2);
                    a0 = fmaf(v.y, wq[4], a0), a1 = fmaf(v.y, wq[5], a1), a2 = fmaf(v.y, wq[6], a2);
                    a0 = fmaf(v.z, wq[8], a0), a1 = fmaf(v.z, wq[9], a1), a2 = fmaf(v.z, wq[10], a2);
                    a0 = fmaf(v.w, wq[12], a0), a1 = fmaf(v.w, wq[13], a1), a2 = fmaf(v.w, wq[14], a2);
                }
            }
        }
    }
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    float* o = out + ((long)y * W + x) * 3;
    o[0] = a0 + bias[0] + mean[0];
    o[1] = a1 + bias[1] + mean[1];
    o[2] = a2 + bias[2] + mean[2];
}

int out_launch(const float* feat, int Hp, int Wp, const float* wp, const float* bias, const float* mean, int pt, int pl, int H, int W, float* out,
               hipStream_t st) {
    TraceScope ts("flavr_frame_out", st);
    flavr_out_kernel<<<dim3(cdiv(W, FO_TILE), cdiv(H, FO_TILE)), 256, 0, st>>>((const float4*)feat, Hp, Wp, wp, bias, mean, pt, pl, H, W, out);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int pad16(int n) { return (n + 15) / 16 * 16; }

struct Gate {
    float *w = nullptr, *b = nullptr;      // device [C][C], [C]
};

struct Block {
    vfi_conv_t *c1 = nullptr, *c2 = nullptr, *ds = nullptr;
    Gate g;
    int cin = 0, c = 0, stride = 1;
};

}  // namespace

struct vfi_flavr : NetObject {
    int n_outputs = 1;
    float *stem_wp = nullptr, *stem_b = nullptr;       // packed stem weights, bias (null for n_outputs == 1)
    Block blk[8];                                      // layer1.0, layer1.1, ..., layer4.1
    vfi_conv_t* dec[5] = {};                           // Conv_3d, upConv3D, upConv3D, Conv_3d, upConv3D
    Gate dg[5];
    vfi_conv_t* fuse = nullptr;
    float *out_wp = nullptr, *out_b = nullptr;
    // workspace for one window at Hp x Wp
    int Hp = 0, Wp = 0;
    float *x = nullptr, *mean = nullptr, *scratch = nullptr;      // scratch: frame-in slots | gate slots + y
    float* e2[3] = {};                                 // [P/4, 6, 64]
    float* e4[3] = {};                                 // [P/16, 6, 128]
    float* e8[3] = {};                                 // [P/64, 6, 256]
    float* f8[3] = {};                                 // [P/64, 6, 512]
    float* cat[4] = {};                                // (dx_0 | x_0) [P/4, 6, 128], (dx_1 | x_1) [P/4, 6, 128], (dx_2 | x_2) [P/16, 6, 256], (dx_3 | x_3) [P/64, 6, 512]
    float *sub = nullptr, *dsout = nullptr;            // sub-sampled input / output of a downsample convolution, [pixels, 4, C]
    float *fin = nullptr, *fused = nullptr;            // last up-convolution [P, 4 * 64], feature_fuse [P, 64]
    bool large = false;                                // vfi_flavr_set_large_frames: padded frames up to kLargeMaxPixels are served
};

namespace {

int ensure_workspace(vfi_flavr* m, int Hp, int Wp, hipStream_t st) {
    if (m->ws.live() && m->Hp == Hp && m->Wp == Wp) return 0;
    if (m->ws.release()) return -1;
    // bordered buffers are zeroed once: their border slices are never written afterwards
    auto get = [&](float** p, size_t floats, bool zero) { return m->ws.alloc(p, floats, zero ? Workspace::kZero : Workspace::kNoFill, st); };
    const size_t P = (size_t)Hp * Wp, P2 = P / 4, P4 = P / 16, P8 = P / 64;
    bool bad = get(&m->x, P * T * 4, false) || get(&m->mean, 4, false) || get(&m->scratch, (size_t)GATE_SLOTS * 512 + 1024, false) ||
               get(&m->sub, std::max(P4 * T * 64, P8 * T * 256), false) || get(&m->dsout, std::max(P4 * T * 128, P8 * T * 512), false) ||
               get(&m->fin, P * T * 64, false) || get(&m->fused, P * 64, false);
    for (int i = 0; i < 3 && !bad; ++i)
        bad = get(&m->e2[i], P2 * TS * 64, true) || get(&m->e4[i], P4 * TS * 128, true) || get(&m->e8[i], P8 * TS * 256, true) ||
              get(&m->f8[i], P8 * TS * 512, true);
    bad = bad || get(&m->cat[0], P2 * TS * 128, true) || get(&m->cat[1], P2 * TS * 128, true) || get(&m->cat[2], P4 * TS * 256, true) ||
          get(&m->cat[3], P8 * TS * 512, true);
    if (bad) return -1;
    m->Hp = Hp, m->Wp = Wp;
    return 0;
}

// a 3x3x3 layer (stride 1 or (1,2,2)) or a transposed (3,4,4) layer: one launch per time slice.  in / out are bordered buffers
// [., ., 6, cin] / [., ., 6, out_c] (out_off = channel offset inside a slice, for concat halves); `flat` = the un-bordered [., ., 4 * cout] output
int conv_t(const vfi_conv_t* L, const float* in, int cin, int h, int w, float* out, int out_c, bool flat, int act, float slope, hipStream_t st) {
    for (int t = 0; t < T; ++t)
        if (vfi_conv_forward_ex(L, in + (size_t)t * cin, TS * cin, h, w, out + (size_t)(flat ? t : t + 1) * out_c, (flat ? T : TS) * out_c, 1, act, slope, 0.f,
                                0.f, nullptr, 0, st))
            return -1;
    return 0;
}

int forward_window(vfi_flavr* m, const float* const* frames, int C, int H, int W, float* out, hipStream_t st) {
    const int Hp = m->Hp, Wp = m->Wp;
    const int h2 = Hp / 2, w2 = Wp / 2, h4 = Hp / 4, w4 = Wp / 4, h8 = Hp / 8, w8 = Wp / 8;
    const long P = (long)Hp * Wp, P2 = P / 4, P4 = P / 16, P8 = P / 64;
    float* ws = m->scratch;
    if (frame_in_launch(frames, C, H, W, Hp, Wp, m->x, m->mean, ws, st)) return -1;
    // x_0 = stem, kept in e2[0] and copied into (dx_0 | x_0)
    if (stem_launch(m->x, Hp, Wp, m->stem_wp, m->stem_b, m->e2[0] + 64, TS * 64, st)) return -1;
    if (slices_launch(m->e2[0] + 64, TS * 64, 64, w2, 1, m->cat[0] + 128 + 64, TS * 128, 128, h2, w2, 64, st)) return -1;
    // encoder: per level three bordered buffers b[0..2]; a block reads b[cur] and leaves its result in another one
    struct Level {
        float** b;
        int h, w;
        long P;
    } lv[4] = {{m->e2, h2, w2, P2}, {m->e4, h4, w4, P4}, {m->e8, h8, w8, P8}, {m->f8, h8, w8, P8}};
    const float* xin = m->e2[0];      // bordered input of the next block
    int cur = 0;                      // index of xin inside its level's buffers (level of the block's OUTPUT when the block keeps the size)
    for (int i = 0; i < 8; ++i) {
        const Block& B = m->blk[i];
        const Level& L = lv[i / 2];
        const bool first = i % 2 == 0, new_level = first && i > 0;
        const int hin = new_level ? lv[i / 2 - 1].h : L.h, win = new_level ? lv[i / 2 - 1].w : L.w;
        // buffers of this block: a = conv1's output, o = conv2's output and the block's result (gated in place)
        int ia, io;
        if (new_level) ia = 1, io = 2;
        else ia = (cur + 1) % 3, io = (cur + 2) % 3;
        float *a = L.b[ia], *o = L.b[io];
        if (conv_t(B.c1, xin, B.cin, hin, win, a, B.c, false, 1, 0.f, st)) return -1;
        if (conv_t(B.c2, a, B.c, L.h, L.w, o, B.c, false, 0, 0.f, st)) return -1;
        const float* res = xin + B.cin;
        long r_ps = (long)TS * B.cin, r_ss = B.cin;
        if (B.ds) {
            if (slices_launch(xin + B.cin, (long)TS * B.cin, B.cin, win, B.stride, m->sub, (long)T * B.cin, B.cin, L.h, L.w, B.cin, st)) return -1;
            if (vfi_conv_forward_ex(B.ds, m->sub, B.cin, L.h, L.w * T, m->dsout, B.c, 1, 0, 0.f, 0.f, 0.f, nullptr, 0, st)) return -1;
            res = m->dsout, r_ps = (long)T * B.c, r_ss = B.c;
        }
        if (gate_launch(o + B.c, (long)TS * B.c, B.c, res, r_ps, r_ss, o + B.c, (long)TS * B.c, B.c, L.P, B.c, B.g.w, B.g.b, 0, ws, st)) return -1;
        xin = o, cur = io;
        if (!first && i < 6) {      // x_1, x_2, x_3 into the second half of their concat buffers
            const int cc = 2 * B.c;
            if (slices_launch(o + B.c, (long)TS * B.c, B.c, L.w, 1, m->cat[i / 2 + 1] + cc + B.c, (long)TS * cc, cc, L.h, L.w, B.c, st)) return -1;
        }
    }
    const float* x4 = xin;
    // decoder: each layer's raw output in a free encoder buffer, gated + lrelu into the first half of the next concat buffer
    if (conv_t(m->dec[0], x4, 512, h8, w8, m->e8[1], 256, false, 0, 0.f, st) ||
        gate_launch(m->e8[1] + 256, TS * 256, 256, nullptr, 0, 0, m->cat[3] + 512, TS * 512, 512, P8, 256, m->dg[0].w, m->dg[0].b, 1, ws, st))
        return -1;
    if (conv_t(m->dec[1], m->cat[3], 512, h8, w8, m->e4[1], 128, false, 0, 0.f, st) ||
        gate_launch(m->e4[1] + 128, TS * 128, 128, nullptr, 0, 0, m->cat[2] + 256, TS * 256, 256, P4, 128, m->dg[1].w, m->dg[1].b, 1, ws, st))
        return -1;
    if (conv_t(m->dec[2], m->cat[2], 256, h4, w4, m->e2[1], 64, false, 0, 0.f, st) ||
        gate_launch(m->e2[1] + 64, TS * 64, 64, nullptr, 0, 0, m->cat[1] + 128, TS * 128, 128, P2, 64, m->dg[2].w, m->dg[2].b, 1, ws, st))
        return -1;
    if (conv_t(m->dec[3], m->cat[1], 128, h2, w2, m->e2[1], 64, false, 0, 0.f, st) ||
        gate_launch(m->e2[1] + 64, TS * 64, 64, nullptr, 0, 0, m->cat[0] + 128, TS * 128, 128, P2, 64, m->dg[3].w, m->dg[3].b, 1, ws, st))
        return -1;
    if (conv_t(m->dec[4], m->cat[0], 128, h2, w2, m->fin, 64, true, 0, 0.f, st) ||
        gate_launch(m->fin, T * 64, 64, nullptr, 0, 0, m->fin, T * 64, 64, P, 64, m->dg[4].w, m->dg[4].b, 1, ws, st))
        return -1;
    // cat(unbind(dx_out, 2), 1) is fin's T * 64 contiguous channels
    if (vfi_conv_forward_ex(m->fuse, m->fin, T * 64, Hp, Wp, m->fused, 64, 1, 1, 0.2f, 0.f, 0.f, nullptr, 0, st)) return -1;
    return out_launch(m->fused, Hp, Wp, m->out_wp, m->out_b, m->mean, (Hp - H) / 2, (Wp - W) / 2, H, W, out, st);
}

// the largest padded frame: the last up-convolution's [Hp, Wp, 4 * 64] output must stay below the convolution kernels' 2^31-byte image limit
// (every other tensor is smaller: the widest bordered one, [Hp/2, Wp/2, 6 * 128], is 3/4 of it)
bool size_ok(int Hp, int Wp) { return (long)Hp * Wp * T * 64 * 4 < 0x7fffffffL; }
constexpr long kMaxPixels = (0x7fffffffL / 4 - 1) / (T * 64);      // 2 097 151: what size_ok admits
// ... with vfi_flavr_set_large_frames: the same tensor, the widest operand image of any layer, must fit the layer kernels' bound for one
// operand with the permission (conv_large.h: kConvHugeMaxFloats floats); the layers that meet an image of 2 GiB or more all have a
// large form (docs/design/flavr.md "4K")
constexpr long kLargeMaxPixels = kConvHugeMaxFloats / (T * 64);      // 8 388 607
static_assert(kMaxPixels == 2097151 && kLargeMaxPixels == 8388607, "FLAVR's frame limits");
bool size_ok_large(int Hp, int Wp) { return (long)Hp * Wp <= kLargeMaxPixels; }

}  // namespace

extern "C" {

int vfi_flavr_frame_in(const float* const* frames_dev, int C, int H, int W, float* out_dev, float* mean_dev, float* workspace_dev, int64_t workspace_bytes,
                       void* stream) {
    VFI_REQUIRE(frames_dev && out_dev && mean_dev && workspace_dev && C >= 3 && H > 0 && W > 0, "vfi_flavr_frame_in: bad arguments (C=%d H=%d W=%d)", C, H, W);
    VFI_REQUIRE(workspace_bytes >= (int64_t)SUM_SLOTS * 4 * 4, "vfi_flavr_frame_in: workspace of %lld bytes, needs %d", (long long)workspace_bytes,
                SUM_SLOTS * 16);
    for (int t = 0; t < T; ++t) VFI_REQUIRE(frames_dev[t], "vfi_flavr_frame_in: null frame pointer %d", t);
    return frame_in_launch(frames_dev, C, H, W, pad16(H), pad16(W), out_dev, mean_dev, workspace_dev, (hipStream_t)stream);
}

int vfi_flavr_stem(const float* x_dev, int Hp, int Wp, const float* w_dev, const float* bias_dev, float* out_dev, int out_cs, float* workspace_dev,
                   int64_t workspace_bytes, void* stream) {
    VFI_REQUIRE(x_dev && w_dev && out_dev && workspace_dev && Hp > 0 && Wp > 0 && out_cs >= T * 64 && out_cs % 4 == 0 && ((uintptr_t)out_dev & 15) == 0,
                "vfi_flavr_stem: bad arguments (Hp=%d Wp=%d out_cs=%d)", Hp, Wp, out_cs);
    VFI_REQUIRE(workspace_bytes >= (int64_t)ST_WFLOATS * 4, "vfi_flavr_stem: workspace of %lld bytes, needs %d", (long long)workspace_bytes, ST_WFLOATS * 4);
    flavr_stem_pack_kernel<<<blocks(ST_WFLOATS), 256, 0, (hipStream_t)stream>>>(w_dev, workspace_dev);
    return stem_launch(x_dev, Hp, Wp, workspace_dev, bias_dev, out_dev, out_cs, (hipStream_t)stream);
}

int vfi_flavr_down1x1(const vfi_conv_t* conv1x1, int Cin, int Cout, const float* in_dev, int64_t in_ps, int64_t in_ss, int Hin, int Win, int stride,
                      float* sub_dev, float* out_dev, void* stream) {
    VFI_REQUIRE(conv1x1 && in_dev && sub_dev && out_dev && Cin > 0 && Cin % 8 == 0 && Cout > 0 && Hin > 0 && Win > 0 && (stride == 1 || stride == 2) &&
                    in_ps % 4 == 0 && in_ss % 4 == 0 && ((uintptr_t)in_dev & 15) == 0,
                "vfi_flavr_down1x1: bad arguments (Cin=%d Cout=%d Hin=%d Win=%d stride=%d)", Cin, Cout, Hin, Win, stride);
    const int h = (Hin + stride - 1) / stride, w = (Win + stride - 1) / stride;
    if (slices_launch(in_dev, in_ps, in_ss, Win, stride, sub_dev, (long)T * Cin, Cin, h, w, Cin, (hipStream_t)stream)) return -1;
    return vfi_conv_forward_ex(conv1x1, sub_dev, Cin, h, w * T, out_dev, Cout, 1, 0, 0.f, 0.f, 0.f, nullptr, 0, stream);
}

int vfi_flavr_gate(const float* x_dev, int64_t x_ps, int64_t x_ss, const float* res_dev, int64_t res_ps, int64_t res_ss, float* out_dev, int64_t out_ps,
                   int64_t out_ss, int64_t pixels, int C, const float* w_dev, const float* b_dev, int mode, float* workspace_dev, int64_t workspace_bytes,
                   void* stream) {
    VFI_REQUIRE(x_dev && out_dev && w_dev && b_dev && workspace_dev && pixels > 0 && C >= 4 && C % 4 == 0 && C <= 1024 && (mode == 0 || mode == 1) &&
                    (mode == 1 || res_dev),
                "vfi_flavr_gate: bad arguments (pixels=%lld C=%d mode=%d; C a multiple of 4 up to 1024)", (long long)pixels, C, mode);
    VFI_REQUIRE((x_ps | x_ss | res_ps | res_ss | out_ps | out_ss) % 4 == 0 && (((uintptr_t)x_dev | (uintptr_t)res_dev | (uintptr_t)out_dev) & 15) == 0,
                "vfi_flavr_gate: strides must be multiples of 4 floats and pointers 16-byte aligned");
    VFI_REQUIRE(workspace_bytes >= ((int64_t)GATE_SLOTS * C + C) * 4, "vfi_flavr_gate: workspace of %lld bytes, needs %lld", (long long)workspace_bytes,
                ((long long)GATE_SLOTS * C + C) * 4);
    return gate_launch(x_dev, x_ps, x_ss, res_dev, res_ps, res_ss, out_dev, out_ps, out_ss, pixels, C, w_dev, b_dev, mode, workspace_dev, (hipStream_t)stream);
}

int vfi_flavr_frame_out(const float* feat_dev, int Hp, int Wp, const float* w_dev, const float* bias_dev, const float* mean_dev, int pad_top, int pad_left,
                        int H, int W, float* out_dev, float* workspace_dev, int64_t workspace_bytes, void* stream) {
    VFI_REQUIRE(feat_dev && w_dev && bias_dev && mean_dev && out_dev && workspace_dev && Hp >= 4 && Wp >= 4 && H > 0 && W > 0 && pad_top >= 0 && pad_left >= 0 &&
                    pad_top + H <= Hp && pad_left + W <= Wp && ((uintptr_t)feat_dev & 15) == 0,
                "vfi_flavr_frame_out: bad arguments (Hp=%d Wp=%d H=%d W=%d pad=%d,%d; reflection by 3 needs at least 4 pixels)", Hp, Wp, H, W, pad_top,
                pad_left);
    VFI_REQUIRE(workspace_bytes >= (int64_t)FO_WFLOATS * 4, "vfi_flavr_frame_out: workspace of %lld bytes, needs %d", (long long)workspace_bytes, FO_WFLOATS * 4);
    flavr_out_pack_kernel<<<blocks(FO_WFLOATS), 256, 0, (hipStream_t)stream>>>(w_dev, workspace_dev);
    return out_launch(feat_dev, Hp, Wp, workspace_dev, bias_dev, mean_dev, pad_top, pad_left, H, W, out_dev, (hipStream_t)stream);
}

vfi_flavr_t* vfi_flavr_create(const float* const* tensors, const int64_t* numels, int n_tensors, int n_outputs) {
    const bool eb = n_outputs > 1;
    const int want = eb ? 76 : 59;
    if (!tensors || !numels || n_outputs < 1 || n_tensors != want) {
        set_error("vfi_flavr_create: expected the %d state_dict tensors of FLAVR (n_outputs=%d) in flavr_spec.flavr_shapes() order, got %d", want, n_outputs,
                  n_tensors);
        return nullptr;
    }
    vfi_flavr* m = new vfi_flavr();
    m->n_outputs = n_outputs;
    TensorCursor cur(tensors, numels, n_tensors, "vfi_flavr_create");
    std::vector<float> w2;
    // Conv3d [cout, cin, 3, 3, 3] -> [cout, 3 cin (dt-major), 3, 3]
    auto conv3 = [&](vfi_conv_t** L, int cout, int cin, int stride, bool bias) {
        const float* w = cur.take((int64_t)cout * cin * 27);
        const float* b = bias ? cur.take(cout) : nullptr;
        if (!cur.ok()) return;
        w2.resize((size_t)cout * cin * 27);
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int dt = 0; dt < 3; ++dt)
                    memcpy(&w2[(((size_t)co * 3 + dt) * cin + ci) * 9], &w[(((size_t)co * cin + ci) * 3 + dt) * 9], 9 * sizeof(float));
        *L = m->add_layer(vfi_conv_create_ex(0, w2.data(), b, cout, 3 * cin, 3, stride, 0, nullptr, 3 * cin, nullptr));
    };
    // ConvTranspose3d [cin, cout, 3, 4, 4] -> ConvTranspose2d [3 cin, cout, 4, 4], window slice j = temporal tap 2 - j
    auto deconv = [&](vfi_conv_t** L, int cin, int cout) {
        const float* w = cur.take((int64_t)cin * cout * 48);
        const float* b = cur.take(cout);
        if (!cur.ok()) return;
        w2.resize((size_t)cin * cout * 48);
        for (int j = 0; j < 3; ++j)
            for (int ci = 0; ci < cin; ++ci)
                for (int co = 0; co < cout; ++co)
                    memcpy(&w2[(((size_t)j * cin + ci) * cout + co) * 16], &w[(((size_t)ci * cout + co) * 3 + (2 - j)) * 16], 16 * sizeof(float));
        *L = m->add_layer(vfi_conv_create_ex(1, w2.data(), b, cout, 3 * cin, 4, 2, 0, nullptr, 3 * cin, nullptr));
    };
    auto conv1x1 = [&](vfi_conv_t** L, int cout, int cin) {
        const float* w = cur.take((int64_t)cout * cin);
        if (cur.ok()) *L = m->add_layer(vfi_conv_create_ex(0, w, nullptr, cout, cin, 1, 1, 0, nullptr, cin, nullptr));
    };
    auto gate = [&](Gate& g, int c) {
        const float* w = cur.take((int64_t)c * c);
        const float* b = cur.take(c);
        if (cur.ok()) g.w = m->upload(w, (size_t)c * c), g.b = m->upload(b, c);
    };
    // stem / outconv weights: re-laid out on the device by their pack kernel (the raw copy stays among the object's parameter blocks)
    auto packed = [&](const float* w, size_t raw_floats, void (*pack)(const float*, float*), size_t floats) -> float* {
        float* raw = m->upload(w, raw_floats);
        float* wp = m->upload(nullptr, floats);
        if (!raw || !wp) return nullptr;
        pack<<<blocks(floats), 256>>>(raw, wp);
        if (hipDeviceSynchronize() != hipSuccess) set_error("vfi_flavr_create: weight pack kernel failed"), m->failed = true;
        return wp;
    };
    {
        const float* w = cur.take(ST_WFLOATS);
        const float* b = eb ? cur.take(64) : nullptr;
        if (cur.ok()) m->stem_wp = packed(w, ST_WFLOATS, flavr_stem_pack_kernel, ST_WFLOATS);
        if (cur.ok() && b) m->stem_b = m->upload(b, 64);
    }
    const int planes[4] = {64, 128, 256, 512};
    int inplanes = 64;
    for (int l = 0; l < 4 && cur.ok(); ++l)
        for (int b = 0; b < 2 && cur.ok(); ++b) {
            Block& B = m->blk[l * 2 + b];
            B.c = planes[l];
            B.cin = b == 0 ? inplanes : planes[l];
            B.stride = (b == 0 && (l == 1 || l == 2)) ? 2 : 1;
            conv3(&B.c1, B.c, B.cin, B.stride, eb);
            conv3(&B.c2, B.c, B.c, 1, eb);
            gate(B.g, B.c);
            if (b == 0 && B.cin != B.c) conv1x1(&B.ds, B.c, B.cin);
            inplanes = planes[l];
        }
    conv3(&m->dec[0], 256, 512, 1, true), gate(m->dg[0], 256);
    deconv(&m->dec[1], 512, 128), gate(m->dg[1], 128);
    deconv(&m->dec[2], 256, 64), gate(m->dg[2], 64);
    conv3(&m->dec[3], 64, 128, 1, true), gate(m->dg[3], 64);
    deconv(&m->dec[4], 128, 64), gate(m->dg[4], 64);
    conv1x1(&m->fuse, 64, T * 64);
    {      // outconv.1: only output 0's three channels are computed (the node takes model(...)[0])
        const float* w = cur.take((int64_t)3 * n_outputs * 64 * 49);
        const float* b = cur.take(3 * n_outputs);
        if (cur.ok()) m->out_wp = packed(w, 3 * 64 * 49, flavr_out_pack_kernel, FO_WFLOATS), m->out_b = m->upload(b, 3);
    }
    if (!cur.finish() || m->failed) {
        vfi_flavr_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_flavr_destroy(vfi_flavr_t* m) { delete m; }

int vfi_flavr_release_workspace(vfi_flavr_t* m) {
    VFI_REQUIRE(m, "vfi_flavr_release_workspace: null object");
    return m->ws.release();
}

int64_t vfi_flavr_workspace_bytes(const vfi_flavr_t* m) { return m ? m->ws.bytes() : 0; }

int64_t vfi_flavr_max_padded_pixels(void) { return kMaxPixels; }

int64_t vfi_flavr_large_max_padded_pixels(void) { return kLargeMaxPixels; }

int64_t vfi_flavr_object_max_padded_pixels(const vfi_flavr_t* m) { return !m ? 0 : (m->large ? kLargeMaxPixels : kMaxPixels); }

// The permission for operand images of 4 GiB and more goes to every layer object with the switch (and leaves with it): below the old limit
// no layer meets an image of 2 GiB, so the permission changes no launch there.
int vfi_flavr_set_large_frames(vfi_flavr_t* m, int on) {
    VFI_REQUIRE(m, "vfi_flavr_set_large_frames: null object");
    for (vfi_conv_t* L : m->layers)
        if (vfi_conv_allow_huge(L, on != 0)) return -1;
    m->large = on != 0;
    return 0;
}

int vfi_flavr_forward(vfi_flavr_t* m, const float* const* frames_dev, int N, int C, int H, int W, float* out_dev, void* stream) {
    VFI_REQUIRE(m && frames_dev && out_dev && N > 0 && C >= 3 && H > 0 && W > 0, "vfi_flavr_forward: bad arguments");
    for (int i = 0; i < T * N; ++i) VFI_REQUIRE(frames_dev[i], "vfi_flavr_forward: null frame pointer %d", i);
    const int Hp = pad16(H), Wp = pad16(W);
    VFI_REQUIRE(m->large || size_ok(Hp, Wp),
                "vfi_flavr_forward: a %dx%d frame (padded %dx%d) is over the size limit: the last up-convolution's [Hp, Wp, 256] fp32 tensor must stay "
                "below 2 GiB (Hp * Wp <= 2097151; 1088x1920 fits)",
                H, W, Hp, Wp);
    VFI_REQUIRE(!m->large || size_ok_large(Hp, Wp),
                "vfi_flavr_forward: a %dx%d frame (padded %dx%d) is over the size limit with large frames on: the last up-convolution's [Hp, Wp, 256] fp32 "
                "tensor must stay within the layer kernels' 2^31 - 1 floats per image (Hp * Wp <= %ld; 2160x3840 fits)",
                H, W, Hp, Wp, kLargeMaxPixels);
    hipStream_t st = (hipStream_t)stream;
    if (ensure_workspace(m, Hp, Wp, st)) return -1;
    for (int n = 0; n < N; ++n)
        if (forward_window(m, frames_dev + (size_t)T * n, C, H, W, out_dev + (size_t)n * H * W * 3, st)) return -1;
    return 0;
}

}  // extern "C"
