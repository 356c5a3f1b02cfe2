// The reference's remaining custom ops (vfi_models/ops/cupy_ops) as HIP kernels for gfx950, NCHW fp32, for the drop-in ops
// backend cfi_amd.ops:
//
//   separable adaptive convolution   replaces sepconv_out,                   cupy_ops/sepconv.py:86-117
//   AdaCoF forward                   replaces kernel_AdaCoF_updateOutput,    cupy_ops/adacof.py:6-65
//   PWC correlation (81 channels)    replaces kernel_Correlation_rearrange + kernel_Correlation_updateOutput, correlation.py:5-102
//   distance transform (two passes)  replaces kernel_dt,                     cupy_ops/batch_edt.py:11-40
//
// Every operand except AdaCoF's is addressed through explicit element strides (the reference's VALUE_4 / OFFSET_4), so channel
// slices such as tenOut[:, :-1] are read in place.  No entry allocates or synchronises; all launches go to the caller's stream.
#include <algorithm>

#include "vfi_common.h"

#include "../../include/vfi_hip.h"

namespace vfi {
namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

struct S4 {   // element strides of an NCHW operand
    long long n, c, y, x;
};

__device__ __forceinline__ size_t at(const S4& s, int n, int c, int y, int x) {
    return (size_t)((long long)n * s.n + (long long)c * s.c + (long long)y * s.y + (long long)x * s.x);
}

// ---- separable adaptive convolution -------------------------------------------------------------------------------------------
// out[n,c,y,x] = sum_fy ver[n,fy,y,x] * (sum_fx in[n,c,y+fy,x+fx] * hor[n,fx,y,x]).  The reference forms in * ver * hor per tap
// and sums all K^2 products with Kahan compensation; here each input row is first reduced against the K horizontal taps (kept in
// registers) and the row sums are weighted by ver — K^2 + K FMAs instead of 2 K^2 multiplies, a different fp32 order.
//
// A workgroup owns an output tile 64 wide x 8 high; a thread owns the pixel PAIR (y, x), (y+1, x) and 4 channels.  Input rows stream
// through LDS, SEP_RS rows at a time, 64 + K - 1 columns, the 4 channels interleaved (one ds_read_b128 per tap): input row r is tap
// row r - y of the upper pixel and r - y - 1 of the lower one, so one LDS read feeds 8 FMAs (two pixels x four channels), which is
// what the LDS array (256 B/clk/CU) needs to keep the f32 VALU at its packed rate (v_pk_fma_f32, two channels per instruction:
// there are no MFMAs in this kernel for packed VALU to steal issue slots from).  A wave is one pixel-row pair, so the "is this row a
// tap of mine" test is wave-uniform.
constexpr int SEP_TX = 64, SEP_TY = 8, SEP_RS = 8;

template <int K>
__global__ __launch_bounds__(256, 2) void sepconv_tile_kernel(const float* __restrict__ in, S4 si, const float* __restrict__ ver, S4 sv,
                                                           const float* __restrict__ hor, S4 sh, float* __restrict__ out, S4 so,
                                                           int C, int Hin, int Win, int Ho, int Wo, int cgroups) {
    constexpr int LW = SEP_TX + K - 1;
    constexpr int ROWS = SEP_TY + K - 1;
    __shared__ float4 lds[SEP_RS][LW];
    const int tid = threadIdx.x;
    const int tx = tid & 63, tp = tid >> 6;          // tp = wave = pixel-row pair
    const int x0 = blockIdx.x * SEP_TX, y0 = blockIdx.y * SEP_TY;
    const int n = blockIdx.z / cgroups, c0 = (blockIdx.z - n * cgroups) * 4;
    const int x = x0 + tx, ya = y0 + 2 * tp, yb = ya + 1;
    const bool va = x < Wo && ya < Ho, vb = x < Wo && yb < Ho;
    float ha[K], hb[K];
#pragma unroll
    for (int f = 0; f < K; ++f) {
        ha[f] = va ? hor[at(sh, n, f, ya, x)] : 0.f;
        hb[f] = vb ? hor[at(sh, n, f, yb, x)] : 0.f;
    }
    f2 aa_lo = {0.f, 0.f}, aa_hi = {0.f, 0.f}, ab_lo = {0.f, 0.f}, ab_hi = {0.f, 0.f};
    for (int r0 = 0; r0 < ROWS; r0 += SEP_RS) {
        __syncthreads();
        for (int i = tid; i < SEP_RS * LW; i += 256) {
            const int rr = i / LW, cc = i - rr * LW;
            const int gy = y0 + r0 + rr, gx = x0 + cc;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (r0 + rr < ROWS && gy < Hin && gx < Win) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < C) v[j] = in[at(si, n, c0 + j, gy, gx)];
            }
            lds[rr][cc] = make_float4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        for (int rr = 0; rr < SEP_RS; ++rr) {
            const int fa = r0 + rr - 2 * tp;        // tap row of the upper pixel; the lower one's is fa - 1
            if (fa < 0 || fa > K) continue;         // wave-uniform
            const bool use_a = fa < K, use_b = fa >= 1;
            f2 ra_lo = {0.f, 0.f}, ra_hi = {0.f, 0.f}, rb_lo = {0.f, 0.f}, rb_hi = {0.f, 0.f};
            if (use_a && use_b) {
#pragma unroll
                for (int f = 0; f < K; ++f) {
                    const float4 v = lds[rr][tx + f];
                    const f2 lo = {v.x, v.y}, hi = {v.z, v.w};
                    ra_lo += lo * ha[f];
                    ra_hi += hi * ha[f];
                    rb_lo += lo * hb[f];
                    rb_hi += hi * hb[f];
                }
            } else if (use_a) {
#pragma unroll
                for (int f = 0; f < K; ++f) {
                    const float4 v = lds[rr][tx + f];
                    ra_lo += f2{v.x, v.y} * ha[f];
                    ra_hi += f2{v.z, v.w} * ha[f];
                }
            } else {
#pragma unroll
                for (int f = 0; f < K; ++f) {
                    const float4 v = lds[rr][tx + f];
                    rb_lo += f2{v.x, v.y} * hb[f];
                    rb_hi += f2{v.z, v.w} * hb[f];
                }
            }
            if (use_a) {
                const float w = va ? ver[at(sv, n, fa, ya, x)] : 0.f;
                aa_lo += ra_lo * w;
                aa_hi += ra_hi * w;
            }
            if (use_b) {
                const float w = vb ? ver[at(sv, n, fa - 1, yb, x)] : 0.f;
                ab_lo += rb_lo * w;
                ab_hi += rb_hi * w;
            }
        }
    }
    const float ra[4] = {aa_lo.x, aa_lo.y, aa_hi.x, aa_hi.y}, rb[4] = {ab_lo.x, ab_lo.y, ab_hi.x, ab_hi.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c0 + j >= C) break;
        if (va) out[at(so, n, c0 + j, ya, x)] = ra[j];
        if (vb) out[at(so, n, c0 + j, yb, x)] = rb[j];
    }
}

// Any other K: one thread per output element, the same row-sum order as the tile kernel.
__global__ __launch_bounds__(256) void sepconv_any_kernel(const float* __restrict__ in, S4 si, const float* __restrict__ ver, S4 sv,
                                                          const float* __restrict__ hor, S4 sh, float* __restrict__ out, S4 so, int N,
                                                          int C, int Ho, int Wo, int K) {
    const long long total = (long long)N * C * Ho * Wo;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho), c = (int)((i / ((long long)Wo * Ho)) % C);
        const int n = (int)(i / ((long long)Wo * Ho * C));
        float acc = 0.f;
        for (int fy = 0; fy < K; ++fy) {
            float rs = 0.f;
            for (int fx = 0; fx < K; ++fx) rs += in[at(si, n, c, y + fy, x + fx)] * hor[at(sh, n, fx, y, x)];
            acc += rs * ver[at(sv, n, fy, y, x)];
        }
        out[at(so, n, c, y, x)] = acc;
    }
}

// ---- AdaCoF forward ---------------------------------------------------------------------------------------------------------------
// One thread per output PIXEL: the F*F taps' weight / offsets and clamped corners are computed once and applied to every channel
// (the reference recomputes them per channel).  Per channel the taps are summed in the reference's order (k, then l) with its exact
// expression; A = (int)alpha truncates toward zero, so a negative offset's fraction alpha - A is negative and the bilinear weights
// extrapolate, as in the reference.  Contiguous operands (adacof.py:286-289).
constexpr int ADACOF_CMAX = 8;   // channels per pass

__global__ __launch_bounds__(256) void adacof_kernel(const float* __restrict__ input, const float* __restrict__ weight,
                                                     const float* __restrict__ off_i, const float* __restrict__ off_j,
                                                     float* __restrict__ output, int N, int C, int H, int W, int Ho, int Wo, int F,
                                                     int dil) {
    const long long total = (long long)N * Ho * Wo;
    const long long p = blockIdx.x * 256ll + threadIdx.x;
    if (p >= total) return;
    const int j = (int)(p % Wo), i = (int)((p / Wo) % Ho), n = (int)(p / ((long long)Wo * Ho));
    const size_t plane = (size_t)Ho * Wo, pix = (size_t)i * Wo + j;
    const size_t tap0 = (size_t)n * F * F * plane + pix;
    const size_t inplane = (size_t)H * W;
    for (int c0 = 0; c0 < C; c0 += ADACOF_CMAX) {
        const int nc = min(ADACOF_CMAX, C - c0);
        float acc[ADACOF_CMAX];
#pragma unroll
        for (int c = 0; c < ADACOF_CMAX; ++c) acc[c] = 0.f;
        const float* src = input + ((size_t)n * C + c0) * inplane;
        for (int k = 0; k < F; ++k) {
            for (int l = 0; l < F; ++l) {
                const size_t t = tap0 + (size_t)(k * F + l) * plane;
                const float w = weight[t], alpha = off_i[t], beta = off_j[t];
                const int A = (int)alpha, B = (int)beta;
                const int ia = min(max(i + k * dil + A, 0), H - 1), ia1 = min(max(i + k * dil + A + 1, 0), H - 1);
                const int jb = min(max(j + l * dil + B, 0), W - 1), jb1 = min(max(j + l * dil + B + 1, 0), W - 1);
                const float fa = alpha - (float)A, fb = beta - (float)B;
                const size_t o00 = (size_t)ia * W + jb, o10 = (size_t)ia1 * W + jb, o01 = (size_t)ia * W + jb1, o11 = (size_t)ia1 * W + jb1;
#pragma unroll
                for (int c = 0; c < ADACOF_CMAX; ++c) {
                    if (c < nc) {
                        const float* s = src + (size_t)c * inplane;
                        acc[c] += w * (s[o00] * (1 - fa) * (1 - fb) + s[o10] * fa * (1 - fb) + s[o01] * (1 - fa) * fb + s[o11] * fa * fb);
                    }
                }
            }
        }
        float* dst = output + ((size_t)n * C + c0) * plane + pix;
#pragma unroll
        for (int c = 0; c < ADACOF_CMAX; ++c)
            if (c < nc) dst[(size_t)c * plane] = acc[c];
    }
}

// ---- PWC correlation ------------------------------------------------------------------------------------------------------------
// out[n, 9*(dy+4) + (dx+4), y, x] = (1/C) sum_c a[n,c,y,x] * b[n,c,y+dy,x+dx], b outside the image = 0 — the reference's
// rearrange-into-a-zero-padded-copy + 32-lane reduction in one kernel.  A workgroup owns a 16x16 pixel tile and keeps its 81 sums
// per pixel in registers; per pass of CORR_CK channels the tile of `a` and the 24x24 halo of `b` (zero outside) come from LDS.
// The sum runs over c in order (the reference's 32 interleaved partial sums differ by rounding only); then / (float)C as there.
constexpr int CORR_T = 16, CORR_HW = CORR_T + 8, CORR_CK = 8;

__global__ __launch_bounds__(256) void correlation_kernel(const float* __restrict__ a, S4 sa, const float* __restrict__ b, S4 sb,
                                                          float* __restrict__ out, int C, int H, int W, int tiles_x) {
    __shared__ float la[CORR_CK][CORR_T * CORR_T];
    __shared__ float lb[CORR_CK][CORR_HW * CORR_HW];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int ty0 = (blockIdx.x / tiles_x) * CORR_T, tx0 = (blockIdx.x % tiles_x) * CORR_T;
    const int py = tid / CORR_T, px = tid % CORR_T;
    float acc[81];
#pragma unroll
    for (int d = 0; d < 81; ++d) acc[d] = 0.f;
    for (int c0 = 0; c0 < C; c0 += CORR_CK) {
        __syncthreads();
        for (int e = tid; e < CORR_CK * CORR_T * CORR_T; e += 256) {
            const int c = e / (CORR_T * CORR_T), q = e - c * CORR_T * CORR_T;
            const int gy = ty0 + q / CORR_T, gx = tx0 + q % CORR_T;
            la[c][q] = (c0 + c < C && gy < H && gx < W) ? a[at(sa, n, c0 + c, gy, gx)] : 0.f;
        }
        for (int e = tid; e < CORR_CK * CORR_HW * CORR_HW; e += 256) {
            const int c = e / (CORR_HW * CORR_HW), q = e - c * CORR_HW * CORR_HW;
            const int gy = ty0 - 4 + q / CORR_HW, gx = tx0 - 4 + q % CORR_HW;
            lb[c][q] = (c0 + c < C && gy >= 0 && gy < H && gx >= 0 && gx < W) ? b[at(sb, n, c0 + c, gy, gx)] : 0.f;
        }
        __syncthreads();
        const int nc = min(CORR_CK, C - c0);
        for (int c = 0; c < nc; ++c) {
            const float va = la[c][py * CORR_T + px];
            const float* row = &lb[c][py * CORR_HW + px];
#pragma unroll
            for (int dy = 0; dy < 9; ++dy)
#pragma unroll
                for (int dx = 0; dx < 9; ++dx) acc[dy * 9 + dx] += va * row[dy * CORR_HW + dx];
        }
    }
    const int y = ty0 + py, x = tx0 + px;
    if (y < H && x < W) {
        const size_t plane = (size_t)H * W;
        float* o = out + (size_t)n * 81 * plane + (size_t)y * W + x;
#pragma unroll
        for (int d = 0; d < 81; ++d) o[d * plane] = acc[d] / (float)C;
    }
}

// ---- distance transform -----------------------------------------------------------------------------------------------------------
// One pass of kernel_dt along lines of length L: out[p] = min(diam2, min_j data[j] + (float)((p - j)^2)).  A workgroup owns one
// line, staged whole in LDS; the line is rows (element stride 1) in the first pass and columns (element stride W) in the second —
// the reference transposes in between instead.  Every candidate is formed exactly as in the reference and min does not depend on
// order, so the result is bit-identical for any data, not only for binary masks.  The second pass also takes the square root,
// correctly rounded like the GPU sqrt after the reference's kernels.  Bit-identical to the exact distance transform at every shape
// tested, 1080p included (tests/test_gpu_ref_ops_edges.py, test_gpu_ref_ops.py::test_edt_1080p).  The one-ulp differences once
// seen at 1080p were the host's: torch's CPU sqrt of a float32 tensor is not correctly rounded (on an EPYC host it is one ulp off
// in 14 % of those pixels); the tests now take numpy's float64 sqrt rounded to float32.
// Correctly rounded sqrt of a non-negative float: sqrtf, then moved by an ulp while m lies outside the square of the rounding
// interval [mid(prev, s), mid(s, next)] — the midpoints have 25 significant bits, so their squares are exact in double.  On gfx950
// sqrtf already lowers to v_sqrt_f32 plus an fma test of both neighbours and is correctly rounded by itself (every integer below
// 2^24 and 2^22 random floats below 2^25, test_edt_sqrt_exhaustive, with or without the loop); the loop is kept as a guard.
__device__ __forceinline__ float sqrt_rn(float m) {
    float s = sqrtf(m);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double lo = 0.5 * ((double)s + (double)nextafterf(s, 0.f));
        const double hi = 0.5 * ((double)s + (double)nextafterf(s, INFINITY));
        if ((double)m < lo * lo) s = nextafterf(s, 0.f);
        else if ((double)m > hi * hi) s = nextafterf(s, INFINITY);
    }
    return s;
}

__global__ __launch_bounds__(256) void edt_line_kernel(const float* __restrict__ data, float* __restrict__ out, int L, int lines_per_img,
                                                       long long img_stride, long long line_stride, long long elem_stride, float diam2,
                                                       int do_sqrt) {
    extern __shared__ float line[];
    const int img = blockIdx.x / lines_per_img, li = blockIdx.x - img * lines_per_img;
    const size_t base = (size_t)img * img_stride + (size_t)li * line_stride;
    for (int j = threadIdx.x; j < L; j += 256) line[j] = data[base + (size_t)j * elem_stride];
    __syncthreads();
    for (int p = threadIdx.x; p < L; p += 256) {
        float m = diam2;
        for (int j = 0; j < L; ++j) {
            const float cost = line[j] + (float)((p - j) * (p - j));
            if (cost < m) m = cost;
        }
        out[base + (size_t)p * elem_stride] = do_sqrt ? sqrt_rn(m) : m;
    }
}

S4 strides(const long long* s) { return S4{s[0], s[1], s[2], s[3]}; }

}  // namespace
}  // namespace vfi

using namespace vfi;

extern "C" {

int vfi_sepconv(const float* in_dev, const long long* in_strides, const float* ver_dev, const long long* ver_strides, const float* hor_dev,
                const long long* hor_strides, float* out_dev, const long long* out_strides, int N, int C, int Hin, int Win, int Ho,
                int Wo, int K, void* stream) {
    VFI_REQUIRE(in_dev && ver_dev && hor_dev && out_dev && in_strides && ver_strides && hor_strides && out_strides,
                "vfi_sepconv: null argument");
    VFI_REQUIRE(N > 0 && C > 0 && Ho > 0 && Wo > 0 && K > 0 && Hin >= Ho + K - 1 && Win >= Wo + K - 1,
                "vfi_sepconv: bad shape N=%d C=%d in %dx%d out %dx%d K=%d (the input must hold out + K - 1 rows and columns)", N, C,
                Hin, Win, Ho, Wo, K);
    hipStream_t s = (hipStream_t)stream;
    const S4 si = strides(in_strides), sv = strides(ver_strides), sh = strides(hor_strides), so = strides(out_strides);
    TraceScope ts("sepconv", s);
    if (K == 51) {
        const int cgroups = (C + 3) / 4;
        VFI_REQUIRE((long long)N * cgroups < 65536, "vfi_sepconv: N*ceil(C/4)=%lld exceeds the grid", (long long)N * cgroups);
        hipLaunchKernelGGL(sepconv_tile_kernel<51>, dim3((Wo + SEP_TX - 1) / SEP_TX, (Ho + SEP_TY - 1) / SEP_TY, N * cgroups), dim3(256),
                           0, s, in_dev, si, ver_dev, sv, hor_dev, sh, out_dev, so, C, Hin, Win, Ho, Wo, cgroups);
    } else {
        const long long total = (long long)N * C * Ho * Wo;
        const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 1 << 20);
        hipLaunchKernelGGL(sepconv_any_kernel, dim3(blocks), dim3(256), 0, s, in_dev, si, ver_dev, sv, hor_dev, sh, out_dev, so, N, C, Ho,
                           Wo, K);
    }
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_adacof(const float* input_dev, const float* weight_dev, const float* offset_i_dev, const float* offset_j_dev, float* out_dev,
               int N, int C, int H, int W, int F, int dilation, int Ho, int Wo, void* stream) {
    VFI_REQUIRE(input_dev && weight_dev && offset_i_dev && offset_j_dev && out_dev, "vfi_adacof: null argument");
    VFI_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && F > 0 && dilation > 0 && Ho > 0 && Wo > 0, "vfi_adacof: bad arguments");
    VFI_REQUIRE(H - ((F - 1) * dilation + 1) == Ho - 1 && W - ((F - 1) * dilation + 1) == Wo - 1,
                "vfi_adacof: output %dx%d does not match input %dx%d with F=%d dilation=%d (adacof.py:274-284)", Ho, Wo, H, W, F,
                dilation);
    hipStream_t s = (hipStream_t)stream;
    const long long px = (long long)N * Ho * Wo;
    TraceScope ts("adacof", s);
    hipLaunchKernelGGL(adacof_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, input_dev, weight_dev, offset_i_dev,
                       offset_j_dev, out_dev, N, C, H, W, Ho, Wo, F, dilation);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_correlation81(const float* a_dev, const long long* a_strides, const float* b_dev, const long long* b_strides, float* out_dev,
                      int N, int C, int H, int W, void* stream) {
    VFI_REQUIRE(a_dev && b_dev && out_dev && a_strides && b_strides, "vfi_correlation81: null argument");
    VFI_REQUIRE(N > 0 && N < 65536 && C > 0 && H > 0 && W > 0, "vfi_correlation81: bad shape N=%d C=%d H=%d W=%d", N, C, H, W);
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (W + CORR_T - 1) / CORR_T, tiles_y = (H + CORR_T - 1) / CORR_T;
    TraceScope ts("correlation81", s);
    hipLaunchKernelGGL(correlation_kernel, dim3(tiles_x * tiles_y, N), dim3(256), 0, s, a_dev, strides(a_strides), b_dev,
                       strides(b_strides), out_dev, C, H, W, tiles_x);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_edt(const float* data_dev, float* tmp_dev, float* out_dev, int N, int H, int W, float diam2, void* stream) {
    VFI_REQUIRE(data_dev && tmp_dev && out_dev && N > 0 && H > 0 && W > 0, "vfi_edt: bad arguments");
    VFI_REQUIRE(tmp_dev != data_dev && tmp_dev != out_dev, "vfi_edt: tmp must not alias data or out");
    VFI_REQUIRE(H <= 16384 && W <= 16384, "vfi_edt: %dx%d: a line of more than 16384 pixels does not fit the LDS", H, W);
    hipStream_t s = (hipStream_t)stream;
    const long long img = (long long)H * W;
    TraceScope ts("edt", s);
    // first pass along rows (batch_edt.py:72-84), second along columns (:86-99)
    hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)(N * H)), dim3(256), W * sizeof(float), s, data_dev, tmp_dev, W, H, img,
                       (long long)W, 1ll, diam2, 0);
    hipLaunchKernelGGL(edt_line_kernel, dim3((unsigned)(N * W)), dim3(256), H * sizeof(float), s, tmp_dev, out_dev, H, W, img, 1ll,
                       (long long)W, diam2, 1);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
