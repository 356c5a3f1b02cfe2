// CAIN interpolator (vfi_models/cain/cain_arch.py CAIN(depth=3), common.py) as a C-side object: vfi_cain_create / vfi_cain_forward /
// vfi_cain_destroy — weights packed once, workspace owned, the ~320 launches of a batch of frame pairs issued by one call.
//
// Forward (cain_arch.py:56-74): sub_mean of both frames (common.py:7-10), reflect padding to a multiple of 128 (InOutPaddings,
// :12-23), pixel_shuffle(1/8) to 192 channels each, Interpolation (:300-335): headConv 384 -> 192 (zero padding), 5 ResidualGroups of
// 12 RCABs + one ConvNorm (reflect padding) plus the group input, res += head, tailConv (zero padding); pixel_shuffle(8), crop, + the
// mean of the two frame means.  No clamp.
//
// New kernels here: the frame-in (mean removal + reflect pad + x8 unshuffle) and frame-out (x8 shuffle + crop + mean) data movement, and
// squeeze-and-excitation channel attention (CALayer, common.py:132-148) in three deterministic launches: per-workgroup channel sums into
// fixed slots, a one-workgroup-per-image pass that sums them in a fixed order and runs the 192 -> 12 -> 192 MLP + sigmoid, and the
// scale-and-residual `t * s + x`.  No float atomics: a frame's bits do not depend on scheduling.  The 3x3 layers run on
// vfi_conv_forward_ex (pad_mode 2 = reflect on the Winograd and direct kernels).
#include <cstring>
#include <vector>

#include "../../include/vfi_hip.h"
#include "net_object.h"
#include "vfi_common.h"

using namespace vfi;

namespace {

constexpr int FEAT = 192;          // 3 * 4^3 channels of the unshuffled frame = n_feats of Interpolation
constexpr int RED = 12;            // CALayer reduction 16: 192 -> 12
constexpr int GROUPS = 5, BLOCKS = 12;
constexpr int SHUF = 8;            // 2^depth
constexpr int ALIGN = 128;         // InOutPaddings: multiple of 2^7
constexpr int MEAN_SLOTS = 256;    // frame-in: row-block partial sums per frame
constexpr int CA_SLOTS = 256;      // channel attention: pixel-block partial sums per image (at most)

// ---- frame-in ------------------------------------------------------------------------------------------------------------
// partial[b][c] = sum of channel c over rows b, b + G, b + 2G, ... (G = gridDim.x); fixed-order tree in LDS
__global__ __launch_bounds__(256) void cain_mean_partial_kernel(const float* __restrict__ f, int C, int H, int W, float* __restrict__ partial) {
    __shared__ float red[3][256];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const float* row = f + (size_t)y * W * C;
        for (int x = threadIdx.x; x < W; x += 256) {
            s0 += row[x * C + 0];
            s1 += row[x * C + 1];
            s2 += row[x * C + 2];
        }
    }
    red[0][threadIdx.x] = s0, red[1][threadIdx.x] = s1, red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void cain_mean_final_kernel(const float* __restrict__ partial, int G, float inv_hw, float* __restrict__ mean) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    float s = 0.f;
    for (int b = 0; b < G; ++b) s += partial[b * 3 + c];
    mean[c] = s * inv_hw;
}

// one thread = (pixel Y, X of the unshuffled map, colour c, sub-row dy): the 8 channels c*64 + dy*8 + 0..7 (pixel_shuffle(1/8),
// common.py:208-210), each = frame[reflect(8Y + dy - top), reflect(8X + dx - left), c] - mean[c]
__global__ __launch_bounds__(256) void cain_frame_in_kernel(const float* __restrict__ f, int C, int H, int W, int top, int left, int h, int w,
                                                            const float* __restrict__ mean, float* __restrict__ out, int out_cs) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)h * w * 24) return;
    const int cd = (int)(idx % 24);
    const long p = idx / 24;
    const int c = cd >> 3, dy = cd & 7;
    const int Y = (int)(p / w), X = (int)(p - (long)Y * w);
    int y = Y * SHUF + dy - top;
    y = y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y);       // padding < H (checked by the host): one reflection is enough
    const float m = mean[c];
    const float* row = f + (size_t)y * W * C + c;
    float v[8];
#pragma unroll
    for (int dx = 0; dx < 8; ++dx) {
        int x = X * SHUF + dx - left;
        x = x < 0 ? -x : (x >= W ? 2 * W - 2 - x : x);
        v[dx] = row[(size_t)x * C] - m;
    }
    float4* o = (float4*)(out + p * out_cs + c * 64 + dy * 8);
    o[0] = make_float4(v[0], v[1], v[2], v[3]);
    o[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- frame-out -----------------------------------------------------------------------------------------------------------------
// out[n, y, x, c] = t[n, (y + top) / 8, (x + left) / 8, c*64 + ((y + top) % 8) * 8 + (x + left) % 8] + (m0[c] + m1[c]) / 2
__global__ __launch_bounds__(256) void cain_frame_out_kernel(const float* __restrict__ t, int h, int w, int top, int left,
                                                             const float* __restrict__ means, float* __restrict__ out, int N, int H, int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * H * W) return;
    const int n = (int)(idx / ((long)H * W));
    const long r = idx - (long)n * H * W;
    const int y = (int)(r / W) + top, x = (int)(r % W) + left;
    const float* src = t + (((size_t)n * h + (y >> 3)) * w + (x >> 3)) * FEAT + (y & 7) * 8 + (x & 7);
    const float* m = means + n * 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[idx * 3 + c] = src[c * 64] + (m[c] + m[3 + c]) / 2.f;
}

// ---- channel attention ---------------------------------------------------------------------------------------------------------
static int ca_blocks(long hw) {      // pixel blocks per image: a function of the image alone (never of the batch)
    const long b = (hw + 63) / 64;
    return (int)(b < CA_SLOTS ? b : CA_SLOTS);
}

// partial[n][b][c] = sum over the pixels of block b of t[n, p, c]; thread = (channel quad, pixel lane)
__global__ __launch_bounds__(256) void ca_partial_kernel(const float* __restrict__ t, long hw, int C, int nb, float* __restrict__ partial) {
    __shared__ float red[256 * 4];
    const int n = blockIdx.y, b = blockIdx.x;
    const int quads = C / 4, lanes = 256 / quads;
    const int q = threadIdx.x % quads, lane = threadIdx.x / quads;
    const long per = (hw + nb - 1) / nb;
    const long p0 = b * per, p1 = p0 + per < hw ? p0 + per : hw;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < lanes) {
        const float* base = t + (size_t)n * hw * C + q * 4;
        for (long p = p0 + lane; p < p1; p += lanes) {
            const float4 v = *(const float4*)(base + p * C);
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        *(float4*)(red + lane * C + q * 4) = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        float a = 0.f;
        for (int l = 0; l < lanes; ++l) a += red[l * C + threadIdx.x];
        partial[((size_t)n * CA_SLOTS + b) * C + threadIdx.x] = a;
    }
}

// scale[n][c] = sigmoid(b2[c] + sum_j w2[c][j] * relu(b1[j] + sum_k w1[j][k] * mean[k]))   (conv_du, common.py:138-143).
// The slot sums are spread over (channel quad, slot lane) threads like ca_partial_kernel; each wave computes hidden units j = wave,
// wave + 4, ... with a fixed butterfly over its 64 lanes.  Every order is fixed: the result does not depend on scheduling.
__global__ __launch_bounds__(256) void ca_mlp_kernel(const float* __restrict__ partial, int nb, float inv_hw, int C, int R,
                                                     const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, float* __restrict__ scale) {
    __shared__ float red[256 * 4];
    __shared__ float mean[256];
    __shared__ float hid[64];
    const int n = blockIdx.x, c = threadIdx.x;
    const int quads = C / 4, lanes = 256 / quads;
    const int q = threadIdx.x % quads, lane = threadIdx.x / quads;
    if (lane < lanes) {
        const float* base = partial + (size_t)n * CA_SLOTS * C + q * 4;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = lane; b < nb; b += lanes) {
            const float4 v = *(const float4*)(base + (size_t)b * C);
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
        *(float4*)(red + lane * C + q * 4) = s;
    }
    __syncthreads();
    if (c < C) {
        float a = 0.f;
        for (int l = 0; l < lanes; ++l) a += red[l * C + c];
        mean[c] = a * inv_hw;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
    for (int j = wave; j < R; j += 4) {
        float a = 0.f;
        for (int k = wl; k < C; k += 64) a += w1[j * C + k] * mean[k];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
        if (wl == 0) hid[j] = fmaxf(b1[j] + a, 0.f);
    }
    __syncthreads();
    if (c < C) {
        float a = b2[c];
        for (int j = 0; j < R; ++j) a += w2[c * R + j] * hid[j];
        scale[n * C + c] = 1.f / (1.f + expf(-a));
    }
}

// out = t * scale[n][c] + x  (scale == nullptr: out = t + x); out may alias t or x
__global__ __launch_bounds__(256) void ca_apply_kernel(const float* t, const float* __restrict__ scale, const float* x, float* out, long per_img4,
                                                       int quads, long total4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const float4 a = ((const float4*)t)[i], r = ((const float4*)x)[i];
        float4 o;
        if (scale) {
            const int n = (int)(i / per_img4), q = (int)(i % quads);
            const float4 s = ((const float4*)scale)[n * quads + q];
            o = make_float4(a.x * s.x + r.x, a.y * s.y + r.y, a.z * s.z + r.z, a.w * s.w + r.w);
        } else {
            o = make_float4(a.x + r.x, a.y + r.y, a.z + r.z, a.w + r.w);
        }
        ((float4*)out)[i] = o;
    }
}

int pad_split(int n, int* before) {     // InOutPaddings (common.py:12-23): total padding to a multiple of 128, floor half before
    const int total = n % ALIGN ? (n / ALIGN + 1) * ALIGN - n : 0;
    *before = total / 2;
    return total;
}

int ca_launch(const float* t, const float* x, float* out, int N, long hw, int C, const float* w1, const float* b1, const float* w2,
              const float* b2, int R, float* ws, hipStream_t st) {
    const int nb = ca_blocks(hw);
    float* partial = ws;
    float* scale = ws + (size_t)N * CA_SLOTS * C;
    {
        TraceScope ts("cain_ca_partial", st);
        ca_partial_kernel<<<dim3(nb, N), 256, 0, st>>>(t, hw, C, nb, partial);
    }
    {
        TraceScope ts("cain_ca_mlp", st);
        ca_mlp_kernel<<<N, 256, 0, st>>>(partial, nb, 1.f / (float)hw, C, R, w1, b1, w2, b2, scale);
    }
    const long total4 = (long)N * hw * C / 4;
    TraceScope ts("cain_ca_apply", st);
    ca_apply_kernel<<<(unsigned)std::min<long>((total4 + 255) / 256, 8192), 256, 0, st>>>(t, scale, x, out, hw * C / 4, C / 4, total4);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

struct vfi_cain : NetObject {
    vfi_conv_t* head = nullptr;
    vfi_conv_t* tail = nullptr;
    vfi_conv_t* body[GROUPS][BLOCKS][2] = {};
    vfi_conv_t* gconv[GROUPS] = {};
    float* ca = nullptr;               // per RCAB: w1 [12][192], b1 [12], w2 [192][12], b2 [192]
    // workspace, for N pairs of h x w feature maps
    int N = 0, h = 0, w = 0;
    float *in = nullptr, *x0 = nullptr, *g[2] = {}, *cur = nullptr, *t1 = nullptr, *t2 = nullptr, *cws = nullptr, *means = nullptr;
};

namespace {

constexpr size_t CA_FLOATS = (size_t)RED * FEAT + RED + FEAT * RED + FEAT;

int ensure_workspace(vfi_cain* m, int N, int h, int w) {
    if (m->ws.live() && m->N >= N && m->h == h && m->w == w) return 0;
    if (m->ws.release()) return -1;
    const size_t px = (size_t)N * h * w;
    float** feats[] = {&m->x0, &m->g[0], &m->g[1], &m->cur, &m->t1, &m->t2};
    auto get = [&](float** p, size_t floats) { return m->ws.alloc(p, floats, Workspace::kNoFill, nullptr); };
    if (get(&m->in, px * 2 * FEAT)) return -1;
    for (float** f : feats)
        if (get(f, px * FEAT)) return -1;
    // channel-attention partials + scales, and the frame-in row partials (2 frames x MEAN_SLOTS x 3 per pair)
    const size_t ws = std::max((size_t)N * (CA_SLOTS + 1) * FEAT, (size_t)MEAN_SLOTS * 3);
    if (get(&m->cws, ws) || get(&m->means, (size_t)N * 6)) return -1;
    m->N = N, m->h = h, m->w = w;
    return 0;
}

int conv(const vfi_conv_t* L, const float* in, int in_cs, const vfi_cain* m, int N, float* out, int act, const float* res, hipStream_t st) {
    return vfi_conv_forward_ex(L, in, in_cs, m->h, m->w, out, FEAT, N, act, 0.2f, 0.f, 0.f, res, res ? FEAT : 0, st);
}

}  // namespace

extern "C" {

vfi_cain_t* vfi_cain_create(const float* const* tensors, const int64_t* numels, int n_tensors) {
    const int want = 4 + GROUPS * (BLOCKS * 8 + 2);
    if (!tensors || !numels || n_tensors != want) {
        set_error("vfi_cain_create: expected the %d state_dict tensors of CAIN(depth=3) in cain_spec.cain_shapes() order, got %d", want, n_tensors);
        return nullptr;
    }
    vfi_cain* m = new vfi_cain();
    TensorCursor cur(tensors, numels, n_tensors, "vfi_cain_create");
    auto make = [&](vfi_conv_t** L, int cin, int pad_mode) {
        const float* w = cur.take((int64_t)FEAT * cin * 9);
        const float* b = cur.take(FEAT);
        if (cur.ok()) *L = m->add_layer(vfi_conv_create_ex(0, w, b, FEAT, cin, 3, 1, pad_mode, nullptr, cin, nullptr));
    };
    std::vector<float> ca((size_t)GROUPS * BLOCKS * CA_FLOATS);
    make(&m->head, 2 * FEAT, 0);                               // conv3x3: zero padding (common.py:247-256)
    for (int gi = 0; gi < GROUPS && cur.ok(); ++gi) {
        for (int bi = 0; bi < BLOCKS && cur.ok(); ++bi) {
            make(&m->body[gi][bi][0], FEAT, 2);                // ConvNorm: ReflectionPad2d(1) + Conv2d (common.py:26-45)
            make(&m->body[gi][bi][1], FEAT, 2);
            float* dst = ca.data() + (size_t)(gi * BLOCKS + bi) * CA_FLOATS;
            const int64_t sizes[4] = {(int64_t)RED * FEAT, RED, (int64_t)FEAT * RED, FEAT};
            for (int i = 0; i < 4; ++i) {
                const float* s = cur.take(sizes[i]);
                if (s) memcpy(dst, s, sizes[i] * sizeof(float));
                dst += sizes[i];
            }
        }
        make(&m->gconv[gi], FEAT, 2);
    }
    make(&m->tail, FEAT, 0);
    if (cur.finish()) m->ca = m->upload(ca.data(), ca.size());
    if (!cur.ok() || m->failed) {
        vfi_cain_destroy(m);
        return nullptr;
    }
    return m;
}

void vfi_cain_destroy(vfi_cain_t* m) { delete m; }

int vfi_cain_release_workspace(vfi_cain_t* m) {
    VFI_REQUIRE(m, "vfi_cain_release_workspace: null object");
    return m->ws.release();
}

int64_t vfi_cain_workspace_bytes(const vfi_cain_t* m) { return m ? m->ws.bytes() : 0; }

int vfi_cain_frame_in(const float* frame_dev, int C, int H, int W, float* out_dev, int out_cs, float* mean_dev, float* workspace_dev,
                      int64_t workspace_bytes, void* stream) {
    VFI_REQUIRE(frame_dev && out_dev && mean_dev && workspace_dev && C >= 3 && H > 0 && W > 0 && out_cs >= FEAT && out_cs % 4 == 0 &&
                    ((uintptr_t)out_dev & 15) == 0,
                "vfi_cain_frame_in: bad arguments (C=%d H=%d W=%d out_cs=%d)", C, H, W, out_cs);
    VFI_REQUIRE(workspace_bytes >= (int64_t)MEAN_SLOTS * 3 * 4, "vfi_cain_frame_in: workspace must hold %d bytes", MEAN_SLOTS * 12);
    int top, left;
    const int ph = pad_split(H, &top), pw = pad_split(W, &left);
    VFI_REQUIRE(ph - top < H && pw - left < W,
                "CAIN: a %dx%d frame is too small for its reflection padding to %dx%d (padding must be smaller than the frame, as in "
                "torch.nn.ReflectionPad2d)", H, W, H + ph, W + pw);
    const int h = (H + ph) / SHUF, w = (W + pw) / SHUF;
    hipStream_t st = (hipStream_t)stream;
    const int G = H < MEAN_SLOTS ? H : MEAN_SLOTS;
    TraceScope ts("cain_frame_in", st);
    cain_mean_partial_kernel<<<G, 256, 0, st>>>(frame_dev, C, H, W, workspace_dev);
    cain_mean_final_kernel<<<1, 64, 0, st>>>(workspace_dev, G, 1.f / ((float)H * (float)W), mean_dev);
    const long n = (long)h * w * 24;
    cain_frame_in_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(frame_dev, C, H, W, top, left, h, w, mean_dev, out_dev, out_cs);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_cain_frame_out(const float* feat_dev, const float* means_dev, float* out_dev, int N, int H, int W, void* stream) {
    VFI_REQUIRE(feat_dev && means_dev && out_dev && N > 0 && H > 0 && W > 0, "vfi_cain_frame_out: bad arguments");
    int top, left;
    const int h = (H + pad_split(H, &top)) / SHUF, w = (W + pad_split(W, &left)) / SHUF;
    const long n = (long)N * H * W;
    hipStream_t st = (hipStream_t)stream;
    TraceScope ts("cain_frame_out", st);
    cain_frame_out_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(feat_dev, h, w, top, left, means_dev, out_dev, N, H, W);
    VFI_CHECK_HIP(hipGetLastError());
    return 0;
}

int vfi_channel_attention(const float* t_dev, const float* x_dev, float* out_dev, int N, int64_t HW, int C, const float* w1_dev,
                          const float* b1_dev, const float* w2_dev, const float* b2_dev, int R, void* workspace_dev, int64_t workspace_bytes,
                          void* stream) {
    VFI_REQUIRE(t_dev && x_dev && out_dev && w1_dev && b1_dev && w2_dev && b2_dev && workspace_dev && N > 0 && HW > 0,
                "vfi_channel_attention: bad arguments");
    VFI_REQUIRE(C % 4 == 0 && C >= 4 && C <= 256 && R >= 1 && R <= 64, "vfi_channel_attention: needs C %% 4 == 0, 4 <= C <= 256, 1 <= R <= 64 (C=%d R=%d)", C, R);
    VFI_REQUIRE(((uintptr_t)t_dev & 15) == 0 && ((uintptr_t)x_dev & 15) == 0 && ((uintptr_t)out_dev & 15) == 0,
                "vfi_channel_attention: tensors must be 16-byte aligned");
    VFI_REQUIRE(workspace_bytes >= (int64_t)N * (CA_SLOTS + 1) * C * 4, "vfi_channel_attention: workspace must hold %lld bytes",
                (long long)N * (CA_SLOTS + 1) * C * 4);
    return ca_launch(t_dev, x_dev, out_dev, N, HW, C, w1_dev, b1_dev, w2_dev, b2_dev, R, (float*)workspace_dev, (hipStream_t)stream);
}

int vfi_cain_forward(vfi_cain_t* m, const float* const* frame0_dev, const float* const* frame1_dev, int N, int C, int H, int W, float* out_dev,
                     void* stream) {
    VFI_REQUIRE(m && frame0_dev && frame1_dev && out_dev && N > 0 && C >= 3 && H > 0 && W > 0, "vfi_cain_forward: bad arguments");
    int top, left;
    const int ph = pad_split(H, &top), pw = pad_split(W, &left);
    VFI_REQUIRE(ph - top < H && pw - left < W,
                "CAIN: a %dx%d frame is too small for its reflection padding to %dx%d (padding must be smaller than the frame, as in "
                "torch.nn.ReflectionPad2d)", H, W, H + ph, W + pw);
    for (int n = 0; n < N; ++n) VFI_REQUIRE(frame0_dev[n] && frame1_dev[n], "vfi_cain_forward: null frame pointer for pair %d", n);
    hipStream_t st = (hipStream_t)stream;
    if (ensure_workspace(m, N, (H + ph) / SHUF, (W + pw) / SHUF)) return -1;
    const long hw = (long)m->h * m->w;
    for (int n = 0; n < N; ++n)
        for (int f = 0; f < 2; ++f)
            if (int rc = vfi_cain_frame_in(f ? frame1_dev[n] : frame0_dev[n], C, H, W, m->in + (size_t)n * hw * 2 * FEAT + f * FEAT, 2 * FEAT,
                                           m->means + n * 6 + f * 3, m->cws, (int64_t)MEAN_SLOTS * 3 * 4, st))
                return rc;
    if (conv(m->head, m->in, 2 * FEAT, m, N, m->x0, 0, nullptr, st)) return -1;
    const float* gin = m->x0;
    for (int gi = 0; gi < GROUPS; ++gi) {
        const float* x = gin;
        for (int bi = 0; bi < BLOCKS; ++bi) {
            // RCAB (common.py:152-178): cur = CA(conv(lrelu(conv(x)))) + x
            if (conv(m->body[gi][bi][0], x, FEAT, m, N, m->t1, 1, nullptr, st) || conv(m->body[gi][bi][1], m->t1, FEAT, m, N, m->t2, 0, nullptr, st))
                return -1;
            const float* ca = m->ca + (size_t)(gi * BLOCKS + bi) * CA_FLOATS;
            if (ca_launch(m->t2, x, m->cur, N, hw, FEAT, ca, ca + RED * FEAT, ca + RED * FEAT + RED, ca + 2 * RED * FEAT + RED, RED, m->cws, st))
                return -1;
            x = m->cur;
        }
        // ResidualGroup (:182-194): body's closing ConvNorm + the group input, ping-ponged between g[0] / g[1]
        float* gout = m->g[gi & 1];
        if (conv(m->gconv[gi], m->cur, FEAT, m, N, gout, 0, gin, st)) return -1;
        gin = gout;
    }
    // res += x (the head output), then tailConv into t1
    {
        const long total4 = (long)N * hw * FEAT / 4;
        TraceScope ts("cain_add_head", st);
        ca_apply_kernel<<<(unsigned)std::min<long>((total4 + 255) / 256, 8192), 256, 0, st>>>(gin, nullptr, m->x0, m->cur, hw * FEAT / 4, FEAT / 4,
                                                                                            total4);
        VFI_CHECK_HIP(hipGetLastError());
    }
    if (conv(m->tail, m->cur, FEAT, m, N, m->t1, 0, nullptr, st)) return -1;
    return vfi_cain_frame_out(m->t1, m->means, out_dev, N, H, W, st);
}

}  // extern "C"
