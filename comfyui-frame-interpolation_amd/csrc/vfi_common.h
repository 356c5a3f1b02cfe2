// Internal helpers shared by the HIP translation units of libvfi_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "conv_large.h"

namespace vfi {

void set_error(const char* fmt, ...);
const char* get_error();

#define VFI_CHECK_HIP(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::vfi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                             __LINE__);                                                       \
            return -1;                                                                        \
        }                                                                                     \
    } while (0)

#define VFI_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            ::vfi::set_error(__VA_ARGS__); \
            return -2;                  \
        }                               \
    } while (0)

// ---- per-kernel event tracing ---------------------------------------------------------
bool trace_on();
void trace_begin(const char* name, hipStream_t s);
void trace_end(hipStream_t s);

struct TraceScope {
    hipStream_t s;
    bool on;
    TraceScope(const char* name, hipStream_t st) : s(st), on(trace_on()) {
        if (on) trace_begin(name, s);
    }
    ~TraceScope() {
        if (on) trace_end(s);
    }
};

// ---- shader-clock probe (vfi_clock_probe) -------------------------------------------------------------------------------------
// While a probe buffer is installed, every launch of the Winograd kernel takes one record (8 x u64, conv_wino.hip): workgroup 0 stamps
// s_memtime (shader cycles) and s_memrealtime (constant-rate counter) when it starts and when it ends.  The ratio of the two deltas is
// the clock the chip actually sustained while THIS kernel ran (it clocks to its power budget: 1.9-2.3 GHz under MFMA load,
// MI355X_MICROARCH.md "DVFS give-back").  clock_probe_tag: the host's index of the launch (its trace name is kept under it), -1 = off.
int clock_probe_tag(const char* name);
int clock_probe_install(unsigned long long* dev_records, int capacity);      // conv_wino.hip: the device-side state, current device
int wino_probe_read(unsigned* out32);                                         // conv_wino.hip: [4][8] stamp sums of the last probed launch

// ---- A/B options of tools/ and tests/ (include/vfi_hip_test.h: vfi_test_set_option) ----------------------------------------
// Every option selects between two CORRECT forms of a kernel or launch (fused / unfused, tile variant, ...).  They are set through
// the test C entry point only — the product library reads NO experiment switch from the environment, so a stray variable cannot
// change a frame (tests/test_gpu_env_hygiene.py).  Values are read at every launch (one relaxed atomic load).
enum Option {
    kOptStageQuad,       // bit mask of the next-block scales (2, 4, 8) whose transition takes the quad kernel (default 14 = all)
    kOptFuseEncode,      // 1: RIFE 4.7 frame pack in one launch (default), 0: prep + encode.0 + encode.1 as three kernels
    kOptFuse0a,          // 1: block 2->3 transition fused with block 3's conv0.0 (default), 0: separate, 2: fused, all 24 padded input channels multiplied
    kOptM2n2Px,          // pixel count from which wide direct-conv layers take the m2n2 tile (default -1 = never)
    kOptGroupedVariant,  // forced tile variant of the grouped (transposed) convolution (default -1 = heuristic)
    kOptSplitK,          // 1: split-K allowed for layer objects (default), 0: never
    kOptSplatAtomic,     // 1: force the LDS-atomic splat kernel, 3: staged list gather with compaction for C == 4 (default 0: list-gather kernel with the atomic kernel as overflow fallback)
    kOptSplatSpillCap,   // spill-list capacity of the list-gather splat (default -1 = built-in)
    kOptWinoXcd,         // 1: XCD-aware work order of the Winograd kernel (default), 0: plain order
    kOptDeconvWino,      // 1: ConvTranspose2d(4, 2, 1) + PixelShuffle (RIFE lastconv) as a 96-channel 3x3 layer on the Winograd kernel (default), 0: grouped direct kernel
    kOptEncodeBatched,   // 1: one frame-pack launch for a batch of frames where the caller offers one (default), 0: one launch per frame
    kOptWinoQuant,       // 1: layer objects leave launches of <= 2 rounds with a nearly empty last round to the direct kernel (default), 0: item count only
    kOptXcdBands,        // 1: XCD-aware workgroup order of the RIFE gather kernels (final blend, quad transitions), 0: plain order (default: r6 A/B measured the banded order 2-5 % SLOWER, profiles/r06_xcd_bands_ab.txt)
    kOptM2mFused,        // 1: M2M render as one kernel (m2m_render.hip; default), 0: splat inputs + summation splat + combine as separate launches
    kOptM2mSide,         // 1: M2M prepare runs the image-pyramid convolutions (EncDec's c features) on a side stream beside the PWC flow network, 0: one stream (default: r6 A/B measured the fork neutral on one pair — 7.00-7.04 vs 7.0-7.1 ms — and 8 % SLOWER under three pair lanes)
    kOptFilmSide,        // 1: FILM forward runs image 1's feature extraction and the backward flow pyramid on a side stream (another hardware queue) beside image 0's / the forward one, 0: one stream
    kOptWinoProbe,       // 1..4: the hot Winograd instantiation takes its cycle-ledger form (conv_wino.hip: g_wino_probe_out; default 0)
    kOptSepconvSplitHeads,  // 1: SepConv++'s four head first-convs as four 64 -> 64 layers, each reading up2(row1) (default 0: one 64 -> 256 layer)
    kOptSepconvPlanar,      // 1: SepConv++'s heads transposed to planar before the output stage (default), 0: the output stage reads them NHWC
    kOptStage0,             // 1: RIFE block 0's input assembled from the per-frame staging images the frame pack kernels write (default), 0: gathered from the packs per pair
    kOptAttKsplit,          // 1..8: the number of key ranges attention_launch_t asks for (attention.hip; reduced so that no range is empty), default 0: chosen from the device's CU count
    kOptWinoDead,           // 1: the Winograd kernel skips the transform planes a transposed-convolution layer's weights leave zero (ConvArgs::wino_dead; default), 0: all 16 planes: same bits
    kOptLargeBytes,         // bytes of one image from which a layer object's operand counts as large and the launch takes the per-tile / per-region descriptors (conv_mfma2.hip, conv_wino.hip: LARGE); default 2^31 - 1, lower values put small images on that path: same bits
    kOptSepconvBandRows,    // SepConv++'s head stage: 0 = automatic (whole frame up to 2 097 151 padded pixels, bands of the default height above, csrc/sepconv_bands.h), n > 0 = bands of n rows at any frame size: same bits
    kOptFuse0a2,            // 1: RIFE's block 1->2 transition fused with block 2's conv0.0 (rife_ops.hip: trans2_conv0a_kernel; default), 0: stage_trans2 + conv0a_b2 as two kernels, 2: fused with one workgroup per CU instead of two: same bits
    kOptCount
};
long option(Option o);
// a new stream that the runtime has bound to another hardware queue than `st` (decided by measurement with vfi_stream_spin; util.hip)
hipStream_t stream_apart_from(hipStream_t st);
void stream_give_back(hipStream_t side);      // to the idle list stream_apart_from draws its candidates from (never destroyed)
int option_set(const char* name, long value);      // 0, or -2 for an unknown name
int variant_override(const char* trace_name);      // tile variant forced for a trace name (vfi_test_variant_override), -1 = none
// What the calling thread's last convolution launch was (vfi_test_last_conv_launch): written by the host-side launchers launch_t,
// launch2_e and wino_launch_t.  Stores under VFI_TEST_TAPS only; in the product library both are empty functions.
//   family 1 / 2 = first / second generation direct kernel, 3 = Winograd;  form: direct 0 plain, 1 EXT, 2 MASKED, 3 LARGE; Winograd MODE;
//   store: out_mode (direct) / SHUF (Winograd; 3 = the LARGE form, whose store is SHUF 0's; 5 = 3 + 2, the LARGE form of SHUF 2, the transposed convolution);  ks: split-K slices (1 = unsplit);  work: tiles (direct) / work items (Winograd)
enum { kConvFamilyGen1 = 1, kConvFamilyGen2 = 2, kConvFamilyWino = 3 };
enum { kWinoStoreLargeDeconv = 5 };
void conv_record_variant(int variant);      // conv_launch: the direct variant id in the common numbering, kept for the launcher's record
void conv_record_launch(int family, int wino_region, int form, int store, int ks, long grid_x, long work);   // wino_region: 8 / 16, direct: 0
int conv_record_read(int32_t* out, int cap);
struct ConvArgs;
void conv_record_large(int family, const ConvArgs& a);      // a LARGE-form launch, kept in a per-thread log (vfi_test_large_launches); empty in the product library
int conv_large_log_read(int32_t* out, int cap_entries);    // entries of 6 ints (family, Hin, Win, in_cs, Cin_p, Cout); reading empties the log

// Compute units the persistent kernels may size their grids for: the device's count minus what vfi_set_reserved_cus holds back for a
// collective kernel running beside them (a resident RCCL kernel takes whole CUs from one-workgroup-per-CU kernels, whose displaced
// workgroups then run as a second round: +37 % while it is resident, profiles/r04_reserved_cus.txt).  A multiple of 8 (XCDs), >= 8.
int launch_cus(int device_cus);

// the 4-channel summation splat on the staged list-gather machinery of m2m_render.hip (round 6): in / out [N,H,W,4], flow [N,H,W,2]
int softsplat4_launch(const float* in, const float* flow, float* out, int N, int H, int W, hipStream_t s);

constexpr int kMaxDevices = 16;   // devices one process may drive (per-device caches are indexed by the HIP device id)

// Row / column read for halo index i of an n-pixel image in pad_mode 1 (replicate) or 2 (reflect: -1 -> 1, n -> n - 2, as
// torch.nn.ReflectionPad2d(1); needs n >= 2).  The result is clamped into [0, n) in both modes: halo pixels of tiles that hang over
// the image's end (whose outputs are never stored) must still read inside it.
__host__ __device__ __forceinline__ int pad_index(int i, int n, int mode) {
    if (mode == 2) i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
    return min(max(i, 0), n - 1);
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return cdiv(a, b) * b; }

// ---- convolution on the fp32 matrix cores -----------------------------------------------
// A convolution "group" is a set of taps sharing one weight block; a plain 3x3 conv has one
// group of 9 taps, the 4x4/stride-2 transposed conv has 4 groups (output parities) of 4 taps.
struct ConvArgs {
    const float* in;    // [N,Hin,Win,in_cs] (channels >= Cin_p readable, zero beyond Cin)
    const float* w;     // packed [group][tap][Cin_p/8][Cout_p][8]
    const float* bias;  // [group][Cout_p]
    const float* beta;  // [Cout_p] or nullptr       y = act((conv+bias)*beta + res)
    const float* res;   // [N,Hout,Wout,res_cs] or nullptr
    float* out;         // [N,Hout,Wout,out_cs]; group g writes channels [g*Cout_p, g*Cout_p+Cout)
    int N, Hin, Win, in_cs;
    int Hout, Wout, out_cs, res_cs;
    int Cin_p, Cout_p, Cout;
    int ntaps;
    int act;      // 0 none, 1 leaky relu(slope), 2 clamp to [0,1], 3 PReLU per channel (prelu[]), 4 sigmoid
    float slope;
    int tiles_x, tiles_y;  // output tiles per image (filled by the launcher)
    int tap_y0, tap_x0;    // origin of the tap rectangle (3x3: -1,-1), ignored for grouped
    int in_plane;          // 0: input is NHWC [.,.,in_cs]; >0: planar4 input, floats between 4-channel planes
                           //    (image = in_cs/4 planes of [Hin][Win][4])
    int out_mode;          // 0: NHWC store; 1 (grouped only): PixelShuffle(2) of the transposed conv, planar4
                           //    [N][2][4*Hout][4*Wout][4] (channel c of Cout/4 -> plane c/4, component c%4);
                           //    2 (grouped only): plain transposed-conv output, NHWC [N][2*Hout][2*Wout][out_cs]
    int out_planes;        // out_mode 1: planes per image of the planar4 output (0 = 2)
    int pad_mode;          // 0: zero padding; 1: replicate (edge clamp); 2: reflect (ReflectionPad2d(1)) padding of the input
    const float* prelu;    // [Cout_p] per-channel negative slopes (act == 3)
    float post_scale, post_shift;  // y = act(...) * post_scale + post_shift  (post_scale == 0 means "not set" = 1, 0)
    int split_ok;          // caller: the launcher may cut K over several workgroups (split-K; generic layer objects only — the
                           //   RIFE network keeps one kernel per layer whatever the batch, so results do not depend on batching)
    short huge_ok;         // host side only: the layer object's permission (vfi_conv_allow_huge) — the LARGE forms may serve operand images of 4 GiB
                           //   and more, up to kConvHugeMaxFloats floats (conv_large.h); 0 = refused from 4 GiB on.  It sits in the four bytes of
                           //   padding in front of the pointer below, so that no kernel argument moved when it was added (static_assert below)
    short res_prelu_ok;    // host side only, the other half of those four bytes: the layer object's permission vfi_conv_allow_large_res_prelu — a 3x3
                           //   stride-1 layer with a residual and per-channel PReLU (act 3) may take its LARGE form; 0 = it keeps the plain form and
                           //   its 2 GiB refusal
    const unsigned char* tapmask;  // 2x2 layers in the "up-sample x2 first" form (conv_mfma2.hip, MASKED): per 64-channel N block the taps (bit a * 2 + b) of
    int par_cout;                  //   its parity; par_cout = channels per parity group (4 groups: Cout_p == 4 * par_cout), output [2 Hout, 2 Wout] interleaved
    int ksplit;            // set by the launcher: > 1 = split-K launch, blockIdx.z owns a K range and the slice
    long split_stride;     //   out + blockIdx.z * split_stride (floats) of the partial-sum workspace
    int cin_live;          // the layer's real input channels where the caller knows them (0 = not given: all Cin_p are multiplied); last, so
                           //   that the kernels' argument offsets of the fields above are what they were
    unsigned wino_dead[4]; // Winograd kernel, transposed-convolution layers (out_mode 1 / 2): the zero transform planes of each 32-channel N
                           //   block, 4 bits per block (kWinoDead*, block nb = bits 4 (nb % 8) of word nb / 8), from WinoDeconvPack; 0 = none known
    int wino_gray;         //   1: the four parity groups of such a layer are packed in the order p00 p01 p11 p10 (wino_gray_order)
};

static_assert(sizeof(ConvArgs) == 208 && offsetof(ConvArgs, tapmask) == 160 && offsetof(ConvArgs, huge_ok) == 156 && offsetof(ConvArgs, res_prelu_ok) == 158, "ConvArgs: the kernels' argument offsets are part of their code");

struct ConvVariant {
    const char* name;
    int stride, taps, mt, nt, wm, wn, ck, grouped;
};
// Variant ids: 0.. = first generation (conv_mfma.hip, weights in registers),
// kConv2Base.. = second generation (conv_mfma2.hip, both operands through LDS-DMA).
constexpr int kConv2Base = 32;
int conv_num_variants();
const ConvVariant& conv_variant(int i);
int conv2_num_variants();
const ConvVariant& conv2_variant(int i);
int conv2_launch(const ConvArgs& a, int idx, hipStream_t s, const char* trace_name);
const ConvVariant* conv_variant_lookup(int id);
// Launch; variant < 0 selects by heuristic.  grouped convs must use a grouped variant.
int conv_pick_variant(const ConvArgs& a, int stride, bool grouped);
int conv_launch(const ConvArgs& a, int stride, bool grouped, int variant, hipStream_t s,
                const char* trace_name);

// Host-side weight packing.  w_oihw: [Cout][Cin][3][3] -> packed (1 group, 9 taps).
void pack_conv3x3(const float* w_oihw, const float* bias, int Cout, int Cin, int Cin_p,
                  int Cout_p, std::vector<float>& wp, std::vector<float>& bp);
// w_iohw: [Cin][Cout][4][4] (ConvTranspose2d, stride 2, pad 1) -> 4 groups x 4 taps, Cout_p = 32k.
void pack_deconv4x4(const float* w_iohw, const float* bias, int Cin, int Cout, int Cin_p,
                    int Cout_p, std::vector<float>& wp, std::vector<float>& bp);
void conv3x3_taps(ConvArgs& a);

// ---- Winograd F(2x2,3x3) form of the 3x3 stride-1 convolution (conv_wino.hip) ------------------------------------------------
// Weights: U = G g G^T, packed [Cout_p/32][Cin_p/8][j][xi/4][half][co%32][xi%4] (16 * Cin_p * Cout_p floats); chan_map translates
// logical to physical input channels (nullptr = identity).  Launch: ConvArgs as for the direct kernel with a.w = that pack;
// variant 0 = pick the region shape, 8 / 16 = 16x8 / 32x4 output pixels per wave.
void pack_wino3x3(const float* w_oihw, int Cout, int Cin, const int* chan_map, int Cin_p, int Cout_p, std::vector<float>& wp);
void pack_deconv_as_conv3x3(const float* w_iohw, const float* bias, int Cin, int LO, std::vector<float>& w3, std::vector<float>& b3);
// The transform planes of each 32-channel N block of a pack_wino3x3 image that hold nothing but zeros, as one form per block: a form is
// reported only when EVERY packed weight of that plane row / column of the block compares == 0.0f (a NaN or a padded channel beside
// live ones keeps its plane alive), a row before a column (a row also saves transform work).  forms[Cout_p / 32].
enum { kWinoDeadNone = 0, kWinoDeadRow0 = 1, kWinoDeadRow3 = 2, kWinoDeadCol0 = 3, kWinoDeadCol3 = 4 };
void wino_dead_forms(const float* wp, int Cin_p, int Cout_p, std::vector<int>& forms);
int wino_dead_planes(const std::vector<int>& forms);      // planes the forms skip (4 per block with one)
// N position co of a 4 * LO-channel transposed-convolution layer -> the row of pack_deconv_as_conv3x3's w3 / b3 that sits there when the
// parity groups are ordered p00 p01 p11 p10 (consecutive groups share py or px, so a 32-channel block that spans two of them keeps a
// dead plane row or column); the Winograd epilogue inverts it (g ^= g >> 1).  The map is its own inverse.
inline int wino_gray_order(int co, int LO) {
    const int g = co / LO;
    return (g ^ (g >> 1)) * LO + co % LO;
}
// A ConvTranspose2d(Cin, LO, 4, 2, 1) layer ready for the Winograd kernel: pack_deconv_as_conv3x3 + (where it raises the number of
// skipped planes) the Gray order + pack_wino3x3 + the dead-plane table.  bias3 / prelu3 [Cout3_p] are the per-channel constants
// repeated per parity group in the SAME order (prelu3 empty without slopes).  apply() hands table and order to a launch.
struct WinoDeconvPack {
    std::vector<float> ww, bias3, prelu3;
    int Cout3_p = 0, gray = 0;
    unsigned dead[4] = {0, 0, 0, 0};
    void apply(ConvArgs& a) const {
        for (int i = 0; i < 4; ++i) a.wino_dead[i] = dead[i];
        a.wino_gray = gray;
    }
};
void pack_deconv_wino(const float* w_iohw, const float* bias, const float* prelu, int Cin, int LO, const int* chan_map, int Cin_p, WinoDeconvPack& out);
bool conv_wino_eligible(const ConvArgs& a);
// Large images (2 GiB <= one image's bytes < 4 GiB; with ConvArgs::huge_ok up to kConvHugeMaxFloats floats, conv_large.h): the direct kernel
// addresses its output and residual with 64 bits in every form, so only its input decides; the Winograd kernel goes through descriptors on
// all three.
inline bool conv_bytes_large(long bytes) { return bytes >= option(kOptLargeBytes); }
inline bool conv_input_large(const ConvArgs& a) { return conv_bytes_large((long)a.Hin * a.Win * a.in_cs * 4); }
int conv_wino_mode(int set);      // set < 0: query.  0 automatic, 1 direct kernel only, 2 Winograd wherever legal, 3 as 2 with 32x4 regions wherever the
                                  //   launcher would pick the region shape.  Process state that only the test hook vfi_test_conv_algo sets (the product library has no
                                  //   setter, so it stays 0 there); conv_wino_eligible and conv_wino_launch read it on every launch, one relaxed atomic load
// A layer call that computes a horizontal BAND of a frame (csrc/sepconv_net.hip) must take the kernel and the tile the whole-frame call
// would take, or the band's bits differ from the frame's (the two kernels sum in different orders): while rows > 0 on the calling thread,
// conv_wino_eligible and conv_pick_variant size a stride-1 layer's choice by `rows` image rows instead of the call's own.  0 (default) = the
// call's own rows; set < 0 queries.  Returns the value in force before the call.
int conv_decide_rows(int set);
struct ConvDecideRows {      // scope guard
    int before;
    explicit ConvDecideRows(int rows) : before(conv_decide_rows(rows)) {}
    ~ConvDecideRows() { conv_decide_rows(before); }
    ConvDecideRows(const ConvDecideRows&) = delete;
    ConvDecideRows& operator=(const ConvDecideRows&) = delete;
};
int conv_wino_launch(const ConvArgs& a, int variant, hipStream_t s, const char* trace_name);
void deconv4x4_taps(ConvArgs& a);

int conv_naive_launch(const float* in, const float* w_oihw_dev, const float* bias_dev,
                      const float* beta_dev, float* out, int N, int H, int W, int Cin, int in_cs,
                      int Cout, int stride, int act, float slope, hipStream_t s);

}  // namespace vfi
