// What the whole-network objects share.  All eight (vfi_film, vfi_m2m, vfi_cain, vfi_sepconvnet, vfi_flavr, vfi_amt, vfi_atm, vfi_xvfi): the
// checkpoint cursor and layer reader of their create functions, the workspace that owns their activations, and the base that owns their
// layers and device parameter blocks.  The three whose activations are all named scratch tensors (AMT, ATM, XVFI) also share the run
// context of a forward call, the frame-pair pad and the entry guard of a padded net.  A net keeps what is its own: the layer table, weight
// re-layouts, its size arithmetic and the forward sequence.
#pragma once
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/vfi_hip.h"
#include "vfi_common.h"

// internal to the library: nothing here (nor a template instantiated over it) is exported
#define VFI_INTERNAL __attribute__((visibility("hidden")))

namespace vfi {

inline int r8(int c) { return (c + 7) & ~7; }      // channel counts are padded to multiples of 8
inline int nblk(long n, int per) { return (int)((n + per - 1) / per); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// returns early on a failed launch or layer call
#define VFI_DO(x)          \
    do {                   \
        if (x) return -1;  \
    } while (0)

struct VFI_INTERNAL Ten {   // [n][h][w][c] fp32
    float* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
};

// Every activation buffer of one object.  All or nothing: a failed allocation releases the whole workspace, so a net never sees a
// half-built one — ensure_workspace asks live() beside its own shape key and never resets that key itself.
class VFI_INTERNAL Workspace {
public:
    enum Fill { kNoFill, kZero };

    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    ~Workspace() { (void)release(); }

    // Zero fills are ordered with the forward's kernels: a NULL-stream memset is not ordered against a non-blocking side stream (torch's)
    // and could clear a lazily allocated scratch tensor AFTER its first producer ran, so a fill on the null stream is waited for.
    int alloc(float** p, size_t floats, Fill fill, hipStream_t st) {
        const size_t bytes = floats * sizeof(float);
        *p = nullptr;
        hipError_t e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) {
            owned_.push_back(*p);
            bytes_ += (int64_t)bytes;
            if (fill == kZero) {
                e = hipMemsetAsync(*p, 0, bytes, st);
                if (e == hipSuccess && !st) e = hipStreamSynchronize(nullptr);
            }
        }
        if (e != hipSuccess) {
            *p = nullptr;
            (void)release();
            set_error("workspace allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
            return -1;
        }
        return 0;
    }

    // a zero-initialised tensor (padded channel positions and borders must hold finite values)
    int ten(Ten& t, int n, int h, int w, int c, hipStream_t st) {
        t.n = n, t.h = h, t.w = w, t.c = c;
        return alloc(&t.p, (size_t)n * h * w * c, kZero, st);
    }

    // scratch tensor `name` of this size, allocated at its first use
    int tmp(const char* name, int n, int h, int w, int c, Ten** out) {
        auto key = std::make_tuple(std::string(name), h, w, c);
        auto it = scratch_.find(key);
        if (it == scratch_.end()) {
            Ten t;
            if (ten(t, n, h, w, c, nullptr)) return -1;
            it = scratch_.emplace(key, t).first;
        }
        *out = &it->second;
        return 0;
    }

    // kernels of the last forward may still read the buffers: the device is drained first
    int release() {
        if (owned_.empty()) return 0;
        const hipError_t e = hipDeviceSynchronize();
        for (float* p : owned_) (void)hipFree(p);
        owned_.clear();
        scratch_.clear();
        bytes_ = 0;
        if (e != hipSuccess) {
            set_error("hipDeviceSynchronize failed before the workspace was freed: %s", hipGetErrorString(e));
            return -1;
        }
        return 0;
    }

    int64_t bytes() const { return bytes_; }
    bool live() const { return !owned_.empty(); }

private:
    std::vector<float*> owned_;
    std::map<std::tuple<std::string, int, int, int>, Ten> scratch_;
    int64_t bytes_ = 0;
};

// The state_dict tensors of a create call, taken in order.  After the first failure every take returns nullptr without touching the arrays.
class VFI_INTERNAL TensorCursor {
public:
    TensorCursor(const float* const* tensors, const int64_t* numels, int n_tensors, const char* who)
        : tensors_(tensors), numels_(numels), n_(n_tensors), who_(who) {}

    const float* take(int64_t numel) {
        if (!ok_) return nullptr;
        if (k_ >= n_) set_error("%s: tensor %d asked for, only %d given", who_, k_, n_);
        else if (numels_[k_] != numel) set_error("%s: tensor %d has %lld elements, expected %lld", who_, k_, (long long)numels_[k_], (long long)numel);
        else if (!tensors_[k_]) set_error("%s: tensor %d is a null pointer", who_, k_);
        else return tensors_[k_++];
        ok_ = false;
        return nullptr;
    }
    float scalar() {   // a one-parameter PReLU slope, alpha
        const float* s = take(1);
        return s ? s[0] : 0.f;
    }
    bool ok() const { return ok_; }
    bool finish() {
        if (ok_ && k_ != n_) {
            set_error("%s: consumed %d of %d tensors", who_, k_, n_);
            ok_ = false;
        }
        return ok_;
    }

private:
    const float* const* tensors_;
    const int64_t* numels_;
    int n_, k_ = 0;
    const char* who_;
    bool ok_ = true;
};

// Base of the vfi_* network structs: the workspace, every created layer and every raw device parameter block.  Destruction frees all
// three, so a net's destroy function is its own streams and events, then `delete`.
struct VFI_INTERNAL NetObject {
    Workspace ws;
    std::vector<vfi_conv_t*> layers;
    std::vector<float*> params;
    bool failed = false;      // a layer or an upload could not be made (the error text is set): the create function gives up at its end

    NetObject() = default;
    NetObject(const NetObject&) = delete;
    NetObject& operator=(const NetObject&) = delete;

    vfi_conv_t* add_layer(vfi_conv_t* L) {
        if (L) layers.push_back(L);
        else failed = true;
        return L;
    }

    // The next layer of the checkpoint, as it is: Conv2d (kind 0) / ConvTranspose2d (kind 1) weights, then the bias and the per-channel
    // PReLU slopes where the layer has them.  map: logical -> physical input channels; cin_phys: the input's channel stride, r8(cin) if 0.
    vfi_conv_t* read_layer(TensorCursor& cur, int kind, int cout, int cin, int k, int stride, bool bias, bool prelu, const int* map = nullptr,
                           int cin_phys = 0) {
        const float* w = cur.take((int64_t)cout * cin * k * k);
        const float* b = bias ? cur.take(cout) : nullptr;
        const float* p = prelu ? cur.take(cout) : nullptr;
        if (!cur.ok()) return nullptr;
        return add_layer(vfi_conv_create_ex(kind, w, b, cout, cin, k, stride, 0, map, cin_phys ? cin_phys : r8(cin), p));
    }

    // device copy of src[0 .. floats); src == nullptr: the block is only allocated (a pack kernel fills it)
    float* upload(const float* src, size_t floats) {
        float* d = nullptr;
        hipError_t e = hipMalloc((void**)&d, floats * sizeof(float));
        if (e == hipSuccess) {
            params.push_back(d);
            if (src) e = hipMemcpy(d, src, floats * sizeof(float), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            set_error("device allocation/upload of a %zu-byte parameter block failed: %s", floats * sizeof(float), hipGetErrorString(e));
            failed = true;
            return nullptr;
        }
        return d;
    }

    ~NetObject() {
        (void)ws.release();
        for (vfi_conv_t* L : layers) vfi_conv_destroy(L);
        for (float* p : params) (void)hipFree(p);
    }
};

// ---- nets that pad a frame pair and keep every activation as a named scratch tensor (AMT, ATM, XVFI) ----------------------------------

// The layers index one image with 32 bits of bytes: the padded pixels a net may take whose widest buffer has px_floats floats per pixel.
inline int64_t max_padded_pixels(int px_floats) { return 0x7fffffffLL / (px_floats * 4); }
// ... and of a net whose layers all have a large-image form (conv_mfma2.hip / conv_wino.hip: LARGE), where one image stays below 4 GiB
inline int64_t max_padded_pixels_large(int px_floats) { return 0xffffffffLL / (px_floats * 4); }

// Base of such a net: the padded size is the key of its workspace.
struct VFI_INTERNAL PaddedNet : NetObject {
    int Hp = 0, Wp = 0;

    // The entry guard of a forward: an H x W frame padded to Hp x Wp is refused before any launch or allocation when it is over the size
    // limit; the workspace is released when the padded size (or the caller's own part of the key, `rekey`) changed; the key is stored.
    // who: the entry point, net: the model's name in the refusal.  large: the object serves images up to 4 GiB (max_padded_pixels_large).
    int enter(const char* who, const char* net, int H, int W, int Hp_, int Wp_, int px_floats, bool rekey = false, bool large = false) {
        VFI_REQUIRE(!large || (int64_t)Hp_ * Wp_ <= max_padded_pixels_large(px_floats),
                    "%s: a %dx%d frame (padded %dx%d) is over the size limit of %s with large frames on, %lld padded pixels: Hp * Wp * %d bytes must stay "
                    "below 4 GiB for the layers' index arithmetic", who, H, W, Hp_, Wp_, net, (long long)max_padded_pixels_large(px_floats), px_floats * 4);
        VFI_REQUIRE(large || (int64_t)Hp_ * Wp_ <= max_padded_pixels(px_floats),
                    "%s: a %dx%d frame (padded %dx%d) is over the size limit of %s, %lld padded pixels: Hp * Wp * %d bytes must stay below 2 GiB "
                    "for the layers' index arithmetic", who, H, W, Hp_, Wp_, net, (long long)max_padded_pixels(px_floats), px_floats * 4);
        if (ws.live() && (Hp != Hp_ || Wp != Wp_ || rekey) && ws.release()) return -1;
        Hp = Hp_, Wp = Wp_;
        return 0;
    }
};

// One forward call of such a net: the scratch tensors by name, the launches' stream and a sticky failure flag (a failed buf() makes every
// later one fail, so a run asks for several and tests `bad` once).  leaky: the slope of act 1 (0: a ReLU).  A net's Run derives from
// this and adds its own launches.
template <class Net>
struct VFI_INTERNAL NetRun {
    Net* m;
    hipStream_t st;
    float leaky = 0.f;
    bool bad = false;
    float* buf(const char* name, int n, int h, int w, int c) {
        Ten* t = nullptr;
        if (bad || m->ws.tmp(name, n, h, w, c, &t)) {
            bad = true;
            return nullptr;
        }
        return t->p;
    }
    int conv(const vfi_conv_t* L, const float* in, int ics, int h, int w, float* out, int ocs, int N, int act, const float* res = nullptr, int rcs = 0) {
        return vfi_conv_forward_ex(L, in, ics, h, w, out, ocs, N, act, act == 1 ? leaky : 0.f, 0.f, 0.f, res, rcs, st);
    }
};

// Both frames' channels 0..2 ([H,W,C>=3]) into img [2,Hp,Wp,8] with the frame at (top, left); the border repeats the frame's edge
// (replicate: InputPadder, AMT and ATM) or is zero (F.pad to the bottom / right with top = left = 0: XVFI).  gen_ops.hip.
VFI_INTERNAL int pad_frame_pair(const float* f0, const float* f1, int C, int H, int W, float* img, int Hp, int Wp, int top, int left, bool replicate,
                                hipStream_t st);

}  // namespace vfi
