// What the whole-network objects (vfi_film, vfi_m2m, vfi_cain, vfi_sepconvnet, vfi_flavr) share: the checkpoint cursor of their create
// functions, the workspace that owns their activations, and the base that owns their layers and device parameter blocks.  A net keeps
// what is its own: the layer table, weight re-layouts, ensure_workspace's size arithmetic and the forward sequence.
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

}  // namespace vfi
