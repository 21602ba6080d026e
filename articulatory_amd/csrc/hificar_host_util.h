// Host-side scaffolding every native handle shares (host C++ only; it sees no HIP type it is not handed):
//   Carver           carves a caller's workspace / tape into buffers, or sizes it (null base)
//   WeightIntake     set_weight's staging: the expected shapes, the staged host tensors, the two refusals, finalize's missing-key check
//   TapTable         the debug taps' name -> (destination, capacity) table and its capacity refusal
//   check_workspace  the alignment and size refusals of a workspace argument
//   launch_conv1     launch_conv for one layer and one ConvIO
//   pack_linear      a Linear's (out, in) weight and bias from a WeightIntake into a one-tap ConvLayer
// The includer defines fail(code, fmt, ...) (the thread's last-error text) ahead of this header; launch_conv1 and pack_linear are templates
// over the includer's engine / layer types and call its launch_conv / xfmr_pack.
#pragma once

#include "../../include/hificar.h"

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

static int fail(int code, const char* fmt, ...);

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

using FeatureShapes = std::map<std::string, std::vector<int64_t>>;  // a handle's expected tensors: state_dict name -> shape

// A bump allocator over a caller's buffer: every take starts on a multiple of `granule` bytes from base (base itself is the caller's to
// align).  With a null base every pointer is null and bytes() sizes the buffer: one planner serves the size query and the carving.
// A buffer that is not taken costs nothing; its planner leaves the pointer null.
class Carver {
public:
    Carver(void* base, size_t granule) : base_(static_cast<char*>(base)), granule_(granule) {}
    // byte offset of the next `bytes` bytes
    size_t take_at(size_t bytes) {
        const size_t at = off_;
        off_ += (bytes + granule_ - 1) / granule_ * granule_;
        return at;
    }
    template <class T>
    T* take(size_t bytes) {
        const size_t at = take_at(bytes);
        return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
    }
    // a buffer of `elems` floats — or of that many 4-byte elements seen as T (split rows are char*)
    template <class T = float>
    T* floats(size_t elems) {
        return take<T>(elems * sizeof(float));
    }
    // offset IN FLOATS of the next `elems` floats (the planners that hand out offsets into a float workspace; granule a multiple of 4)
    size_t floats_at(size_t elems) { return take_at(elems * sizeof(float)) / sizeof(float); }
    size_t bytes() const { return off_; }

private:
    char* base_;
    size_t granule_, off_ = 0;
};

// What a handle knows of its weights between create and finalize.  `expected` stays after finalize (the training entry points and
// feature_upload go by it); `tensors` are the host copies set() staged, dropped by clear_staged() once they are packed.
struct WeightIntake {
    FeatureShapes expected;
    std::map<std::string, HostTensor> tensors;

    // the body of every hificar_*_set_weight behind its own null-argument and after-finalize refusals; a second set of a name replaces the first
    int set(const char* name, const float* data, const int64_t* shape, int ndim) {
        auto it = expected.find(name);
        if (it == expected.end()) return fail(HIFICAR_E_INVALID, "unexpected tensor name '%s' for this configuration", name);
        std::vector<int64_t> s(shape, shape + ndim);
        if (s != it->second) {
            std::string want, got;
            for (auto v : it->second) want += std::to_string(v) + ",";
            for (auto v : s) got += std::to_string(v) + ",";
            return fail(HIFICAR_E_INVALID, "size mismatch for %s: expected (%s) got (%s)", name, want.c_str(), got.c_str());
        }
        size_t n = 1;
        for (auto v : s) n *= (size_t)v;
        HostTensor t;
        t.shape = s;
        t.data.assign(data, data + n);
        tensors[name] = std::move(t);
        return HIFICAR_OK;
    }
    // the first expected name (in the map's order) that was not set, or null
    const std::string* first_missing() const {
        for (auto& kv : expected)
            if (!tensors.count(kv.first)) return &kv.first;
        return nullptr;
    }
    // finalize's refusal of an incomplete state_dict
    int check_complete() const {
        const std::string* k = first_missing();
        return k ? fail(HIFICAR_E_STATE, "Missing key(s) in state_dict: \"%s\"", k->c_str()) : HIFICAR_OK;
    }
    const HostTensor& at(const std::string& name) const { return tensors.at(name); }
    const std::vector<float>& data(const std::string& name) const { return tensors.at(name).data; }
    void clear_staged() { tensors.clear(); }
};

// The debug taps of a handle (hificar_*_debug_tap): the copy itself and a model's own refusals stay with the model.
class TapTable {
public:
    // name null: forget all; dst null: forget one; otherwise the next forwards copy `name` into dst (capacity in floats)
    void set(const char* name, float* dst, size_t capacity) {
        if (!name) taps_.clear();
        else if (!dst) taps_.erase(name);
        else taps_[name] = {dst, capacity};
    }
    bool wanted(const std::string& name) const { return taps_.count(name) != 0; }
    bool empty() const { return taps_.empty(); }
    // whether any tapped name contains `part`
    bool any_contains(const char* part) const {
        for (auto& kv : taps_)
            if (kv.first.find(part) != std::string::npos) return true;
        return false;
    }
    // *dst: the tap's destination, or null when `name` is not tapped; refused when its buffer holds fewer than `need` floats
    int find(const std::string& name, size_t need, float** dst) const {
        *dst = nullptr;
        auto it = taps_.find(name);
        if (it == taps_.end()) return HIFICAR_OK;
        if (it->second.cap < need) return fail(HIFICAR_E_INVALID, "debug tap '%s' needs %zu floats, buffer has %zu", name.c_str(), need, it->second.cap);
        *dst = it->second.dst;
        return HIFICAR_OK;
    }

private:
    struct Tap {
        float* dst;
        size_t cap;
    };
    std::map<std::string, Tap> taps_;
};

// "<what>: " in front of a refusal (what null: none)
static inline std::string refusal_prefix(const char* what) { return what ? std::string(what) + ": " : std::string(); }

static inline int check_workspace_size(const char* what, size_t have, size_t need) {
    if (have < need) return fail(HIFICAR_E_WORKSPACE, "%sworkspace too small: %zu < %zu", refusal_prefix(what).c_str(), have, need);
    return HIFICAR_OK;
}

// a workspace argument: a 256-byte aligned pointer to at least `need` bytes
static inline int check_workspace(const char* what, const void* ptr, size_t have, size_t need) {
    if (!ptr || reinterpret_cast<uintptr_t>(ptr) % 256)
        return fail(HIFICAR_E_INVALID, "%sworkspace must be a 256-byte aligned device pointer", refusal_prefix(what).c_str());
    return check_workspace_size(what, have, need);
}

// launch_conv of one layer and one ConvIO; tail: slope_out, the ragged context, the stream and, for a grouped conv, its ConvRep.  The layer goes
// by reference and is never copied: launch plans are keyed by the layers' addresses.
template <class Engine, class Layer, class IO, class... Tail>
static int launch_conv1(Engine* h, const Layer& layer, int nseq, int rows, const IO& io, const Tail&... tail) {
    const Layer* ls[1] = {&layer};
    return launch_conv(h, ls, 1, nseq, rows, &io, tail...);
}

// torch.nn.Linear `name` of the intake ((out, in) weight, bias) as the one-tap conv L, in the engine's arithmetic (xfmr_pack)
template <class Engine, class Layer>
static int pack_linear(Engine* h, Layer& L, const WeightIntake& w, const std::string& name) {
    HostTensor W = w.at(name + ".weight");
    W.shape.push_back(1);
    return xfmr_pack(h, L, W, &w.data(name + ".bias"));
}
