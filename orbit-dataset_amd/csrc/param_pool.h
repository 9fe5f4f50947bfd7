// The parameter pool of a native handle (orbit_extractor, orbit_vit, orbit_filmgen): every tensor of the model at a fixed,
// aligned offset of ONE device allocation, filled by key from host or device memory or, all tensors at once, by one gather
// launch from a table of device pointers. The kernels of a plan read parameters as pool + offset; offsets are final once the
// plan is built, so a plan can be enumerated (keys, sizes) on a host without a GPU.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>
#include "common.h"

namespace orbit {

struct ParamPool {
    struct Param {
        std::string key;
        size_t numel = 0, off = 0;  // offset (floats) into the pool
        bool loaded = false;
    };
    // align: every tensor starts at a multiple of `align` floats (4: float4 loads of packed layouts; 64: 256-byte rows)
    explicit ParamPool(size_t align_floats) : align(align_floats) {}

    const size_t align;
    std::string owner;  // model name, for the "unexpected key" message
    std::vector<Param> params;
    std::unordered_map<std::string, int> index;
    size_t pool_floats = 0;
    float* d_pool = nullptr;
    // load_all_async: device table of source pointers + its host shadow, and the static table of (offset, numel) per tensor
    const float** d_src = nullptr;
    size_t* d_meta = nullptr;  // [n][2]
    std::vector<const float*> h_src;

    int add(const std::string& key, size_t numel) {
        Param p;
        p.key = key, p.numel = numel, p.off = pool_floats;
        pool_floats += (numel + align - 1) / align * align;
        params.push_back(p);
        index[key] = (int)params.size() - 1;
        return (int)params.size() - 1;
    }
    int find(const std::string& key) const {
        auto it = index.find(key);
        return it == index.end() ? -1 : it->second;
    }
    int size() const { return (int)params.size(); }
    size_t off(int i) const { return params[i].off; }
    float* ptr(int i) const { return d_pool + params[i].off; }
    const char* name(int i) const { return (i >= 0 && i < size()) ? params[i].key.c_str() : nullptr; }
    size_t numel(int i) const { return (i >= 0 && i < size()) ? params[i].numel : 0; }
    bool all_loaded(const char** missing) const {
        for (const Param& p : params)
            if (!p.loaded) {
                *missing = p.key.c_str();
                return false;
            }
        return true;
    }

    // the device side is created on first use (csrc/param_pool.hip); `who` prefixes the error text ("extractor_load", ...)
    int ensure_device();  // allocates the pool, zero-filled (the alignment gaps are read by float4 loads)
    void free_device();
    int load(const char* who, const char* key, const float* data, size_t numel);  // host or device memory, synchronous
    int load_async(const char* who, const char* key, const float* device_data, size_t numel, hipStream_t s);
    // every tensor in one launch of grid (chunks, n); ptrs[i] is the device tensor of parameter i
    int load_all_async(const char* who, const float* const* ptrs, int n, int chunks, hipStream_t s);
};

}  // namespace orbit
