// Parameter upload of the native handles (csrc/param_pool.h): the three ways a tensor reaches the pool.
#include "param_pool.h"

namespace orbit {

// one kernel copies every parameter tensor into the pool: grid (chunks, parameters)
__global__ __launch_bounds__(256) void gather_params_kernel(const float* const* __restrict__ src,
                                                            const size_t* __restrict__ meta, float* __restrict__ pool) {
    const float* s_ = src[blockIdx.y];
    float* d = pool + meta[2 * blockIdx.y];
    const size_t n = meta[2 * blockIdx.y + 1];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) d[i] = s_[i];
}

int ParamPool::ensure_device() {
    if (d_pool) return ORBIT_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_pool), pool_floats * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d_pool, 0, pool_floats * sizeof(float));
    if (e != hipSuccess) {
        free_device();
        (void)hipGetLastError();
        return set_err(ORBIT_ERR_HIP, "parameter pool: device allocation failed: %s", hipGetErrorString(e));
    }
    return ORBIT_OK;
}

void ParamPool::free_device() {
    (void)hipFree(d_pool);
    (void)hipFree(d_src);
    (void)hipFree(d_meta);
    d_pool = nullptr, d_src = nullptr, d_meta = nullptr;
    h_src.clear();
    for (Param& p : params) p.loaded = false;
}

// the checks every per-key load makes before it touches the device
static int find_param(ParamPool& pool, const char* who, const char* key, size_t numel, ParamPool::Param** out) {
    const int i = pool.find(key);
    ORBIT_REQUIRE(i >= 0, "%s: unexpected key '%s' for %s", who, key, pool.owner.c_str());
    ParamPool::Param& p = pool.params[i];
    ORBIT_REQUIRE(p.numel == numel, "%s: '%s' has %zu elements, expected %zu", who, key, numel, p.numel);
    *out = &p;
    return pool.ensure_device();
}

int ParamPool::load(const char* who, const char* key, const float* data, size_t numel) {
    Param* p;
    if (int rc = find_param(*this, who, key, numel, &p)) return rc;
    ORBIT_HIP_CHECK(hipMemcpy(d_pool + p->off, data, numel * sizeof(float), hipMemcpyDefault));
    p->loaded = true;
    return ORBIT_OK;
}

int ParamPool::load_async(const char* who, const char* key, const float* device_data, size_t numel, hipStream_t s) {
    Param* p;
    if (int rc = find_param(*this, who, key, numel, &p)) return rc;
    ORBIT_HIP_CHECK(hipMemcpyAsync(d_pool + p->off, device_data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    p->loaded = true;
    return ORBIT_OK;
}

int ParamPool::load_all_async(const char* who, const float* const* ptrs, int n, int chunks, hipStream_t s) {
    ORBIT_REQUIRE(n == size(), "%s: %d pointers for %zu parameters", who, n, params.size());
    if (int rc = ensure_device()) return rc;
    if (!d_src) {
        ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_src), n * sizeof(float*)));
        ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_meta), 2 * n * sizeof(size_t)));
        std::vector<size_t> meta(2 * n);
        for (int i = 0; i < n; ++i) meta[2 * i] = params[i].off, meta[2 * i + 1] = params[i].numel;
        ORBIT_HIP_CHECK(hipMemcpy(d_meta, meta.data(), meta.size() * sizeof(size_t), hipMemcpyHostToDevice));
    }
    bool same = (int)h_src.size() == n;
    for (int i = 0; same && i < n; ++i) same = h_src[i] == ptrs[i];
    if (!same) {  // the tensors moved (first call, load_state_dict with new storage): refresh the pointer table
        for (int i = 0; i < n; ++i) ORBIT_REQUIRE(ptrs[i], "%s: null tensor %d", who, i);
        h_src.clear();                             // (a failure below leaves no shadow that a later call could match)
        ORBIT_HIP_CHECK(hipStreamSynchronize(s));  // the table may still be read by an earlier gather on this stream
        ORBIT_HIP_CHECK(hipMemcpy(d_src, ptrs, n * sizeof(float*), hipMemcpyHostToDevice));
        h_src.assign(ptrs, ptrs + n);
    }
    gather_params_kernel<<<dim3(chunks, n), 256, 0, s>>>(d_src, d_meta, d_pool);
    ORBIT_LAUNCH_CHECK();
    for (Param& p : params) p.loaded = true;
    return ORBIT_OK;
}

}  // namespace orbit
