// Multi-tensor optimizer step of the learners: reference utils/optim.py:11-33 builds torch.optim.Adam / torch.optim.SGD over
// two parameter groups; single-step-learner.py:163 steps it once per `tasks_per_batch` tasks and the FineTuner
// (few_shot_recognisers.py:207-217) `personalize_num_grad_steps` times per test task. Here ONE launch updates every tensor of
// the model, whatever their number: grid (chunks, tensors) over a device table of rows (orbit_optim_row_t), the layout of
// gather_params_kernel (csrc/param_pool.hip).
//
// The arithmetic is torch.optim's, op for op, in the rounding order of its foreach path (each foreach op is one rounding;
// `a + alpha * b` inside one op is a fused multiply-add there):
//   Adam  g' = fma(wd, p, g)                 (skipped for wd == 0)
//         m  = lerp(m, g', 1 - beta1)        = fma(w, g' - m, m) for w < 0.5
//         v  = fma(1 - beta2, g' * g', v * beta2)
//         p  = fma(-lr / (1 - beta1^t), m / (sqrt(v) / sqrt(1 - beta2^t) + eps), p)
//   SGD   g' = fma(wd, p, g);  buf = g' (first step of a tensor) or buf * mu + g';  p = fma(-lr, buf, p)   (mu == 0: buf = g')
// The bias corrections and step sizes are computed on the host in double and rounded to float once, as torch passes them.
// sqrtf and `/` are the correctly rounded forms (the default of hipcc for HIP; no fast reciprocal). Contraction is off inside
// the element functions so that only the fmaf calls written here fuse.
//
// Memory-bound: 28 bytes per element for Adam (p, g, m, v in; p, m, v out), 12 or 20 for SGD. A row whose pointers are all
// 16-byte aligned goes through float4 loads and stores with a scalar tail; any other row (a view into a flat gradient bucket,
// a sliced tensor) takes the scalar path. 64-bit element indices, no atomics, no LDS.
#include "common.h"

namespace orbit {

constexpr int OPTIM_CHUNK = 8192;        // elements per (block, iteration): 256 threads x 8 float4
constexpr int OPTIM_MAX_BLOCKS = 2048;   // memory-bound idiom: 256 CUs x 8 blocks, the rest is walked by the grid-stride loop
constexpr int OPTIM_MAX_TENSORS = 65535; // gridDim.y

struct OptimGroups {
    float step[ORBIT_OPTIM_MAX_GROUPS];  // Adam: -lr / (1 - beta1^t); SGD: -lr
    float wd[ORBIT_OPTIM_MAX_GROUPS];
};

struct AdamOp {
    static constexpr bool S1 = true, S2 = true;
    OptimGroups g;
    float w1, one_minus_w1, beta2, w2, bc2_sqrt, eps;
    __device__ __forceinline__ void operator()(float& p, float grad, float& m, float& v, int group, int) const {
#pragma clang fp contract(off)
        const float wd = g.wd[group];
        if (wd != 0.f) grad = fmaf(wd, p, grad);
        const float d = grad - m;
        m = w1 < 0.5f ? fmaf(w1, d, m) : grad - d * one_minus_w1;  // at::lerp's two branches
        v = fmaf(w2, grad * grad, v * beta2);  // addcmul: input + value * (t1 * t2)
        const float denom = sqrtf(v) / bc2_sqrt + eps;
        p = fmaf(g.step[group], m / denom, p);
    }
};

template <bool MOMENTUM>
struct SgdOp {
    static constexpr bool S1 = MOMENTUM, S2 = false;
    OptimGroups g;
    float mu;
    __device__ __forceinline__ void operator()(float& p, float grad, float& buf, float&, int group, int flags) const {
#pragma clang fp contract(off)
        const float wd = g.wd[group];
        if (wd != 0.f) grad = fmaf(wd, p, grad);
        if (MOMENTUM) {
            buf = (flags & ORBIT_OPTIM_FIRST_STEP) ? grad : buf * mu + grad;
            grad = buf;
        }
        p = fmaf(g.step[group], grad, p);
    }
};

template <class Op>
__global__ __launch_bounds__(256) void optim_step_kernel(const orbit_optim_row_t* __restrict__ rows, const Op op) {
    const orbit_optim_row_t r = rows[blockIdx.y];
    float* p = (float*)r.p;
    const float* g = (const float*)r.grad;
    float* s1 = (float*)r.state1;
    float* s2 = (float*)r.state2;
    const size_t n = r.numel;
    const size_t nchunks = (n + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    uintptr_t bits = (uintptr_t)p | (uintptr_t)g;
    if (Op::S1) bits |= (uintptr_t)s1;
    if (Op::S2) bits |= (uintptr_t)s2;
    const bool vec = (bits & 15) == 0;
    for (size_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const size_t lo = c * OPTIM_CHUNK;
        const size_t hi = lo + OPTIM_CHUNK < n ? lo + OPTIM_CHUNK : n;
        size_t tail = lo;  // first element of the chunk that the scalar loop takes
        if (vec) {
            const size_t nvec = (hi - lo) / 4;  // lo is a multiple of 4
            for (size_t q = threadIdx.x; q < nvec; q += 256) {
                const size_t i = lo + 4 * q;
                float4 P = *reinterpret_cast<const float4*>(p + i);
                const float4 G = *reinterpret_cast<const float4*>(g + i);
                float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
                if (Op::S1) A = *reinterpret_cast<const float4*>(s1 + i);
                if (Op::S2) B = *reinterpret_cast<const float4*>(s2 + i);
                op(P.x, G.x, A.x, B.x, r.group, r.flags);
                op(P.y, G.y, A.y, B.y, r.group, r.flags);
                op(P.z, G.z, A.z, B.z, r.group, r.flags);
                op(P.w, G.w, A.w, B.w, r.group, r.flags);
                *reinterpret_cast<float4*>(p + i) = P;
                if (Op::S1) *reinterpret_cast<float4*>(s1 + i) = A;
                if (Op::S2) *reinterpret_cast<float4*>(s2 + i) = B;
            }
            tail = lo + 4 * nvec;
        }
        for (size_t i = tail + threadIdx.x; i < hi; i += 256) {
            float P = p[i], A = 0.f, B = 0.f;
            if (Op::S1) A = s1[i];
            if (Op::S2) B = s2[i];
            op(P, g[i], A, B, r.group, r.flags);
            p[i] = P;
            if (Op::S1) s1[i] = A;
            if (Op::S2) s2[i] = B;
        }
    }
}

// Everything an optimizer step checks before it touches the device, from the HOST copy of the table. *total / *longest receive
// the element count of the table and of its longest row.
static int check_rows(const char* who, const void* d_rows, const orbit_optim_row_t* h, int n, const double* lr, const double* wd,
                      int n_groups, bool need1, bool need2, size_t* total, size_t* longest) {
    ORBIT_REQUIRE(d_rows && h && lr && wd, "%s: null pointer (table, host table, group lr or group weight_decay)", who);
    ORBIT_REQUIRE(n > 0 && n <= OPTIM_MAX_TENSORS, "%s: n_tensors must be in [1, %d] (got %d)", who, OPTIM_MAX_TENSORS, n);
    ORBIT_REQUIRE(n_groups >= 1 && n_groups <= ORBIT_OPTIM_MAX_GROUPS, "%s: n_groups must be in [1, %d] (got %d)", who,
                  ORBIT_OPTIM_MAX_GROUPS, n_groups);
    for (int k = 0; k < n_groups; ++k)
        ORBIT_REQUIRE(lr[k] >= 0.0 && wd[k] >= 0.0, "%s: group %d has a negative (or NaN) lr or weight_decay", who, k);
    *total = 0, *longest = 0;
    for (int i = 0; i < n; ++i) {
        const orbit_optim_row_t& r = h[i];
        ORBIT_REQUIRE(r.p && r.grad && (!need1 || r.state1) && (!need2 || r.state2), "%s: row %d: null pointer", who, i);
        uintptr_t bits = (uintptr_t)r.p | (uintptr_t)r.grad;
        if (need1) bits |= (uintptr_t)r.state1;
        if (need2) bits |= (uintptr_t)r.state2;
        ORBIT_REQUIRE((bits & 3) == 0, "%s: row %d: pointers must be 4-byte aligned", who, i);
        ORBIT_REQUIRE(r.numel > 0, "%s: row %d: numel == 0", who, i);
        ORBIT_REQUIRE(r.group >= 0 && r.group < n_groups, "%s: row %d: group index %d out of range [0, %d)", who, i, r.group,
                      n_groups);
        *total += r.numel;
        if (r.numel > *longest) *longest = r.numel;
    }
    return ORBIT_OK;
}

template <class Op>
static int launch_optim(const char* name, const orbit_optim_row_t* d_rows, int n, size_t total, size_t longest, double bytes_per_el,
                        const Op& op, hipStream_t s) {
    const size_t chunks = (longest + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
    const size_t cap = OPTIM_MAX_BLOCKS / n > 0 ? OPTIM_MAX_BLOCKS / n : 1;
    const int pi = prof_start(name, 0.0, bytes_per_el * (double)total, s);
    optim_step_kernel<Op><<<dim3((unsigned)(chunks < cap ? chunks : cap), n), 256, 0, s>>>(d_rows, op);
    prof_stop(pi, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_optim_adam_step(const orbit_optim_row_t* rows, const orbit_optim_row_t* host_rows, int n_tensors, const double* group_lr,
                          const double* group_weight_decay, int n_groups, int64_t step, double beta1, double beta2, double eps,
                          orbit_stream_t stream) {
    size_t total, longest;
    if (int rc = check_rows("optim_adam_step", rows, host_rows, n_tensors, group_lr, group_weight_decay, n_groups, true, true, &total,
                            &longest))
        return rc;
    ORBIT_REQUIRE(step >= 1, "optim_adam_step: step must be >= 1 (got %lld)", (long long)step);
    ORBIT_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "optim_adam_step: betas must be in [0, 1)");
    ORBIT_REQUIRE(eps >= 0.0, "optim_adam_step: eps must not be negative");
    AdamOp op;
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    for (int k = 0; k < ORBIT_OPTIM_MAX_GROUPS; ++k) {
        op.g.step[k] = k < n_groups ? (float)((group_lr[k] / bc1) * -1.0) : 0.f;
        op.g.wd[k] = k < n_groups ? (float)group_weight_decay[k] : 0.f;
    }
    op.w1 = (float)(1.0 - beta1), op.one_minus_w1 = 1.0f - op.w1;
    op.beta2 = (float)beta2, op.w2 = (float)(1.0 - beta2);
    op.bc2_sqrt = (float)sqrt(bc2), op.eps = (float)eps;
    return launch_optim("optim_adam", rows, n_tensors, total, longest, 28.0, op, (hipStream_t)stream);
}

int orbit_optim_sgd_step(const orbit_optim_row_t* rows, const orbit_optim_row_t* host_rows, int n_tensors, const double* group_lr,
                         const double* group_weight_decay, int n_groups, double momentum, orbit_stream_t stream) {
    ORBIT_REQUIRE(momentum >= 0.0, "optim_sgd_step: momentum must not be negative");
    const bool mom = momentum != 0.0;
    size_t total, longest;
    if (int rc = check_rows("optim_sgd_step", rows, host_rows, n_tensors, group_lr, group_weight_decay, n_groups, mom, false, &total,
                            &longest))
        return rc;
    OptimGroups g;
    for (int k = 0; k < ORBIT_OPTIM_MAX_GROUPS; ++k) {
        g.step[k] = k < n_groups ? (float)-group_lr[k] : 0.f;
        g.wd[k] = k < n_groups ? (float)group_weight_decay[k] : 0.f;
    }
    if (mom) {
        SgdOp<true> op;
        op.g = g, op.mu = (float)momentum;
        return launch_optim("optim_sgd", rows, n_tensors, total, longest, 20.0, op, (hipStream_t)stream);
    }
    SgdOp<false> op;
    op.g = g, op.mu = 0.f;
    return launch_optim("optim_sgd", rows, n_tensors, total, longest, 12.0, op, (hipStream_t)stream);
}

}  // extern "C"
