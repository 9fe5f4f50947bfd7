// ORBIT benchmark metrics of one task's target videos in one launch (reference utils/eval_metrics.py:27-69).
//
// Frame accuracy, frames-to-recognition and video accuracy are functions of the per-frame argmax alone, so a whole task's
// evaluation is an integer reduction over the logits the head left on the device: per video the number of correct frames,
// the index of the first correct frame and the histogram of predicted classes. Everything is an integer add or min - no
// floating-point accumulation anywhere - so the outputs are exactly reproducible whatever order the LDS atomics arrive in.
//
// Mapping: one block per video, one thread per frame, the block looping over videos longer than its 256 threads. The shapes
// are tiny (C is 2 .. 15 in practice, a 200-frame video is ~8 KB of logits) and the launch is latency-bound: a thread walks
// its own row of C floats (neighbouring threads' rows share cache lines, every line is fetched once into L1), the histogram
// row lives in LDS, and the two scalars are reduced per wave with shuffles before one LDS atomic per wave. A video's frames
// mostly predict ONE class, so the histogram add is a same-address LDS atomic (~64 serialised adds per wave instruction,
// tens of nanoseconds for the 4 waves of a 200-frame video): not worth a ballot-aggregation loop at these sizes.
#include "common.h"
#include "device_util.h"

namespace orbit {

constexpr int EVAL_THREADS = 256;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ __launch_bounds__(EVAL_THREADS) void video_metrics_kernel(
    const float* __restrict__ logits, int M, int C, const int32_t* __restrict__ video_offsets,
    const int64_t* __restrict__ video_labels, int32_t* __restrict__ preds, int32_t* __restrict__ correct,
    int32_t* __restrict__ first_correct, int32_t* __restrict__ hist) {
    extern __shared__ int32_t s_hist[];  // [C]
    __shared__ int32_t s_correct, s_first;
    const int v = blockIdx.x;
    // the offsets are device data the host cannot validate: clamped into [0, M] and made ascending here, so a bad table
    // gives wrong counts, never a read or a write outside logits / preds
    const int lo = min(max(video_offsets[v], 0), M);
    const int hi = min(max(video_offsets[v + 1], lo), M);
    const int n = hi - lo;
    const int64_t label = video_labels[v];  // outside [0, C): equals no prediction
    for (int c = threadIdx.x; c < C; c += EVAL_THREADS) s_hist[c] = 0;
    if (threadIdx.x == 0) s_correct = 0, s_first = n;  // n: "no frame correct"; 0 for an empty video
    __syncthreads();
    int my_correct = 0, my_first = n;
    for (int f = threadIdx.x; f < n; f += EVAL_THREADS) {
        const float* row = logits + (size_t)(lo + f) * C;
        float best = -INFINITY;
        int best_c = 0;
        for (int c = 0; c < C; ++c) argmax_step(row[c], c, best, best_c);
        if (preds != nullptr) preds[lo + f] = best_c;
        atomicAdd(&s_hist[best_c], 1);
        if ((int64_t)best_c == label) {
            ++my_correct;
            my_first = min(my_first, f);  // f ascends within a thread: the first hit stays
        }
    }
    my_correct = wave_sum_int(my_correct);
    my_first = wave_min_int(my_first);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_correct, my_correct);
        atomicMin(&s_first, my_first);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += EVAL_THREADS) hist[(size_t)v * C + c] = s_hist[c];
    if (threadIdx.x == 0) correct[v] = s_correct, first_correct[v] = s_first;
}

}  // namespace orbit

using namespace orbit;

extern "C" int orbit_video_metrics(const float* logits, int M, int C, const int32_t* video_offsets,
                                   const int64_t* video_labels, int V, int32_t* preds, int32_t* correct,
                                   int32_t* first_correct, int32_t* hist, orbit_stream_t stream) {
    ORBIT_REQUIRE(M >= 0 && V >= 0 && C >= 1, "video_metrics: bad sizes (M %d, V %d, C %d)", M, V, C);
    ORBIT_REQUIRE(C <= ORBIT_VIDEO_METRICS_MAX_C, "video_metrics: C = %d exceeds the limit of %d classes (the histogram row is kept in LDS)",
                  C, ORBIT_VIDEO_METRICS_MAX_C);
    ORBIT_REQUIRE(logits && video_offsets && video_labels && correct && first_correct && hist, "video_metrics: null pointer");
    if (M == 0 || V == 0) return ORBIT_OK;
    hipStream_t s = (hipStream_t)stream;
    const int rec = prof_start("video_metrics", 0.0, 4.0 * M * C + 4.0 * M + 4.0 * V * (C + 3.0) + 8.0 * V, s);
    video_metrics_kernel<<<V, EVAL_THREADS, (size_t)C * sizeof(int32_t), s>>>(logits, M, C, video_offsets, video_labels, preds,
                                                                              correct, first_correct, hist);
    prof_stop(rec, s);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}
