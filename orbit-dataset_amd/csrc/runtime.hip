// Library-wide services of liborbit_hip, no kernels: the thread-local error buffer, the option table, the per-launch event
// profiler every kernel family reports to (prof_start / prof_stop, orbit_prof_*) and the runtime entry points of the C-ABI.
#include <cstdlib>
#include <mutex>
#include <vector>
#include "common.h"

namespace orbit {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- library options (tuning switches): name -> int; initial value from the environment ORBIT_<NAME upper-cased>
struct Option {
    const char* name;
    const char* env;
    int value;
    bool init;
};
static Option g_options[] = {
    // network runtime
    {"graph", "ORBIT_GRAPH", 2, false},              // forward launch sequences as HIP graphs: 0 never, 1 always, 2 adaptive
    {"train_graph", "ORBIT_TRAIN_GRAPH", 1, false},  // the same for the training entry points: 0 never, 1 from the second sight of a call
    {"mbconv_rows", "ORBIT_MBCONV_ROWS", 1, false},  // row-streaming fused MBConv fronts at plan creation (0 = conv + depthwise pair)
    {"stem_rows", "ORBIT_STEM_ROWS", 1, false},      // the same for stem + first depthwise
    {"train_dw_xf", "ORBIT_TRAIN_DW_XF", 1, false},  // no-backward training forwards: BatchNorm + SiLU applied on the depthwise load
    {"train_fused_fronts", "ORBIT_TRAIN_FUSED_FRONTS", 1, false},  // ... and MBConv fronts as statistics sweep + row-streaming kernel
    // dense convolutions
    {"conv_tile", "ORBIT_CONV_TILE", 0, false},      // 0 heuristic; 3 = 64x64, 4 = 128x32, 6 = 32x32 with K split over the waves
    {"conv_bk", "ORBIT_CONV_BK", 0, false},          // 0 = widest K-tile that divides Cin; 8 / 16 / 32 caps it
    {"conv_splitk", "ORBIT_CONV_SPLITK", 1, false},  // split-K over blocks for short, long-K layers
    {"conv_rgemm", "ORBIT_CONV_RGEMM", 1, false},    // pointwise register GEMMs (pw_rgemm, pw_stream): 0 never, 1 where measured faster, 2 wherever supported
    {"conv_bf3", "ORBIT_CONV_BF3", 0, false},        // OPT-IN bf16 x 3 split (bit 1 dense convs, bit 2 fused-front expands); never in `value`
    // depthwise kernel families: 1 = where measured faster (default), 0 = never, 2 = wherever it fits
    {"dw_window", "ORBIT_DW_WINDOW", 1, false},
    {"dw_lds", "ORBIT_DW_LDS", 1, false},
    {"dw_pipe", "ORBIT_DW_PIPE", 1, false},
    // head
    {"head_stream", "ORBIT_HEAD_STREAM", 1, false}};  // streaming distance kernel (T = 1, D = 512 / 1280); 0 = general LDS form
static Option* find_option(const char* name) {
    for (Option& o : g_options)
        if (strcmp(o.name, name) == 0) {
            if (!o.init) {
                const char* e = getenv(o.env);
                if (e) o.value = atoi(e);
                o.init = true;
            }
            return &o;
        }
    return nullptr;
}
int get_option(const char* name) {
    Option* o = find_option(name);
    return o ? o->value : 0;
}
// bumped by every orbit_set_option that changes a value: captured launch sequences (csrc/graph_cache.h) carry the
// epoch they were recorded under in their key, so a graph never replays kernels chosen under other option values
static int g_option_epoch = 0;
int option_epoch() { return g_option_epoch; }

// ---- optional per-launch profiling (bench.py roofline): HIP events recorded on the launch stream ------
struct ProfRec {
    hipEvent_t start, stop;
    int variant;
    double flops, bytes, silu;
};
struct ProfVariant {
    char name[48];
    long launches;
    double ms, flops, bytes;
    double floor_ms;  // sum over the launches of max(bytes / HBM rate, FLOP / matrix rate): the launch-by-launch roofline floor
    double silu;      // SiLU evaluations (two transcendentals each: the VALU work the matrix roof does not see)
    double floor_simd_ms;  // ... of max(bytes / HBM rate, FLOP / matrix rate + SiLU / SiLU rate): on gfx950 a SIMD issues EITHER
                           // an MFMA OR VALU instructions (profiles/r03_coexec_probe.txt), so matrix and SiLU time add up
};
// orbit_prof_set_roofs. SiLU: 11.06 ns of one SIMD per 64 evaluations at 8 waves per SIMD (v_exp_f32 + v_rcp_f32 + 3 packed
// multiply-adds, profiles/r03_valu_probe.txt) x 1024 SIMDs
static double g_roof_bytes_per_s = 6.3e12, g_roof_flop_per_s = 157.3e12, g_roof_silu_per_s = 64.0 * 1024.0 / 11.06e-9;
static bool g_prof_on = false;
bool conv_prof_enabled() { return g_prof_on; }
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;
static std::vector<ProfVariant> g_prof_variants;
// the record lists are shared by every thread that launches: the input pipeline's staging thread resizes frames
// (orbit_frames_resize_from_uint8, csrc/ingest.hip) while the main thread runs the extractor
static std::mutex g_prof_mu;

static hipEvent_t prof_event() {
    if (!g_prof_pool.empty()) {
        hipEvent_t e = g_prof_pool.back();
        g_prof_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
static int prof_variant(const char* name) {
    for (size_t i = 0; i < g_prof_variants.size(); ++i)
        if (strcmp(g_prof_variants[i].name, name) == 0) return (int)i;
    ProfVariant v;
    memset(&v, 0, sizeof(v));
    snprintf(v.name, sizeof(v.name), "%s", name);
    g_prof_variants.push_back(v);
    return (int)g_prof_variants.size() - 1;
}

// called by every kernel family's launchers: returns a record index or -1 when profiling is off
int prof_start(const char* name, double flops, double bytes, hipStream_t s, double silu) {
    if (!g_prof_on) return -1;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    ProfRec r;
    r.start = prof_event(), r.stop = prof_event(), r.variant = prof_variant(name);
    r.flops = flops, r.bytes = bytes, r.silu = silu;
    (void)hipEventRecord(r.start, s);
    g_prof_recs.push_back(r);
    return (int)g_prof_recs.size() - 1;
}
void prof_stop(int idx, hipStream_t s) {
    if (idx < 0) return;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (idx < (int)g_prof_recs.size()) (void)hipEventRecord(g_prof_recs[idx].stop, s);
}

}  // namespace orbit

using namespace orbit;

extern "C" {

int orbit_version(void) { return 100; }

/* Once per device the library is used on: keep freed stream-ordered allocations in the device's default memory pool. The
 * few entry points that take scratch with hipMallocAsync / hipFreeAsync (single-operator test entries, the FiLM generator's
 * backward) otherwise hit a pool whose release threshold is 0: every synchronisation trims it, the next call allocates for
 * real, and the real free that follows synchronises the device under the host's feet. */
int orbit_runtime_init(void) {
    int dev = 0;
    ORBIT_HIP_CHECK(hipGetDevice(&dev));
    static bool done[64] = {false};
    if (dev < 0 || dev >= 64 || done[dev]) return ORBIT_OK;
    hipMemPool_t pool = nullptr;
    ORBIT_HIP_CHECK(hipDeviceGetDefaultMemPool(&pool, dev));
    uint64_t keep = UINT64_MAX;
    ORBIT_HIP_CHECK(hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep));
    done[dev] = true;
    return ORBIT_OK;
}

int orbit_set_option(const char* name, int value) {
    ORBIT_REQUIRE(name, "set_option: null name");
    Option* o = find_option(name);
    ORBIT_REQUIRE(o != nullptr, "set_option: unknown option '%s'", name);
    if (o->value != value) ++g_option_epoch;
    o->value = value;
    return ORBIT_OK;
}
int orbit_get_option(const char* name) {
    if (!name) return -1;
    return find_option(name) ? get_option(name) : -1;
}
const char* orbit_last_error(void) { return err_buf(); }

int orbit_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_err(ORBIT_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

// Profiling of the dominant kernel (all conv_igemm instantiations). enable(1) starts recording one HIP event
// pair per launch on the launch stream; collect() waits for them, folds them into per-variant totals and
// returns the grand totals; variant(i) reads one row. Launches may be recorded from several threads; enable / collect are
// for one thread, called while no other thread is launching.
int orbit_prof_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = on != 0;
    if (on) {
        for (ProfRec& r : g_prof_recs) g_prof_pool.push_back(r.start), g_prof_pool.push_back(r.stop);
        g_prof_recs.clear();
        g_prof_variants.clear();
    }
    return ORBIT_OK;
}

int orbit_prof_collect(double* total_ms, double* total_flops, long* launches) {
    double ms = 0, fl = 0;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    for (ProfRec& r : g_prof_recs) {
        ORBIT_HIP_CHECK(hipEventSynchronize(r.stop));
        float t = 0.f;
        ORBIT_HIP_CHECK(hipEventElapsedTime(&t, r.start, r.stop));
        ProfVariant& v = g_prof_variants[r.variant];
        v.launches += 1, v.ms += t, v.flops += r.flops, v.bytes += r.bytes, v.silu += r.silu;
        const double fb = r.bytes / g_roof_bytes_per_s, ff = r.flops / g_roof_flop_per_s;
        v.floor_ms += 1e3 * (fb > ff ? fb : ff);
        const double fs = ff + r.silu / g_roof_silu_per_s;
        v.floor_simd_ms += 1e3 * (fb > fs ? fb : fs);
        ms += t, fl += r.flops;
        g_prof_pool.push_back(r.start), g_prof_pool.push_back(r.stop);
    }
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    if (launches) *launches = (long)g_prof_recs.size();
    g_prof_recs.clear();
    return ORBIT_OK;
}

int orbit_prof_num_variants(void) { return (int)g_prof_variants.size(); }

int orbit_prof_set_roofs(double hbm_bytes_per_s, double matrix_flop_per_s, double silu_evals_per_s) {
    ORBIT_REQUIRE(hbm_bytes_per_s > 0 && matrix_flop_per_s > 0 && silu_evals_per_s > 0, "prof_set_roofs: rates must be positive");
    g_roof_bytes_per_s = hbm_bytes_per_s, g_roof_flop_per_s = matrix_flop_per_s, g_roof_silu_per_s = silu_evals_per_s;
    return ORBIT_OK;
}

int orbit_prof_variant_floor(int i, double* floor_ms, double* floor_simd_ms, double* silu_evals) {
    ORBIT_REQUIRE(i >= 0 && i < (int)g_prof_variants.size(), "prof_variant_floor: index out of range");
    if (floor_ms) *floor_ms = g_prof_variants[i].floor_ms;
    if (floor_simd_ms) *floor_simd_ms = g_prof_variants[i].floor_simd_ms;
    if (silu_evals) *silu_evals = g_prof_variants[i].silu;
    return ORBIT_OK;
}

int orbit_prof_variant(int i, char* name48, long* launches, double* ms, double* flops, double* bytes) {
    ORBIT_REQUIRE(i >= 0 && i < (int)g_prof_variants.size(), "prof_variant: index out of range");
    const ProfVariant& v = g_prof_variants[i];
    if (name48) memcpy(name48, v.name, sizeof(v.name));
    if (launches) *launches = v.launches;
    if (ms) *ms = v.ms;
    if (flops) *flops = v.flops;
    if (bytes) *bytes = v.bytes;
    return ORBIT_OK;
}

}  // extern "C"
