// Training runtime of the network plans: forward with a tape (raw convolution outputs + activations + pooling
// argmax), train- or eval-mode BatchNorm, and the reverse pass producing parameter gradients (flat, in the layout of
// the parameter pool), FiLM gamma/beta gradients and nothing else (frames need no gradient).
//
// Reference: the graph autograd records for model/few_shot_recognisers.py:99-122 (_get_features with grad enabled),
// :345-356 (_get_task_embedding on the LITE subset) and walks in single-step-learner.py:234 (loss.backward()).
// BatchNorm mode follows :176-183: batch statistics (and running-stat updates, also on the no-grad LITE cache
// passes) iff the extractor is being learned; the set encoder always normalises with running statistics.
//
// Generic over the plan ops: OP_CONV (+BN, ReLU / SiLU, residual, squeeze-excite gate on the input, fused 2x2 pool),
// OP_DWCONV (+BN, SiLU), OP_SE, OP_MAXPOOL, OP_AVGPOOL — i.e. resnet18, efficientnet_b0 and the set encoder. (The
// opt-in fused MBConv front op of the inference plan has no training form.) efficientnet_v2_s, whose ConvBnAct blocks add
// their skip after the activation (Op::res_post), runs on an ORBIT_PLAN_RES_POST_BACKWARD plan in frozen form only: running
// statistics, BatchNorm weight / bias (FiLM) gradients, no filter gradients (plan_frozen_only) - and on an
// ORBIT_PLAN_RES_POST_TRAINING plan like the others: batch statistics, running-statistics updates, every parameter gradient
// (the LITE recipe of its checkpoints). Its 80 dense convs and 30 squeeze-excite blocks exceed the job lists of the two
// batched end-of-pass launches (WGRAD_REDUCE_JOBS, SE_PARAM_JOBS): the reverse pass flushes a full list with a launch and
// goes on collecting.
#include "extractor.h"

namespace orbit {

__global__ __launch_bounds__(256) void bn_eval_stats_kernel(const BNDev* __restrict__ descs,
                                                            const float* __restrict__ pool, float* __restrict__ mean,
                                                            float* __restrict__ invstd) {
    const BNDev d = descs[blockIdx.x];
    for (int c = blockIdx.y * 256 + threadIdx.x; c < d.C; c += gridDim.y * 256) {
        const float cb = d.conv_bias != (size_t)-1 ? pool[d.conv_bias + c] : 0.f;
        mean[d.fold_off + c] = pool[d.mean + c] - cb;  // xhat = (y_conv - mean') * invstd
        invstd[d.fold_off + c] = 1.0f / sqrtf(pool[d.var + c] + d.eps);
    }
}

// dst[0][fold_off + c] = running_mean, dst[1][fold_off + c] = running_var
__global__ __launch_bounds__(256) void bn_export_kernel(const BNDev* __restrict__ descs, const float* __restrict__ pool,
                                                        float* __restrict__ dst, size_t fold_floats) {
    const BNDev d = descs[blockIdx.x];
    for (int c = blockIdx.y * 256 + threadIdx.x; c < d.C; c += gridDim.y * 256) {
        dst[d.fold_off + c] = pool[d.mean + c];
        dst[fold_floats + d.fold_off + c] = pool[d.var + c];
    }
}

// running = (1 - momentum) * running + momentum * stat for every BatchNorm: the update an ORBIT_TRAIN_DEFER_RUNNING_STATS forward
// left undone (stat[0][fold_off + c] = batch mean (+ conv bias), stat[1][.] = unbiased batch variance; the expression is the one
// bn_stats_finalize_kernel evaluates)
__global__ __launch_bounds__(256) void bn_apply_deferred_kernel(const BNDev* __restrict__ descs, float* __restrict__ pool,
                                                                const float* __restrict__ stat, size_t fold_floats,
                                                                float momentum) {
    const BNDev d = descs[blockIdx.x];
    for (int c = blockIdx.y * 256 + threadIdx.x; c < d.C; c += gridDim.y * 256) {
        pool[d.mean + c] = (1.f - momentum) * pool[d.mean + c] + momentum * stat[d.fold_off + c];
        pool[d.var + c] = (1.f - momentum) * pool[d.var + c] + momentum * stat[fold_floats + d.fold_off + c];
    }
}

struct TapeLayout {
    // byte offsets per op ((size_t)-1: none). conv / depthwise: y raw output, a activation, p/idx fused pool.
    // squeeze-excite: p = pooled means [B][C], a = gate [B][C]. max-pool: p output, idx argmax.
    std::vector<size_t> y, a, p, idx;
    size_t mean = 0, invstd = 0, scale = 0, shift = 0, partial = 0, pool = 0, total = 0;
    size_t rstat = 0;  // [2][fold_floats]: batch mean / unbiased variance of an ORBIT_TRAIN_DEFER_RUNNING_STATS forward
};

static const size_t NONE = (size_t)-1;

static bool plan_trainable(const orbit_extractor* fe) {
    for (const Op& o : fe->ops) {
        if (o.kind == OP_MBFRONT) return false;
        if ((o.kind == OP_CONV || o.kind == OP_DWCONV) && o.bn < 0) return false;
        if (o.kind == OP_CONV && o.use_gate && (o.pool2 || o.x_nchw)) return false;
        // efficientnet_v2_s: the backward through the post-activation skip is opt-in (ORBIT_PLAN_RES_POST_BACKWARD)
        if (o.kind == OP_CONV && o.res_post && !fe->res_post_backward) return false;
    }
    return true;
}

// a plan that holds a post-activation skip trains in frozen form only - running statistics, no filter gradients - unless it was
// created with ORBIT_PLAN_RES_POST_TRAINING (the first opt-in keeps the scope it was merged and measured with)
static bool plan_frozen_only(const orbit_extractor* fe) {
    if (fe->res_post_training) return false;
    for (const Op& o : fe->ops)
        if (o.kind == OP_CONV && o.res_post) return true;
    return false;
}

static bool has_bn(const Op& o) { return o.kind == OP_CONV || o.kind == OP_DWCONV; }
static DwInXf in_xf(const BnFoldC& bn, int act) { return DwInXf{bn.scale, bn.shift, act}; }  // a layer's BatchNorm + activation as an input transform

// no op from `first` on reads buffer `id` before it is written again
static bool no_later_reader(const orbit_extractor* fe, size_t first, int id) {
    for (size_t j = first; j < fe->ops.size(); ++j) {
        const Op& q = fe->ops[j];
        if (q.in == id || q.res == id) return false;
        if (q.out == id) break;
    }
    return true;
}

// the depthwise op whose activated output squeeze-excite op i pools: the nearest one before it (-1: malformed plan)
static int se_source(const orbit_extractor* fe, size_t i) {
    for (int j = (int)i - 1; j >= 0; --j)
        if (fe->ops[j].kind == OP_DWCONV) return j;
    return -1;
}

// The two-sweep fused front (train_forms below) writes one statistics row per frame and strip-band tile. The partial buffer is
// sized for this many tiles per frame; wider maps (Wo = 113 / 120 for 452 / 480 pixel frames: 25 tiles) take the unfused pair
// before any statistics are touched.
static const int FRONT_TILE_CAP = 16;

static size_t max_bn_partial_floats(const orbit_extractor* fe, int B) {
    size_t m = 4;
    for (const Op& o : fe->ops)
        if (has_bn(o)) {
            const size_t M = (size_t)B * o.Ho * o.Wo;
            m = std::max(m, (size_t)bn_reduce_blocks((int)M, o.Cout) * 2 * o.Cout + 3 * (size_t)o.Cout);
            // statistics partials written by the producing kernel's epilogue (one per 32+ conv rows / per depthwise chunk)
            if (o.kind == OP_CONV) {
                m = std::max(m, bn_partial_floats((M + 31) / 32, o.Cout));
                // backward: reduction written by the data gradient of the depthwise convolution it feeds (+ coefficients)
                for (int st : {1, 2}) {
                    LayerGeom dw;  // (of that depthwise layer only what dwconv_dgrad_bn_blocks reads)
                    dw.B = B, dw.H = o.Ho, dw.W = o.Wo, dw.Cin = o.Cout, dw.stride = st;
                    m = std::max(m, bn_partial_floats((size_t)dwconv_dgrad_bn_blocks(dw), o.Cout) + 3 * (size_t)o.Cout);
                }
            }
            else {
                m = std::max(m, bn_partial_floats((size_t)B * dwconv_se_chunks(o.Ho), o.Cout));
                // (the two-sweep fused front writes one row per frame and strip-band tile instead; its first sweep's Gram
                // partials of the block input live here too)
                m = std::max(m, bn_partial_floats((size_t)B * FRONT_TILE_CAP, o.Cout));
                m = std::max(m, bn_gram_scratch_floats(B * o.H * o.W, BN_GRAM_MAX_CIN));
            }
            // backward of a depthwise BatchNorm whose reduction rides on the squeeze-excite backward (+ 3*C coefficients)
            if (o.kind == OP_DWCONV)
                m = std::max(m, bn_partial_floats((size_t)B * se_pool_chunks(B, o.Ho * o.Wo, o.Cout), o.Cout) + 3 * (size_t)o.Cout);
        }
    return m;
}

// squeeze-excite pooling partials of the pooled apply pass (launch_scale_shift_act_pool): [B][chunks][C]
static size_t max_se_pool_floats(const orbit_extractor* fe, int B) {
    size_t m = 4;
    for (size_t i = 0; i < fe->ops.size(); ++i) {
        const Op& o = fe->ops[i];
        const int dw = o.kind == OP_SE ? se_source(fe, i) : -1;
        if (dw >= 0) m = std::max(m, (size_t)B * se_pool_chunks(B, fe->ops[dw].Ho * fe->ops[dw].Wo, o.Cin) * o.Cin);
    }
    return m;
}

static TapeLayout tape_layout(const orbit_extractor* fe, int B) {
    TapeLayout L;
    const size_t n = fe->ops.size();
    L.y.assign(n, NONE), L.a.assign(n, NONE), L.p.assign(n, NONE), L.idx.assign(n, NONE);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(bytes, 256);
        return o;
    };
    for (size_t i = 0; i < n; ++i) {
        const Op& o = fe->ops[i];
        if (o.kind == OP_CONV) {
            const size_t e = (size_t)B * o.Ho * o.Wo * o.Cout;
            L.y[i] = take(e * 4), L.a[i] = take(e * 4);
            if (o.pool2) {
                const size_t pe = (size_t)B * (o.Ho / 2) * (o.Wo / 2) * o.Cout;
                L.p[i] = take(pe * 4), L.idx[i] = take(pe);
            }
            // (a gated projection reads x and the gate separately - forward through the GATE prologue of conv_igemm, filter
            // gradient through conv_wgrad's - so the product x * gate is never materialised and has no place on the tape)
        } else if (o.kind == OP_DWCONV) {
            const size_t e = (size_t)B * o.Ho * o.Wo * o.Cout;
            L.y[i] = take(e * 4), L.a[i] = take(e * 4);
        } else if (o.kind == OP_SE) {
            L.p[i] = take((size_t)B * o.Cin * 4), L.a[i] = take((size_t)B * o.Cin * 4);
        } else if (o.kind == OP_MAXPOOL) {
            const size_t pe = (size_t)B * o.Ho * o.Wo * o.Cout;
            L.p[i] = take(pe * 4), L.idx[i] = take(pe);
        }
    }
    L.mean = take(fe->fold_floats * 4), L.invstd = take(fe->fold_floats * 4);
    L.scale = take(fe->fold_floats * 4), L.shift = take(fe->fold_floats * 4);
    L.partial = take(max_bn_partial_floats(fe, B) * 4);
    L.pool = take(max_se_pool_floats(fe, B) * 4);
    L.rstat = take(2 * fe->fold_floats * 4);
    L.total = off;
    return L;
}

// which op produced the tensor an op reads (index into ops, -1 = the frames)
struct Producers {
    std::vector<int> in, res, gate;  // gate: the squeeze-excite op whose output a gated conv multiplies into its input
};
static Producers producers(const orbit_extractor* fe) {
    Producers P;
    std::map<int, int> last;  // buffer id -> op index
    for (size_t i = 0; i < fe->ops.size(); ++i) {
        const Op& o = fe->ops[i];
        P.in.push_back(o.in >= 0 && last.count(o.in) ? last[o.in] : -1);
        P.res.push_back(o.res >= 0 && last.count(o.res) ? last[o.res] : -1);
        P.gate.push_back(o.kind == OP_CONV && o.use_gate && last.count(BUF_GATE) ? last[BUF_GATE] : -1);
        last[o.out] = (int)i;
    }
    return P;
}

// ---- the training form of every op ----------------------------------------------------------------------------------------
// Decided here, once per run, for the forward AND the backward (both call train_forms on the same plan, batch and BatchNorm mode;
// the backward with no_backward = false). This is the only reader of the options train_dw_xf and train_fused_fronts: do not flip
// them between a forward and its backward. The sizing functions above stay independent of options and flags (the tape is sized
// without them): they take the maximum over the forms.
enum ConvForm {
    CONV_PLAIN,       // (batch statistics, then) the activation pass
    CONV_DUAL,        // running-statistics BatchNorm: the conv's epilogue writes the raw output AND the activation
    CONV_RAW_TO_DW,   // batch statistics only: the depthwise conv that follows applies BatchNorm + activation as it loads
    CONV_SWEEP_GRAM,  // sweep 1 of a fused front: batch statistics from the Gram matrix of the conv's input, no conv
    CONV_SWEEP_CONV   // sweep 1 of a fused front: the conv run for its statistics alone (ConvDesc::stats_only)
};
struct OpForm {
    ConvForm conv = CONV_PLAIN;  // OP_CONV
    int tiles = 0;               // ... the two sweeps: strip-band tiles per frame of the fused front (<= FRONT_TILE_CAP)
    int raw_src = -1;            // OP_DWCONV: the conv whose RAW output it reads (CONV_RAW_TO_DW; the backward's raw_fed), or -1
    int front = -1;              // ... the conv it runs with as the row-streaming fused front (sweep 2), or -1
    bool pooled = false;         // ... its activation pass also leaves the squeeze-excite pooling partials in TapeLayout::pool
    bool through_act = false;    // ... backward: its data gradient may go through the producing conv's activation (DwBnBwd)
    bool wgrad_rides = false;    // ... backward: and its filter gradient may ride on that kernel (DwBnBwd::wgrad_partial)
    bool se_sums_only = false;   // OP_CONV with a gate: backward: the squeeze-excite backward may leave only the BatchNorm sums
    int se_dw = -1;              // OP_SE: the depthwise op it pools
    bool se_batched = false;     // ... backward: its parameter gradients fit the batched end-of-pass launch
};
typedef std::vector<OpForm> TrainForms;

static TrainForms train_forms(const orbit_extractor* fe, int B, int bn_train, bool no_backward) {
    const int dw_xf = get_option("train_dw_xf"), fronts = get_option("train_fused_fronts");
    const size_t n = fe->ops.size();
    const Producers P = producers(fe);
    TrainForms F(n);
    // what raw-fed and through-act share: a batch-statistics conv, no fused pool, no residual, float4 channels, option on
    auto xf_conv = [&](const Op& o) {
        return o.kind == OP_CONV && bn_train && dw_xf && !o.pool2 && o.res < 0 && o.Cout % 4 == 0;
    };
    for (size_t i = 0; i < n; ++i) {
        const Op& o = fe->ops[i];
        OpForm& f = F[i];
        if (o.kind == OP_CONV) {
            // the depthwise conv that follows and reads this output, and whether it is the ONLY reader
            const Op* d = i + 1 < n && fe->ops[i + 1].kind == OP_DWCONV && fe->ops[i + 1].in == o.out ? &fe->ops[i + 1] : nullptr;
            const bool sole = d && no_later_reader(fe, i + 2, o.out);
            // Two-sweep fused front: on a NO-BACKWARD batch-statistics forward (the cache pass of the LITE step: 200 frames under
            // torch.no_grad() while the extractor is being learned, reference few_shot_recognisers.py:404-408) an MBConv block's
            // expansion conv + depthwise conv run as the row-streaming fused front of the inference plans in two sweeps: (1) the
            // first BatchNorm's batch statistics - from the Gram matrix of the block's input where bn_gram_supported (csrc/
            // train_ops.hip launch_bn_stats_from_gram), else from the expansion conv as a STATISTICS SWEEP (same kernel, same
            // tiles, nothing stored), (2) the fused front (csrc/mbconv_rows.hip, RAW form) re-expands in its LDS ring with that
            // scale / shift, stores the RAW depthwise outputs and their column sums - the second BatchNorm then proceeds as on the
            // unfused path. The 6x-expanded tensor (963 MB per 200 frames for block 1.0) is neither written nor read. Taped
            // forwards keep the unfused pair: their backward reads that tensor.
            // `train_fused_fronts`: 1 (default) = where measured faster (the 112x112 / 56x56 blocks), 0 = never, 2 = every
            // supported shape, 3 = as 2 with the statistics sweep of the conv instead of the Gram-matrix statistics (parity tests:
            // bit-identical first BatchNorm).
            bool front = fronts && bn_train && no_backward && sole && !o.x_nchw && !o.pool2 && o.res < 0 && !o.use_gate &&
                         o.KH == 1 && o.KW == 1 && o.stride == 1 && o.act == ORBIT_ACT_SILU && d->act == ORBIT_ACT_SILU &&
                         d->Cin == o.Cout && mbconv_rows_supported(o.H, o.W, o.Cin, o.Cout, d->KH, d->stride) &&
                         fe->bns[o.bn].conv_bias < 0;
            if (front && fronts == 1 && o.H < 56) front = false;  // (the 28x28 blocks: statistics sweep + front measured no faster than the pair)
            const int tiles = front ? mbconv_rows_tiles(o.H, o.W, o.Cin, o.Cout, d->KH, d->stride) : 0;
            if (tiles <= 0 || tiles > FRONT_TILE_CAP) front = false;
            // Raw-to-depthwise: a batch-statistics conv whose activated output is read by ONE consumer, the depthwise conv that
            // follows (EfficientNet's expansion convs and stem): that consumer applies the conv's BatchNorm + SiLU as it loads the
            // RAW output (DwInXf in csrc/ops.hip), so the activated 6x-expanded tensor is never written - on forwards that run no
            // backward and on TAPED ones: the only other reader of the activation is the depthwise filter gradient, whose LDS form
            // applies the same transform as it stages its input patch (dwconv_wgrad_lds_kernel, csrc/train_mbconv.hip; each
            // element passes once). A first attempt with the transform inside the global-load filter-gradient kernel - every
            // input loaded K times, SiLU per load - lost more there (1.76 -> 3.98 ms) than the forward gained
            // (profiles/r05_lite_ab_taped_xf.txt). The activation must not be ReLU on a taped forward (its BatchNorm backward
            // reads the mask from the activated tensor).
            const bool raw = xf_conv(o) && sole &&
                             (no_backward || ((o.act == ORBIT_ACT_SILU || o.act == ORBIT_ACT_NONE) &&
                                              dwconv_wgrad_xf_supported(d->geom(B))));
            // Dual write: running-statistics BatchNorm (frozen extractor: CNAPs meta-training, FiLM fine-tuning): scale / shift
            // are known before the conv runs, so its epilogue writes BOTH the raw output (tape: xhat and the SiLU derivative need
            // it) and the activation - no separate activation pass over the tensor
            // (a post-activation skip keeps CONV_PLAIN: conv_igemm has no dual-output form of that epilogue, and the two such
            // ops of efficientnet_v2_s do not pay for one - raw conv, then the activation pass in its post-skip form)
            if (front) f.conv = bn_gram_supported(o.Cin) && fronts != 3 ? CONV_SWEEP_GRAM : CONV_SWEEP_CONV, f.tiles = tiles;
            else if (!bn_train && !o.pool2 && !o.res_post) f.conv = CONV_DUAL;
            else if (raw) f.conv = CONV_RAW_TO_DW;
            const int src = P.in[i];  // (the 2^32 bound: the 32-bit element index of the BatchNorm apply pass that rebuilds g)
            f.se_sums_only = o.use_gate && src >= 0 && fe->ops[src].kind == OP_DWCONV &&
                             (unsigned long long)B * o.H * o.W * (o.Cin / 4) < (1ull << 32);
        } else if (o.kind == OP_DWCONV) {
            const int prev = (int)i - 1;  // (a conv in one of the three forms below is followed by its depthwise reader)
            if (prev >= 0 && F[prev].conv == CONV_RAW_TO_DW) f.raw_src = prev;
            if (prev >= 0 && (F[prev].conv == CONV_SWEEP_GRAM || F[prev].conv == CONV_SWEEP_CONV)) f.front = prev;
            // the activation pass also produces the squeeze-excite pooling partials when an SE op consumes this tensor
            f.pooled = i + 1 < n && fe->ops[i + 1].kind == OP_SE;
            // the producer is a convolution + BatchNorm + SiLU right before this layer. Not raw_fed: no filter-gradient fit test
            // and no later-reader test here (the data gradient's epilogue needs neither), but no conv bias.
            const int src = P.in[i];
            f.through_act = src >= 0 && src == prev && xf_conv(fe->ops[src]) && fe->bns[fe->ops[src].bn].conv_bias < 0 &&
                            (fe->ops[src].act == ORBIT_ACT_SILU || fe->ops[src].act == ORBIT_ACT_NONE);
            f.wgrad_rides = f.through_act && f.raw_src >= 0 && dwconv_bwd_fused_scratch_floats(o.geom(B)) > 0;
        } else if (o.kind == OP_SE) {
            f.se_dw = se_source(fe, i);
            f.se_batched = o.R <= SE_PARAM_MAX_R;
        }
    }
    return F;
}

struct BwdLayout {
    static const int NSLOTS = 8;
    size_t slot_bytes = 0, slots = 0, up = 0, wgrad = 0, partial = 0, total = 0;
    // byte offsets per op (NONE: the op has none). OP_CONV: the partial tiles of its filter gradient; OP_SE: the scratch of its
    // backward. A region per layer, because their reductions run batched at the end of the pass (WgradReduceJobs, SeParamJobs).
    std::vector<size_t> cwgrad, se;
};
static BwdLayout bwd_layout(const orbit_extractor* fe, int B) {
    BwdLayout L;
    const size_t n = fe->ops.size();
    L.cwgrad.assign(n, NONE), L.se.assign(n, NONE);
    size_t slot = 4, up = 4, wg = 4, se = 0, cwg = 0;
    // (in the order the reverse pass meets the layers: the last layer's regions come first)
    for (size_t i = n; i-- > 0;) {
        const Op& o = fe->ops[i];
        const LayerGeom g = o.geom(B);
        if (o.kind == OP_DWCONV) {
            slot = std::max(slot, (size_t)B * o.H * o.W * o.Cin);
            slot = std::max(slot, (size_t)B * o.Ho * o.Wo * o.Cout);
            wg = std::max(wg, dwconv_wgrad_scratch_floats(g));
            wg = std::max(wg, dwconv_bwd_fused_scratch_floats(g));
        } else if (o.kind == OP_SE) {
            L.se[i] = se * 4, se += align_up(se_bwd_scratch_floats(B, o.Cin, o.R), 64);
        } else if (o.kind == OP_CONV) {
            slot = std::max(slot, (size_t)B * o.Ho * o.Wo * o.Cout);
            if (!o.x_nchw) slot = std::max(slot, (size_t)B * o.H * o.W * o.Cin);
            if (o.stride > 1 && !o.x_nchw) up = std::max(up, (size_t)B * o.H * o.W * o.Cout);
            L.cwgrad[i] = cwg * 4, cwg += align_up(conv_wgrad_scratch_floats(g), 64);
        } else if (o.kind == OP_MAXPOOL || o.kind == OP_AVGPOOL) {
            slot = std::max(slot, (size_t)B * o.H * o.W * o.Cin);
        }
    }
    size_t off = 0;
    L.slot_bytes = align_up(slot * 4, 256);
    L.slots = off, off += L.slot_bytes * BwdLayout::NSLOTS;
    L.up = off, off += align_up(up * 4, 256);
    L.wgrad = off, off += align_up(wg * 4, 256);
    for (size_t& c : L.cwgrad)
        if (c != NONE) c += off;
    off += align_up((cwg + 4) * 4, 256);
    L.partial = off, off += align_up(max_bn_partial_floats(fe, B) * 4, 256);
    for (size_t& c : L.se)
        if (c != NONE) c += off;
    off += align_up((se + 4) * 4, 256);
    L.total = off;
    return L;
}

}  // namespace orbit

using namespace orbit;

// the dgrad-packed filters follow the parameters: built at the first backward, repacked whenever a load cleared dgrad_packed
static int ensure_dgrad_filters(orbit_extractor* fe, hipStream_t s) {
    if (fe->dgrad_off.empty()) {
        fe->dgrad_off.assign(fe->ops.size(), NONE);
        size_t off = 0;
        for (size_t i = 0; i < fe->ops.size(); ++i) {
            const Op& o = fe->ops[i];
            if (o.kind != OP_CONV || o.x_nchw) continue;
            fe->dgrad_off[i] = off;
            off += conv_dgrad_packed_floats(o.Cin, o.Cout, o.KH, o.KW);
        }
        ORBIT_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&fe->d_dgrad), std::max<size_t>(off, 4) * sizeof(float)));
    }
    if (!fe->dgrad_packed) {
        if (fe->dgrad_jobs.empty()) {
            for (size_t i = 0; i < fe->ops.size(); ++i) {
                const Op& o = fe->ops[i];
                if (fe->dgrad_off[i] == NONE) continue;
                const ConvPackGeom g = conv_pack_geom(o.Cout, o.Cin, o.KH, o.KW, 0);  // the dgrad conv: Cin' = Cout, Cout' = Cin
                PackJob j;
                j.src = fe->param(o.weight), j.dst = fe->d_dgrad + fe->dgrad_off[i], j.kind = 4;
                j.Cin = o.Cin, j.Cout = o.Cout, j.KH = o.KH, j.KW = o.KW, j.cin_pad = g.cin_pad, j.KT = g.kt;
                j.cout_pad = g.cout_pad, j.total = (unsigned)((size_t)g.cout_pad * g.kt);
                fe->dgrad_jobs.push_back(j);
            }
        }
        if (int rc = run_pack_jobs(fe->dgrad_jobs, &fe->d_dgrad_jobs, s)) return rc;
        fe->dgrad_packed = true;
    }
    return ORBIT_OK;
}

static int train_forward_run(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                             const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                             hipStream_t s, bool no_backward = false, bool defer_stats = false);

extern "C" {

int orbit_extractor_supports_training(const orbit_extractor_t* fe) { return fe && plan_trainable(fe) ? 1 : 0; }

size_t orbit_extractor_tape_bytes(const orbit_extractor_t* fe, int B) {
    if (!fe || B <= 0 || !plan_trainable(fe)) return 0;
    return tape_layout(fe, B).total;
}

size_t orbit_extractor_backward_workspace_bytes(const orbit_extractor_t* fe, int B) {
    if (!fe || B <= 0 || !plan_trainable(fe)) return 0;
    return bwd_layout(fe, B).total;
}

size_t orbit_extractor_grad_floats(const orbit_extractor_t* fe) { return fe ? fe->pool.pool_floats : 0; }
size_t orbit_extractor_param_offset(const orbit_extractor_t* fe, int i) {
    return (fe && i >= 0 && i < fe->pool.size()) ? fe->pool.off(i) : 0;
}
size_t orbit_extractor_bn_stat_floats(const orbit_extractor_t* fe) { return fe ? fe->fold_floats : 0; }

int orbit_extractor_export_bn_stats(orbit_extractor_t* fe, float* dst, orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && dst, "extractor_export_bn_stats: null pointer");
    if (!fe->finalized) return set_err(ORBIT_ERR_STATE, "extractor_export_bn_stats: plan is not finalized");
    bn_export_kernel<<<dim3((unsigned)fe->bns.size(), 2), 256, 0, (hipStream_t)stream>>>(fe->d_bn, fe->pool.d_pool, dst,
                                                                                        fe->fold_floats);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

int orbit_extractor_train_forward(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                                  const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                                  size_t tape_bytes, orbit_stream_t stream) {
    return orbit_extractor_train_forward_ex(fe, frames, B, film_gamma, film_beta, bn_train, momentum, feats, tape, tape_bytes,
                                            0, stream);
}

int orbit_extractor_train_forward_ex(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                                     const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                                     size_t tape_bytes, int flags, orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && frames && feats && tape, "extractor_train_forward: null pointer");
    ORBIT_REQUIRE((flags & ~(ORBIT_TRAIN_NO_BACKWARD | ORBIT_TRAIN_DEFER_RUNNING_STATS)) == 0,
                  "extractor_train_forward: unknown flags %d", flags);
    const bool no_backward = (flags & ORBIT_TRAIN_NO_BACKWARD) != 0;
    const bool defer_stats = (flags & ORBIT_TRAIN_DEFER_RUNNING_STATS) != 0;
    ORBIT_REQUIRE(B > 0, "extractor_train_forward: empty batch");
    if (!fe->finalized) return set_err(ORBIT_ERR_STATE, "extractor_train_forward: call orbit_extractor_finalize first");
    if (!plan_trainable(fe))
        return set_err(ORBIT_ERR_STATE, "extractor_train_forward: the %s plan has no training path yet", fe->name.c_str());
    if (bn_train && plan_frozen_only(fe))
        return set_err(ORBIT_ERR_STATE,
                       "extractor_train_forward: the %s plan trains in frozen form only (running statistics, FiLM / BatchNorm "
                       "gradients): batch statistics and filter gradients are not built for it",
                       fe->name.c_str());
    ORBIT_REQUIRE((film_gamma == nullptr) == (film_beta == nullptr),
                  "extractor_train_forward: film_gamma and film_beta must be given together");
    const TapeLayout L = tape_layout(fe, B);
    ORBIT_REQUIRE(tape_bytes >= L.total, "extractor_train_forward: tape too small (%zu < %zu bytes)", tape_bytes, L.total);
    ORBIT_REQUIRE(((uintptr_t)tape & 255) == 0, "extractor_train_forward: tape must be 256-byte aligned");
    orbit_extractor::TrainGraphKey key;
    memset(&key, 0, sizeof(key));
    key.p[0] = frames, key.p[1] = film_gamma, key.p[2] = film_beta, key.p[3] = feats, key.p[4] = tape;
    key.v[0] = (no_backward ? 3 : 1) /* forward */ + (defer_stats ? 16 : 0), key.v[1] = B, key.v[2] = bn_train;
    memcpy(&key.v[3], &momentum, sizeof(float));
    return fe->run_train_graphed(key, (hipStream_t)stream, [&](hipStream_t s) {
        return train_forward_run(fe, frames, B, film_gamma, film_beta, bn_train, momentum, feats, tape, s, no_backward,
                                 defer_stats);
    });
}

int orbit_extractor_apply_deferred_bn_stats(orbit_extractor_t* fe, const void* tape, size_t tape_bytes, int B, float momentum,
                                            orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && tape && B > 0, "extractor_apply_deferred_bn_stats: null pointer or empty batch");
    if (!fe->finalized) return set_err(ORBIT_ERR_STATE, "extractor_apply_deferred_bn_stats: plan is not finalized");
    const TapeLayout L = tape_layout(fe, B);
    ORBIT_REQUIRE(tape_bytes >= L.total, "extractor_apply_deferred_bn_stats: tape too small (%zu < %zu bytes)", tape_bytes, L.total);
    bn_apply_deferred_kernel<<<dim3((unsigned)fe->bns.size(), 2), 256, 0, (hipStream_t)stream>>>(
        fe->d_bn, fe->pool.d_pool, reinterpret_cast<const float*>(static_cast<const char*>(tape) + L.rstat), fe->fold_floats, momentum);
    ORBIT_LAUNCH_CHECK();
    // the static fold follows the running statistics this call just changed (the deferred forward skipped its own re-fold)
    bn_fold_all_kernel<<<dim3((unsigned)fe->bns.size(), 2), 256, 0, (hipStream_t)stream>>>(
        fe->d_bn, fe->pool.d_pool, nullptr, nullptr, fe->d_fold, fe->d_fold + fe->fold_floats);
    ORBIT_LAUNCH_CHECK();
    return ORBIT_OK;
}

}  // extern "C"

static int train_forward_run(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                             const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                             hipStream_t s, bool no_backward, bool defer_stats) {
    const TapeLayout L = tape_layout(fe, B);
    char* tp = static_cast<char*>(tape);
    auto fl = [&](size_t off) { return reinterpret_cast<float*>(tp + off); };
    // deferred running statistics: the finalize kernels run their update with momentum 1 (the statistics replace the slot's
    // content, which is never read) on a slot of the tape instead of on the plan's running statistics;
    // orbit_extractor_apply_deferred_bn_stats applies the real update later - so this forward may overlap, on another stream,
    // with a forward that updates them
    defer_stats = defer_stats && bn_train;
    if (defer_stats) momentum = 1.0f;
    const bool film = film_gamma && fe->film_size > 0;
    auto param = [&](int k) { return fe->param(k); };
    // a layer's slice of the fold arrays on the tape, and the inputs of its train-mode finalize
    auto fold = [&](const BNDesc& bn) {
        return BnFold{fl(L.mean) + bn.fold_off, fl(L.invstd) + bn.fold_off, fl(L.scale) + bn.fold_off, fl(L.shift) + bn.fold_off};
    };
    auto affine = [&](const BNDesc& bn) {
        const bool fm = film && bn.film_off >= 0;
        BnAffine a;
        a.gamma = fm ? film_gamma + bn.film_off : param(bn.gamma), a.beta = fm ? film_beta + bn.film_off : param(bn.beta);
        a.conv_bias = bn.conv_bias >= 0 ? param(bn.conv_bias) : nullptr;
        a.running_mean = defer_stats ? fl(L.rstat) + bn.fold_off : param(bn.mean);
        a.running_var = defer_stats ? fl(L.rstat) + fe->fold_floats + bn.fold_off : param(bn.var);
        a.eps = bn.eps, a.momentum = momentum;
        return a;
    };
    if (!bn_train) {
        dim3 grid((unsigned)fe->bns.size(), 2);
        bn_fold_all_kernel<<<grid, 256, 0, s>>>(fe->d_bn, fe->pool.d_pool, film ? film_gamma : nullptr,
                                                film ? film_beta : nullptr, fl(L.scale), fl(L.shift));
        ORBIT_LAUNCH_CHECK();
        bn_eval_stats_kernel<<<grid, 256, 0, s>>>(fe->d_bn, fe->pool.d_pool, fl(L.mean), fl(L.invstd));
        ORBIT_LAUNCH_CHECK();
    }
    const TrainForms F = train_forms(fe, B, bn_train, no_backward);
    std::map<int, const float*> cur;  // buffer id -> tensor currently held
    cur[-1] = frames;
    for (size_t i = 0; i < fe->ops.size(); ++i) {
        const Op& o = fe->ops[i];
        const OpForm& f = F[i];
        int rc = ORBIT_OK;
        if (o.kind == OP_CONV) {
            const BNDesc& bn = fe->bns[o.bn];
            const BnFold bf = fold(bn);
            const float* xin = cur[o.in];
            if (f.conv == CONV_SWEEP_GRAM) {
                rc = launch_bn_stats_from_gram(xin, B * o.H * o.W, o.Cin, param(o.weight), o.Cout, affine(bn), bf, fl(L.partial), s);
                if (rc != ORBIT_OK) return rc;
                cur[o.out] = nullptr;  // the fused front below re-expands in LDS
                continue;
            }
            ConvDesc d = o.conv_desc(B);
            d.act = ORBIT_ACT_NONE, d.pool2 = 0, d.res_post = 0;  // the raw conv: its epilogue is ops of their own here (but CONV_DUAL)
            d.x = xin, d.w_packed = fe->d_packed + o.packed_off, d.y = fl(L.y[i]);
            // squeeze-excite: the projection multiplies the gate into its A operand on the fly (as the inference plan does)
            if (o.use_gate) d.gate = cur[BUF_GATE];
            int stat_blocks = 0;  // train-mode BatchNorm: column sums of the raw outputs come from the conv's epilogue
            if (bn_train) d.stats = fl(L.partial), d.stats_blocks = &stat_blocks;
            if (f.conv == CONV_DUAL) {
                d.y_raw = fl(L.y[i]), d.y = fl(L.a[i]);
                d.scale = bf.scale, d.shift = bf.shift;
                d.residual = o.res >= 0 ? cur[o.res] : nullptr;
                d.act = o.act;
            }
            if (f.conv == CONV_SWEEP_CONV) d.y = nullptr, d.stats_only = true;
            rc = launch_conv(d, s);
            if (rc != ORBIT_OK) return rc;
            if (f.conv == CONV_DUAL) {
                cur[o.out] = fl(L.a[i]);
                continue;
            }
            if (f.conv == CONV_SWEEP_CONV && stat_blocks <= 0)
                return set_err(ORBIT_ERR_STATE, "extractor_train_forward: the statistics sweep of op %zu emitted no partials", i);
            const int M = B * o.Ho * o.Wo;
            if (bn_train) {
                if (stat_blocks > 0)
                    rc = launch_bn_stats_from_partials(fl(L.partial), stat_blocks, M, o.Cout, affine(bn), bf, s);
                else  // (fused pooling / split-K launches do not emit them: the statistics pass of its own)
                    rc = launch_bn_stats(d.y, M, o.Cout, affine(bn), bf, fl(L.partial), s);
                if (rc != ORBIT_OK) return rc;
            }
            if (f.conv == CONV_SWEEP_CONV) {
                cur[o.out] = nullptr;  // the fused front below re-expands in LDS
                continue;
            }
            if (f.conv == CONV_RAW_TO_DW) {
                cur[o.out] = d.y;  // the activated tensor is neither written nor read back
                continue;
            }
            rc = launch_scale_shift_act(d.y, bf.scale, bf.shift, o.res >= 0 ? cur[o.res] : nullptr, o.act, (size_t)M, o.Cout,
                                        fl(L.a[i]), s, o.res_post);
            if (rc != ORBIT_OK) return rc;
            if (o.pool2) {
                rc = launch_maxpool_idx(fl(L.a[i]), fl(L.p[i]), reinterpret_cast<uint8_t*>(tp + L.idx[i]), o.pool2_geom(B), s);
                cur[o.out] = fl(L.p[i]);
            } else {
                cur[o.out] = fl(L.a[i]);
            }
        } else if (o.kind == OP_DWCONV) {
            const BNDesc& bn = fe->bns[o.bn];
            const BnFold bf = fold(bn);
            float* y = fl(L.y[i]);
            // train-mode BatchNorm: the depthwise kernel itself emits the column sums / sums of squares of its raw outputs
            int stat_rows = B * dwconv_se_chunks(o.Ho);
            if (f.front >= 0) {
                // sweep 2 of the fused front: expand (first BatchNorm's batch statistics from the sweep above) + depthwise in
                // one row-streaming kernel, RAW depthwise outputs + their column sums out
                const Op& c = fe->ops[f.front];
                const BnFold f1 = fold(fe->bns[c.bn]);
                rc = launch_mbconv_rows(cur[c.in], param(c.weight), f1.scale, f1.shift, fe->d_packed + o.packed_off, nullptr, nullptr,
                                        y, fl(L.partial), B, c.H, c.W, c.Cin, c.Cout, o.KH, o.stride, o.pad_t, o.pad_l, o.Ho, o.Wo,
                                        s, 0, true);
                stat_rows = B * F[f.front].tiles;
            } else {
                DwInXf in;  // the producing conv's BatchNorm + activation, applied to its RAW output as it is loaded
                if (f.raw_src >= 0) in = in_xf(fold(fe->bns[fe->ops[f.raw_src].bn]), fe->ops[f.raw_src].act);
                rc = launch_dwconv_se(cur[o.in], fe->d_packed + o.packed_off, y, nullptr, nullptr,
                                      bn_train ? fl(L.partial) : nullptr, o.geom(B), ORBIT_ACT_NONE, s, bn_train ? 1 : 0, in);
            }
            if (rc != ORBIT_OK) return rc;
            const int M = B * o.Ho * o.Wo;
            if (bn_train) {
                rc = launch_bn_stats_from_partials(fl(L.partial), stat_rows, M, o.Cout, affine(bn), bf, s);
                if (rc != ORBIT_OK) return rc;
            }
            if (f.pooled)
                rc = launch_scale_shift_act_pool(y, bf.scale, bf.shift, o.act, B, o.Ho * o.Wo, o.Cout, fl(L.a[i]), fl(L.pool), s);
            else
                rc = launch_scale_shift_act(y, bf.scale, bf.shift, nullptr, o.act, (size_t)M, o.Cout, fl(L.a[i]), s);
            cur[o.out] = fl(L.a[i]);
        } else if (o.kind == OP_SE) {
            // squeeze (mean over the depthwise output) + excite MLP -> gate [B][C]
            if (f.se_dw < 0) return set_err(ORBIT_ERR_STATE, "extractor_train_forward: squeeze-excite without a producer");
            const Op& dw = fe->ops[f.se_dw];
            if (F[f.se_dw].pooled) {
                // the inference gate kernel on the partial sums the activation pass left; the pooled means it forms go on the
                // tape (the gate MLP's backward reads them)
                rc = launch_se_gate2(fl(L.pool), se_pool_chunks(B, dw.Ho * dw.Wo, o.Cin), dw.Ho * dw.Wo, param(o.se_w1),
                                     param(o.se_b1), fe->d_packed + o.packed_off, param(o.se_b2), fl(L.a[i]), B, o.Cin, o.R, s,
                                     fl(L.p[i]));
            } else {
                rc = launch_colmean(fl(L.a[f.se_dw]), fl(L.p[i]), B, dw.Ho * dw.Wo, o.Cin, s);
                if (rc != ORBIT_OK) return rc;
                // the inference gate kernel, fed with the means as a single "partial sum" over one element
                rc = launch_se_gate2(fl(L.p[i]), 1, 1, param(o.se_w1), param(o.se_b1), fe->d_packed + o.packed_off,
                                     param(o.se_b2), fl(L.a[i]), B, o.Cin, o.R, s);
            }
            cur[BUF_GATE] = fl(L.a[i]);
        } else if (o.kind == OP_MAXPOOL) {
            rc = launch_maxpool_idx(cur[o.in], fl(L.p[i]), reinterpret_cast<uint8_t*>(tp + L.idx[i]), o.geom(B), s);
            cur[o.out] = fl(L.p[i]);
        } else {  // OP_AVGPOOL
            rc = launch_avgpool(cur[o.in], feats, B, o.H * o.W, o.Cin, s);
        }
        if (rc != ORBIT_OK) return rc;
    }
    if (bn_train && !defer_stats) {
        // the forward plans fold the running statistics at finalize time: refresh the static fold and drop graphs. (A forward
        // with deferred running statistics did not change them and may run beside a forward that does: it must neither read
        // d_pool's statistics nor write the plan-owned d_fold here - orbit_extractor_apply_deferred_bn_stats re-folds after
        // the join)
        dim3 grid((unsigned)fe->bns.size(), 2);
        bn_fold_all_kernel<<<grid, 256, 0, s>>>(fe->d_bn, fe->pool.d_pool, nullptr, nullptr, fe->d_fold,
                                                fe->d_fold + fe->fold_floats);
        ORBIT_LAUNCH_CHECK();
    }
    return ORBIT_OK;
}

// ---- the reverse pass -----------------------------------------------------------------------------------------------------
// One object per call: the views of the tape and the workspace, the gradient-slot pool, what the pass knows about every op and
// the two job lists of the batched end-of-pass launches; run() walks the ops backwards and calls one step per kind. Runs inside
// stream capture (run_train_graphed): nothing here allocates on the device, synchronises or reads back, and the job lists travel
// as by-value kernel arguments.
struct BackwardPass {
    orbit_extractor_t* fe;  // the call's arguments
    const float *frames, *film_gamma, *film_beta, *dfeats;
    float *param_grads, *dfilm_gamma, *dfilm_beta;
    int B, bn_train;
    hipStream_t s;
    // wg false (filter_grads == 0): only the BatchNorm weight / bias gradients are wanted (FiLM fine-tuning of a frozen extractor,
    // few_shot_recognisers.py:196-199): skip every filter / squeeze-excite / bias gradient
    // se_per_block (A/B and parity runs): every squeeze-excite block sums its parameter gradients in a launch of its own
    const bool film, wg, se_per_block;
    const TapeLayout L;
    const BwdLayout W;
    const Producers P;
    const TrainForms F;
    const char* tp;
    char* ws;
    float *up, *wgrad_scratch, *partial;
    int first_needed;  // the earliest op whose backward yields something that was asked for

    struct OpState {
        int slot = -1;  // the slot holding the gradient w.r.t. the OUTPUT tensor of the op, or -1
        // > 0: that slot already holds g = d out * act'(.) and `partial` the [n][2][C] sums of the op's BatchNorm backward
        // (written by the squeeze-excite backward of the block, launch_se_gate_backward with SeBnFuse, or - for the expansion
        // convolution - by the data gradient of the depthwise convolution it feeds, DwBnBwd)
        int pre_reduced = 0;
        // ... and when the squeeze-excite backward left only the SUMS (gate != nullptr): the slot holds d(x * gate) and g is
        // rebuilt in the BatchNorm's apply pass from it, the gate and the pooled-branch gradient (launch_bn_backward_reduced_gated)
        const float *gate = nullptr, *dpooled = nullptr;
        int HW = 0;
    };
    std::vector<OpState> st;
    bool used[BwdLayout::NSLOTS] = {false};
    // the batched end-of-pass launches: the split reductions of the dense filter gradients, the parameter gradients of the
    // squeeze-excite blocks. Every layer owns its scratch region (BwdLayout) and nothing in the pass reads the reduced gradients,
    // so a full list is flushed with a launch of its own and goes on collecting (efficientnet_v2_s: 80 dense convs, 30 blocks).
    WgradReduceJobs wg_jobs;
    int n_wg_jobs = 0;
    SeParamJobs se_jobs;
    int n_se_jobs = 0;

    BackwardPass(orbit_extractor_t* fe_, const float* frames_, int B_, const float* film_gamma_, const float* film_beta_,
                 int bn_train_, const float* dfeats_, const void* tape, float* param_grads_, int filter_grads,
                 float* dfilm_gamma_, float* dfilm_beta_, void* workspace, hipStream_t s_)
        : fe(fe_), frames(frames_), film_gamma(film_gamma_), film_beta(film_beta_), dfeats(dfeats_), param_grads(param_grads_),
          dfilm_gamma(dfilm_gamma_), dfilm_beta(dfilm_beta_), B(B_), bn_train(bn_train_), s(s_),
          film(film_gamma_ && film_beta_ && fe_->film_size > 0), wg(param_grads_ != nullptr && filter_grads != 0),
          se_per_block(filter_grads == ORBIT_FILTER_GRADS_SE_PER_BLOCK), L(tape_layout(fe_, B_)), W(bwd_layout(fe_, B_)),
          P(producers(fe_)), F(train_forms(fe_, B_, bn_train_, false)), tp(static_cast<const char*>(tape)),
          ws(static_cast<char*>(workspace)), up(wsf(W.up)), wgrad_scratch(wsf(W.wgrad)), partial(wsf(W.partial)),
          st(fe_->ops.size()) {
        const int n = (int)fe->ops.size();
        first_needed = n;
        for (int i = 0; i < n && first_needed == n; ++i) {
            const Op& o = fe->ops[i];
            if (!has_bn(o)) continue;
            if (param_grads || (dfilm_gamma && fe->bns[o.bn].film_off >= 0)) first_needed = i;
        }
    }

    const float* tf(size_t off) const { return reinterpret_cast<const float*>(tp + off); }
    const uint8_t* tidx(int i) const { return reinterpret_cast<const uint8_t*>(tp + L.idx[i]); }
    float* wsf(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    float* slot_ptr(int k) const { return wsf(W.slots + (size_t)k * W.slot_bytes); }
    float* pgrad(int param) const { return param_grads + fe->pool.off(param); }
    const BNDesc& bn_of(int i) const { return fe->bns[fe->ops[i].bn]; }
    const float* out_tensor(int i) const {  // forward output of op i
        if (i < 0) return frames;
        const Op& o = fe->ops[i];
        if (o.kind == OP_CONV) return o.pool2 ? tf(L.p[i]) : tf(L.a[i]);
        if (o.kind == OP_DWCONV) return tf(L.a[i]);
        return tf(L.p[i]);
    }
    // a layer's slice of the fold arrays on the tape; the gamma its forward used (FiLM's or the plan's) with the matching places
    // of its gradients
    BnFoldC fold(const BNDesc& bn) const {
        return BnFoldC{tf(L.mean) + bn.fold_off, tf(L.invstd) + bn.fold_off, tf(L.scale) + bn.fold_off, tf(L.shift) + bn.fold_off};
    }
    BnGrads grads(const BNDesc& bn) const {
        const bool fm = film && bn.film_off >= 0;
        BnGrads p;
        p.gamma = fm ? film_gamma + bn.film_off : fe->param(bn.gamma);
        if (fm) {
            if (dfilm_gamma) p.dgamma = dfilm_gamma + bn.film_off, p.dbeta = dfilm_beta + bn.film_off;
        } else if (param_grads) {
            p.dgamma = pgrad(bn.gamma), p.dbeta = pgrad(bn.beta);
        }
        if (wg && bn.conv_bias >= 0) p.dbias = pgrad(bn.conv_bias);
        return p;
    }
    // the gradient slots: take() hands out the lowest free one, or -1 with the error set
    int take() {
        for (int k = 0; k < BwdLayout::NSLOTS; ++k)
            if (!used[k]) {
                used[k] = true;
                return k;
            }
        set_err(ORBIT_ERR_STATE, "extractor_backward: gradient slots exhausted");
        return -1;
    }
    void release(int k) {
        if (k >= 0) used[k] = false;
    }
    // the gradient of op i's output is consumed: its slot returns to the pool
    void consumed(int i) { release(st[i].slot), st[i].slot = -1; }
    // the next free job of each list, after the flush of a full one
    int next_wgrad_job(WgradReduceJob** job) {
        if (n_wg_jobs == WGRAD_REDUCE_JOBS) {
            if (int rc = launch_conv_wgrad_reduce_batched(wg_jobs, n_wg_jobs, s)) return rc;
            n_wg_jobs = 0;
        }
        *job = &wg_jobs.j[n_wg_jobs++];
        return ORBIT_OK;
    }
    int next_se_job(SeParamJob** job) {
        if (n_se_jobs == SE_PARAM_JOBS) {
            if (int rc = launch_se_param_grad_batched(se_jobs, n_se_jobs, s)) return rc;
            n_se_jobs = 0;
        }
        *job = &se_jobs.j[n_se_jobs++];
        return ORBIT_OK;
    }

    int run() {
        for (int i = (int)fe->ops.size() - 1; i >= first_needed; --i) {
            int rc = ORBIT_OK;
            switch (fe->ops[i].kind) {
            case OP_AVGPOOL: rc = avgpool(i); break;
            case OP_MAXPOOL: rc = maxpool(i); break;
            case OP_DWCONV: rc = dwconv(i); break;
            case OP_CONV: rc = conv(i); break;
            default: break;  // OP_SE: handled together with the gated convolution that consumes the gate
            }
            if (rc != ORBIT_OK) return rc;
        }
        if (int rc = launch_conv_wgrad_reduce_batched(wg_jobs, n_wg_jobs, s)) return rc;
        return launch_se_param_grad_batched(se_jobs, n_se_jobs, s);
    }

    int avgpool(int i) {
        const Op& o = fe->ops[i];
        const int src = P.in[i];
        if (src < first_needed) return ORBIT_OK;
        ORBIT_REQUIRE(st[src].slot < 0, "extractor_backward: unexpected fan-out into the global pool");
        if ((st[src].slot = take()) < 0) return ORBIT_ERR_STATE;
        return launch_avgpool_bwd(dfeats, slot_ptr(st[src].slot), B, o.H * o.W, o.Cin, s);
    }

    int maxpool(int i) {
        const int src = P.in[i], g = st[i].slot;
        if (g < 0) return ORBIT_OK;
        if (src >= first_needed) {
            ORBIT_REQUIRE(st[src].slot < 0, "extractor_backward: unexpected fan-out into a max-pool");
            if ((st[src].slot = take()) < 0) return ORBIT_ERR_STATE;
            if (int rc = launch_maxpool_bwd(slot_ptr(g), tidx(i), slot_ptr(st[src].slot), fe->ops[i].geom(B), s)) return rc;
        }
        consumed(i);
        return ORBIT_OK;
    }

    // BatchNorm (+ activation, + residual fan-out) of op i: g = the gradient of its output, dy (nullable: reductions only)
    // receives the gradient of the raw conv output. `partial` holds [blocks][2][C] followed by the 3*C apply coefficients.
    int bn_backward(int i, const float* g, float* dy, const BnGrads& bp, float* dres, int dres_acc) {
        const Op& o = fe->ops[i];
        const BnFoldC bf = fold(bn_of(i));
        const int M = B * o.Ho * o.Wo, pre = st[i].pre_reduced;
        if (pre > 0) {
            float* coef = partial + bn_partial_floats((size_t)pre, o.Cout);
            if (st[i].gate)
                return launch_bn_backward_reduced_gated(g, st[i].gate, st[i].dpooled, st[i].HW, BnTaped{tf(L.y[i]), bf, o.act, partial},
                                                        bp, bn_train, M, o.Cout, dy, pre, coef, s);
            return launch_bn_backward_reduced(g, tf(L.y[i]), bf, bp, bn_train, M, o.Cout, dy, partial, pre, coef, s);
        }
        float* coef = partial + (size_t)bn_reduce_blocks(M, o.Cout) * 2 * o.Cout;
        return launch_bn_backward(g, tf(L.a[i]), tf(L.y[i]), bf, bp, bn_train, o.act, M, o.Cout, dy, dres, dres_acc, partial, coef, s,
                                  o.res_post);
    }

    // the filter gradient of depthwise op i in a launch of its own (dy: the gradient of its raw output)
    int dw_filter_gradient(int i, const float* dy) {
        const Op& o = fe->ops[i];
        const int src = P.in[i];
        if (F[i].raw_src < 0) return launch_dwconv_wgrad(out_tensor(src), dy, pgrad(o.weight), wgrad_scratch, o.geom(B), s);
        // the forward never wrote this layer's input: the filter gradient rebuilds it from the producing conv's raw output as it
        // stages its patch
        return launch_dwconv_wgrad(tf(L.y[src]), dy, pgrad(o.weight), wgrad_scratch, o.geom(B), s,
                                   in_xf(fold(bn_of(src)), fe->ops[src].act));
    }

    int dwconv(int i) {
        const Op& o = fe->ops[i];
        const int g = st[i].slot;
        if (g < 0) return ORBIT_OK;
        const int src = P.in[i];
        const bool need_dx = src >= first_needed;
        const bool need_dy = need_dx || wg;
        const int kdy = need_dy ? take() : -1;
        if (need_dy && kdy < 0) return ORBIT_ERR_STATE;
        float* dy = need_dy ? slot_ptr(kdy) : nullptr;
        if (int rc = bn_backward(i, slot_ptr(g), dy, grads(bn_of(i)), nullptr, 0)) return rc;
        consumed(i);
        // the producer is a convolution + BatchNorm + SiLU right before this layer (see the data gradient below); on the stride-2
        // layers and the large 3x3 maps the filter gradient rides on that data-gradient kernel (train_forms decides both)
        const bool through_act = need_dx && F[i].through_act;
        const bool wg_fused = wg && need_dx && F[i].wgrad_rides;
        if (wg && !wg_fused)
            if (int rc = dw_filter_gradient(i, dy)) return rc;
        if (need_dx) {
            ORBIT_REQUIRE(st[src].slot < 0, "extractor_backward: unexpected fan-out into a depthwise convolution");
            const int k = st[src].slot = take();
            if (k < 0) return ORBIT_ERR_STATE;
            // wgrad_scratch is free again here (the weight-gradient launches above are earlier on the stream)
            // through_act: the data gradient goes through the producer's activation in the same kernel and leaves the channel
            // sums of that BatchNorm's backward, so the convolution's own backward starts at the finalize step (no reduction
            // pass over dx and y)
            int nblk = 0, wrows = 0;
            DwBnBwd bnb;
            if (through_act) {
                if (wg_fused)
                    bnb.wgrad_partial = wgrad_scratch + dwconv_bwd_fused_partial_offset(o.Cin, o.KH), bnb.wgrad_rows = &wrows;
                bnb.y = tf(L.y[src]), bnb.bn = fold(bn_of(src)), bnb.act = fe->ops[src].act;
                bnb.partial = partial, bnb.nblk = &nblk;
            }
            if (int rc = launch_dwconv_dgrad(dy, fe->d_packed + o.packed_off, slot_ptr(k), o.geom(B), s, wgrad_scratch,
                                             through_act ? &bnb : nullptr))
                return rc;
            if (through_act) st[src].pre_reduced = nblk;  // 0: that kernel form has no such epilogue, the slot holds plain dx
            if (wg_fused) {
                const int rc = wrows > 0 ? launch_dwconv_wgrad_reduce(bnb.wgrad_partial, wrows, o.KH, o.Cin, pgrad(o.weight), s)
                                         : dw_filter_gradient(i, dy);
                if (rc != ORBIT_OK) return rc;
            }
        }
        release(kdy);
        return ORBIT_OK;
    }

    int conv(int i) {
        const Op& o = fe->ops[i];
        int g = st[i].slot;
        if (g < 0) return ORBIT_OK;  // no gradient reaches this op
        if (o.pool2) {
            const int k = take();
            if (k < 0) return ORBIT_ERR_STATE;
            if (int rc = launch_maxpool_bwd(slot_ptr(g), tidx(i), slot_ptr(k), o.pool2_geom(B), s)) return rc;
            release(g), g = st[i].slot = k;
        }
        // BatchNorm (+ReLU, + residual fan-out)
        const BnGrads bp = grads(bn_of(i));
        float* dres = nullptr;
        int dres_acc = 0;
        const int rsrc = o.res >= 0 ? P.res[i] : -1;
        if (rsrc >= first_needed) {
            dres_acc = st[rsrc].slot >= 0;
            if (!dres_acc && (st[rsrc].slot = take()) < 0) return ORBIT_ERR_STATE;
            dres = slot_ptr(st[rsrc].slot);
        }
        const int src = P.in[i];
        const bool need_dx = src >= first_needed;
        const bool need_dy = need_dx || wg;
        const int kdy = need_dy ? take() : -1;
        if (need_dy && kdy < 0) return ORBIT_ERR_STATE;
        float* dy = need_dy ? slot_ptr(kdy) : nullptr;
        // (reductions only, but the residual branch would still need g: the apply pass does not run without dy)
        if (!need_dy && dres) return set_err(ORBIT_ERR_STATE, "extractor_backward: residual fan-out without a data gradient");
        ORBIT_REQUIRE(st[i].pre_reduced <= 0 || (!dres && !bp.dbias && !o.pool2),
                      "extractor_backward: pre-reduced BatchNorm with a residual or bias");
        if (int rc = bn_backward(i, slot_ptr(g), dy, bp, dres, dres_acc)) return rc;
        consumed(i);
        if (wg) {
            // a gated projection: d/dW of conv(x * gate) - the gate is multiplied into x inside the kernel. The layer's
            // partial tiles stay in a region of their own: the split reductions of all layers run as ONE launch at the end
            WgradReduceJob* defer = nullptr;
            if (int rc = next_wgrad_job(&defer)) return rc;
            if (int rc = launch_conv_wgrad(out_tensor(src), o.x_nchw, dy, pgrad(o.weight), o.geom(B), wsf(W.cwgrad[i]), s,
                                           o.use_gate ? tf(L.a[P.gate[i]]) : nullptr, defer))
                return rc;
        }
        if (need_dx && o.use_gate) {
            if (int rc = gated_input_gradient(i, dy)) return rc;
        } else if (need_dx) {
            const float* acc = st[src].slot >= 0 ? slot_ptr(st[src].slot) : nullptr;
            if (!acc && (st[src].slot = take()) < 0) return ORBIT_ERR_STATE;
            if (int rc = launch_conv_dgrad(dy, fe->d_dgrad + fe->dgrad_off[i], acc, slot_ptr(st[src].slot), up, o.geom(B), s)) return rc;
        }
        release(kdy);
        return ORBIT_OK;
    }

    // the input side of gated projection i: d(x * gate) = its data gradient, then the squeeze-excite backward (gate MLP + average
    // pool) down to the gradient of x, the activated output of op P.in[i]
    int gated_input_gradient(int i, const float* dy) {
        const Op& o = fe->ops[i];
        const int src = P.in[i], se = P.gate[i];
        ORBIT_REQUIRE(se >= 0 && st[src].slot < 0, "extractor_backward: malformed squeeze-excite block");
        const Op& so = fe->ops[se];
        float* se_scratch = wsf(W.se[se]);  // this block's own (see se_jobs)
        const int kt = take();
        if (kt < 0) return ORBIT_ERR_STATE;
        if (int rc = launch_conv_dgrad(dy, fe->d_dgrad + fe->dgrad_off[i], nullptr, slot_ptr(kt), up, o.geom(B), s)) return rc;
        // the four parameter gradients of the block's MLP: summed over the frames for ALL blocks in one launch at the end of the
        // reverse pass (nothing in it reads them), or by this block's own launch
        const SeGrads dparams = wg ? SeGrads{pgrad(so.se_w1), pgrad(so.se_b1), pgrad(so.se_w2), pgrad(so.se_b2)} : SeGrads{};
        const bool batched = wg && !se_per_block && F[se].se_batched;
        if (batched) {
            SeParamJob* job = nullptr;
            if (int rc = next_se_job(&job)) return rc;
            *job = se_bwd_param_job(se_scratch, tf(L.p[se]), B, o.Cin, so.R, dparams);
        }
        // x = SiLU(BatchNorm(depthwise output)): the first (reduction) pass of that BatchNorm's backward is folded into the last
        // pass of the squeeze-excite backward, which then leaves only the sums - g itself is rebuilt by that BatchNorm's apply
        // pass from d(x * gate) (slot kt stays the depthwise op's gradient slot)
        const bool sums_only = F[i].se_sums_only;
        const int k = st[src].slot = sums_only ? kt : take();
        if (k < 0) return ORBIT_ERR_STATE;
        SeBnFuse fuse;
        const bool dw_src = fe->ops[src].kind == OP_DWCONV;
        if (dw_src) {
            fuse = BnTaped{tf(L.y[src]), fold(bn_of(src)), fe->ops[src].act, partial};
            st[src].pre_reduced = B * se_pool_chunks(B, o.H * o.W, o.Cin);
            if (sums_only)
                st[src].gate = tf(L.a[se]), st[src].dpooled = se_bwd_dpooled(se_scratch, B, o.Cin, so.R), st[src].HW = o.H * o.W;
        }
        const SeWeights w{fe->param(so.se_w1), fe->param(so.se_b1), fe->param(so.se_w2), fe->param(so.se_b2), fe->d_packed + so.packed_off};
        const int rc = launch_se_gate_backward(slot_ptr(kt), out_tensor(src), tf(L.p[se]), tf(L.a[se]), w,
                                               sums_only ? nullptr : slot_ptr(k), wg && !batched ? &dparams : nullptr, se_scratch, B,
                                               o.H * o.W, o.Cin, so.R, s, dw_src ? &fuse : nullptr);
        if (!sums_only) release(kt);
        return rc;
    }
};

extern "C" {

int orbit_extractor_backward(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                             const float* film_beta, int bn_train, const float* dfeats, const void* tape,
                             size_t tape_bytes, float* param_grads, int filter_grads, float* dfilm_gamma,
                             float* dfilm_beta, void* workspace, size_t workspace_bytes, orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && frames && dfeats && tape && workspace, "extractor_backward: null pointer");
    ORBIT_REQUIRE(B > 0, "extractor_backward: empty batch");
    if (!fe->finalized) return set_err(ORBIT_ERR_STATE, "extractor_backward: call orbit_extractor_finalize first");
    if (!plan_trainable(fe))
        return set_err(ORBIT_ERR_STATE, "extractor_backward: the %s plan has no training path yet", fe->name.c_str());
    if ((bn_train || filter_grads) && plan_frozen_only(fe))
        return set_err(ORBIT_ERR_STATE,
                       "extractor_backward: the %s plan trains in frozen form only (running statistics, FiLM / BatchNorm "
                       "gradients): batch statistics and filter gradients are not built for it",
                       fe->name.c_str());
    ORBIT_REQUIRE((dfilm_gamma == nullptr) == (dfilm_beta == nullptr),
                  "extractor_backward: dfilm_gamma and dfilm_beta must be given together");
    const bool film = film_gamma && film_beta && fe->film_size > 0;
    ORBIT_REQUIRE(!dfilm_gamma || film, "extractor_backward: FiLM gradients requested without FiLM inputs");
    if (!param_grads && !dfilm_gamma) return ORBIT_OK;  // nothing to compute
    const TapeLayout L = tape_layout(fe, B);
    const BwdLayout W = bwd_layout(fe, B);
    ORBIT_REQUIRE(tape_bytes >= L.total, "extractor_backward: tape too small");
    ORBIT_REQUIRE(workspace_bytes >= W.total, "extractor_backward: workspace too small (%zu < %zu bytes)", workspace_bytes,
                  W.total);
    ORBIT_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)tape & 255) == 0,
                  "extractor_backward: tape and workspace must be 256-byte aligned");
    // the dgrad-packed filters follow the parameters: repacked OUTSIDE any captured graph whenever they changed
    if (int rc = ensure_dgrad_filters(fe, (hipStream_t)stream)) return rc;
    orbit_extractor::TrainGraphKey key;
    memset(&key, 0, sizeof(key));
    key.p[0] = frames, key.p[1] = film_gamma, key.p[2] = film_beta, key.p[3] = dfeats, key.p[4] = tape;
    key.p[5] = param_grads, key.p[6] = dfilm_gamma, key.p[7] = dfilm_beta, key.p[8] = workspace;
    key.v[0] = 2 /* backward */, key.v[1] = B, key.v[2] = bn_train, key.v[3] = filter_grads;
    return fe->run_train_graphed(key, (hipStream_t)stream, [&](hipStream_t s) {
        return BackwardPass(fe, frames, B, film_gamma, film_beta, bn_train, dfeats, tape, param_grads, filter_grads, dfilm_gamma,
                            dfilm_beta, workspace, s)
            .run();
    });
}

// diagnostics: how many training-entry calls of this plan replayed a captured graph / ran eagerly
int orbit_extractor_train_graph_stats(const orbit_extractor_t* fe, long* replays, long* eager) {
    ORBIT_REQUIRE(fe, "extractor_train_graph_stats: null pointer");
    if (replays) *replays = fe->train_graph_replays;
    if (eager) *eager = fe->train_graph_eager;
    return ORBIT_OK;
}

}  // extern "C"
