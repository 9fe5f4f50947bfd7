/*
 * orbit_hip.h — C-ABI of liborbit_hip.so: the MI355X (gfx950) implementation of ORBIT's episodic
 * few-shot recognition hot path (FewShotRecogniser.personalise()/predict()).
 *
 * The reference (microsoft/ORBIT-Dataset) is pure Python/PyTorch and has no FFI of its own; the seam
 * this library replaces is the ATen op sequence under these reference call sites (file:line are
 * relative to the reference tree):
 *
 *   orbit_proto_configure / _finalize   model/classifier_heads.py:94-119 (_build_class_reps),
 *                                        :232-263 (PrototypicalClassifier.configure)
 *   orbit_proto_predict                  model/classifier_heads.py:202-230 (PrototypicalClassifier.predict)
 *   orbit_mean_pool                      model/poolers.py:7-16 (MeanPooler.forward)
 *   orbit_extractor_*                    model/feature_extractors.py:37-79 (create_feature_extractor) and
 *                                        model/few_shot_recognisers.py:99-153 (_get_features[_in_batches]);
 *                                        "set_encoder": model/set_encoders.py:81-120 (SimplePrePoolNet)
 *   film_gamma / film_beta arguments     model/few_shot_recognisers.py:114-115,143-144
 *                                        (functional_call with the FiLM dict), model/film.py:38-94
 *   orbit_set_mean                       model/set_encoders.py:61-75 (SetEncoder.aggregate 'mean')
 *   orbit_filmgen_*                      model/feature_adapters.py:36-78 (FilmParameterGenerator),
 *                                        model/mlps.py:52-63 (DenseBlock)
 *   orbit_vit_*                          model/feature_extractors.py:49-63 (vit_s_32, vit_b_32, vit_b_32_clip: timm
 *                                        0.6.12 VisionTransformer, num_classes=0), inference only; FiLM on the
 *                                        LayerNorms model/film.py:57-66
 *   orbit_op_*                           single operators (conv/pool/depthwise/SE) exposed for parity tests
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer to contiguous memory owned by the caller (fp32 unless stated,
 *     labels int64). The library never frees or retains caller memory past the call.
 *   - `stream` is a hipStream_t passed as void*. Calls only enqueue work and return immediately.
 *   - return 0 on success, negative on error; orbit_last_error() returns a thread-local message.
 *   - the library uses the calling thread's current HIP device; handles belong to the device they were
 *     created on. One process per GPU is the intended deployment.
 *   - no global mutable state besides the thread-local error string.
 */
#ifndef ORBIT_HIP_H
#define ORBIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orbit_extractor orbit_extractor_t;
typedef struct orbit_filmgen orbit_filmgen_t;
typedef struct orbit_vit orbit_vit_t;
typedef void* orbit_stream_t; /* hipStream_t */

#define ORBIT_OK 0
#define ORBIT_ERR_ARG (-1)
#define ORBIT_ERR_HIP (-2)
#define ORBIT_ERR_STATE (-3)
#define ORBIT_ERR_NOMEM (-4)

#define ORBIT_ACT_NONE 0
#define ORBIT_ACT_RELU 1
#define ORBIT_ACT_SILU 2
#define ORBIT_ACT_ELU 3   /* alpha = 1; only orbit_dense_rows */

#define ORBIT_REDUCE_NONE 0
#define ORBIT_REDUCE_MEAN 1
#define ORBIT_REDUCE_SUM 2

/* ---- library ---------------------------------------------------------------------------------- */
int orbit_version(void);
/* Call once per device before the first launch (idempotent): freed stream-ordered scratch stays in the device's default
 * memory pool instead of being returned - and synchronously re-allocated - around every task. */
int orbit_runtime_init(void);
const char* orbit_last_error(void);
/* number of visible HIP devices (<=0: no usable GPU); does not create a context on failure */
int orbit_device_count(void);
/* Runtime options (15). Every option has an environment default ORBIT_<NAME in upper case>; the defaults are the measured-best
 * path. They exist so that the parity tests can reach every kernel a default path uses and so that A/B comparisons run
 * inside one process on one box. Setting an option bumps an epoch that invalidates captured launch sequences.
 *  network runtime:
 *   "graph"         HIP-graph replay of extractor forwards: 0 = never, 1 = always, 2 = adaptive (default: only while an
 *                   eager kernel launch costs > ~12 us of host time on this host); read per forward
 *   "train_graph"   1 (default) = the training entry points (orbit_extractor_train_forward / _backward) replay captured HIP
 *                   graphs from the second sight of a call on (same pointers, same sizes; the first runs eagerly); 0 = eager launches
 *   "mbconv_rows"   1 (default) = EfficientNet blocks 1.0 .. 3.0 (112x112 .. 28x28 maps) run the row-streaming fused front
 *                   (csrc/mbconv_rows.hip: expand 1x1 + BN + SiLU + depthwise + BN + SiLU + SE partials, expanded rows in an
 *                   LDS ring); 0 = conv + depthwise kernel pair everywhere. Read when a plan is created
 *   "stem_rows"     1 (default) = conv_stem + BN + SiLU + the first depthwise as one row-streaming kernel; 0 = direct stem
 *                   kernel + depthwise kernel. Read when a plan is created
 *   "train_dw_xf"   1 (default) = ORBIT_TRAIN_NO_BACKWARD forwards skip the activation pass between an expand / stem conv and
 *                   its depthwise conv (applied on load instead); 0 = always the separate pass
 *   "train_fused_fronts"  1 (default) = on ORBIT_TRAIN_NO_BACKWARD batch-statistics forwards (the LITE cache pass) the expansion
 *                   conv + depthwise conv of EfficientNet's 112x112 / 56x56 MBConv blocks run as a statistics sweep of the
 *                   expansion conv (nothing stored) + the row-streaming fused front of the inference plans in its RAW form
 *                   (raw depthwise outputs + their column sums): the 6x-expanded tensor never reaches HBM; 2 = every shape the
 *                   fused front serves; 0 = never (conv + depthwise pair); 3 = as 2, with the first BatchNorm's statistics from a
 *                   statistics sweep of the conv itself (bit-identical to the pair's) instead of the Gram matrix of the block
 *                   input (launch_bn_stats_from_gram: Cin = 16 / 24). Statistics agree to summation order
 *  dense convolutions (csrc/conv_igemm.hip, pw_rgemm.hip, conv_bf3.hip):
 *   "conv_tile"     0 = heuristic (default); 3 = 64x64, 4 = 128x32, 6 = 32x32 with K split over the four waves (the three
 *                   tilings the heuristic chooses from)
 *   "conv_bk"       cap the K-tile width: 0 = widest of 32/16/8 dividing Cin, 16 on the layers where that measured faster
 *                   (default); 8, 16, 32 (read when weights are packed AND at launch: set it before creating / finalizing a plan)
 *   "conv_splitk"   1 (default) = convs with few output tiles and a long reduction are split over K (partial tiles + a
 *                   deterministic reduce), 0 = never
 *   "conv_rgemm"    1 (default) = the barrier-free 16x16x4-MFMA register GEMM on fragment-packed weights serves the stride-1
 *                   pointwise convs for which it is a gain inside the network: projections of at most 8x8 maps from >= 512 to
 *                   more than 256 channels (EfficientNet-B0's 1152 -> 320 at 7x7; a rule on the layer, not on the batch, so a
 *                   frame's bits do not depend on the batch it arrives in); 0 = never; 2 = every conv it supports. Read at plan
 *                   creation (which filters get a fragment-ordered copy) and at launch
 *                   The same switch (!= 0) lets the streaming gated projection (csrc/pw_stream.hip) serve EfficientNet's narrow
 *                   projections (32 -> 16, 96 / 144 -> 24, 144 -> 40; H * W % 16 == 0) with the squeeze-excite gate computed in its prologue,
 *                   instead of a se_gate2 launch + the LDS-tiled conv; 0 = that pair
 *   "conv_bf3"      0 (default) = every product is an fp32 x fp32 MFMA. OPT-IN bits: 1 = dense convs with Cin % 16 == 0,
 *                   Cin >= 64, Cout >= 40 split both operands three ways into bf16 and sum six of the nine bf16 x bf16 products on
 *                   v_mfma_f32_32x32x16_bf16 (csrc/conv_bf3.hip); 2 = the expand GEMM of the row-streaming fused fronts does the
 *                   same; 3 = both. NOT the reference's arithmetic bit for bit - a measured alternative, frozen, never the
 *                   default, never part of bench.py's value
 *  depthwise kernel families (csrc/ops.hip): 1 = where measured faster (default), 0 = never, 2 = wherever it fits
 *   "dw_window"     register-window kernel (default: 3x3, stride 1, >= 14 rows)
 *   "dw_lds"        input patch staged in LDS (default: stride-1 5x5 and small 3x3 maps)
 *   "dw_pipe"       software-pipelined streaming kernel (default: large stride-2 layers)
 *  prototype head (csrc/head.hip):
 *   "head_stream"   1 (default) = the streaming distance kernel (rows requested before the weight staging, 8 waves x 2 rows)
 *                   for T = 1, D = 512 / 1280 launches with >= 64 query rows; 0 = the general LDS-staged kernel */
int orbit_set_option(const char* name, int value);
/* current value of an option (after its environment default was applied), -1 for an unknown name */
int orbit_get_option(const char* name);

/* ---- prototype head ---------------------------------------------------------------------------- */
/* The label set of a task without a host round trip: class_ids[0 .. cap) = the ascending unique values of labels[N] - the
 * logit column order, what the reference takes from torch.unique(context_labels) with an .item() loop
 * (model/classifier_heads.py:96-100,246-248) - slots beyond the count repeat the last value; *count = number of distinct
 * labels, or cap + 1 if there are more than cap. Both outputs are device memory; the caller copies *count to the host
 * whenever it needs it (orbit-dataset_amd/model/classifier_heads.py resolves it on a side stream while the extractor runs). */
int orbit_label_set(const int64_t* labels, int N, int64_t* class_ids, int cap, int32_t* count, orbit_stream_t stream);

/* Per-class sums of per-clip mean-pooled support features.
 *   feats   [n_tasks][N*T][D]   frame features, clip-major (clip i owns rows i*T .. i*T+T-1)
 *   labels  [n_tasks][N]        int64 clip labels
 *   class_ids [n_tasks][C]      int64 ascending unique labels (column order of the logits)
 *   sums    [n_tasks][C][D] out Σ over clips of class c of mean_T(feats)   (all-reduce payload)
 *   counts  [n_tasks][C]    out number of clips of class c (as float)      (all-reduce payload)
 * Summation order per (class, d) is ascending clip index: deterministic. */
int orbit_proto_configure(const float* feats, const int64_t* labels, const int64_t* class_ids,
                          int n_tasks, int N, int T, int D, int C,
                          float* sums, float* counts, orbit_stream_t stream);

/* W[c] = 2*mu_c, b[c] = -mu_c.mu_c with mu_c = sums[c]/counts[c]  (classifier_heads.py:253-255).
 * cosine != 0: b is not written (may be NULL). */
int orbit_proto_finalize(const float* sums, const float* counts, int n_tasks, int C, int D, int cosine,
                         float* W, float* b, orbit_stream_t stream);

/* logits[m][c] = logit_scale * (q_m . W_c + b_c)                       (euclidean, :213)
 *              = logit_scale * cos(q_m, W_c), eps 1e-8 per norm        (cosine, :215-217)
 * with q_m = mean over the T frames of clip m of Q.   Q [n_tasks][M*T][D]; logits [n_tasks][M][C];
 * argmax [n_tasks][M] int32 or NULL (first maximal column, as torch.argmax). */
int orbit_proto_predict(const float* Q, const float* W, const float* b,
                        int n_tasks, int M, int T, int D, int C, float logit_scale, int cosine,
                        float* logits, int32_t* argmax, orbit_stream_t stream);

/* The ORBIT benchmark metrics of one task's target videos in ONE launch (utils/eval_metrics.py:27-69: frame accuracy,
 * frames-to-recognition and video accuracy are functions of the per-frame argmax alone). All pointers are device pointers.
 *   logits        [M][C]   the task's target-frame logits, videos back to back
 *   video_offsets [V+1]    ascending, [0] = 0, [V] = M: video v owns rows offsets[v] .. offsets[v+1]-1 (entries are clamped
 *                          into [0, M] on the device: a bad table gives wrong counts, never an access out of range)
 *   video_labels  [V]      the videos' labels as logit COLUMNS; a label outside [0, C) matches no frame
 *   preds         [M] out  per-frame predicted column, or NULL; the argmax rule is orbit_proto_predict's (first maximal
 *                          column, as torch.argmax - one device function serves both)
 *   correct       [V] out  frames of video v predicted as its label
 *   first_correct [V] out  index inside the video of its first correct frame; n_v when no frame is correct
 *   hist       [V][C] out  frames of video v predicted as class c
 * An empty video writes correct = 0, first_correct = 0 and a zero histogram row. Integer adds and mins only: the outputs
 * are exactly reproducible. M, V >= 0, 1 <= C <= ORBIT_VIDEO_METRICS_MAX_C and non-null pointers (preds excepted) are
 * checked on the host (ORBIT_ERR_ARG, nothing launched); M == 0 or V == 0 is a no-op returning 0. */
#define ORBIT_VIDEO_METRICS_MAX_C 4096
int orbit_video_metrics(const float* logits, int M, int C, const int32_t* video_offsets, const int64_t* video_labels, int V,
                        int32_t* preds, int32_t* correct, int32_t* first_correct, int32_t* hist, orbit_stream_t stream);

/* out[i][d] = mean_t x[i*T+t][d]  (poolers.py:13-16) */
int orbit_mean_pool(const float* x, int N, int T, int D, float* out, orbit_stream_t stream);

/* Clip pooling of a video's sliding windows without duplicating frames: x [F][D] per-frame features, out [F][D] with
 * out[f] = mean_{j<T} x[max(f-T+1+j, 0)] — attach_frame_history (data/utils.py:8-28) + MeanPooler (poolers.py:13-16) on
 * features instead of on frames, bit-identical to pooling the T-times larger clip tensor. */
int orbit_history_mean_pool(const float* x, int F, int T, int D, float* out, orbit_stream_t stream);
/* out[d] = (1/n) Σ_i x[i][d]  (set_encoders.py:70-71; also the LITE concat-mean) */
int orbit_set_mean(const float* x, int n, int D, float* out, orbit_stream_t stream);

/* ---- feature extractors / set encoder ---------------------------------------------------------- */
/* name: "resnet18" | "efficientnet_b0" | "efficientnet_v2_s" | "set_encoder".  H,W: frame size the plan is built for.
 * "efficientnet_v2_s" (timm tf_efficientnetv2_s_in21k, num_classes = 0; 1280-d features) is an inference plan by default: its
 * ConvBnAct blocks add their skip after the activation, and orbit_extractor_supports_training is 0 and the tape /
 * backward-workspace size queries return 0 for it - unless the plan was created with ORBIT_PLAN_RES_POST_BACKWARD (below), which
 * opens the FROZEN training path: FiLM / BatchNorm weight and bias gradients under running statistics, nothing else - or with
 * ORBIT_PLAN_RES_POST_TRAINING, which opens all of the training path (batch statistics, every parameter gradient). */
int orbit_extractor_create(const char* name, int H, int W, orbit_extractor_t** out);
/* flags: ORBIT_PLAN_UNFUSED = a plan for forwards that record a tape or use batch statistics (the LITE training step,
 * few_shot_recognisers.py:176-183): every MBConv block stays a conv + depthwise pair, whose outputs the backward needs;
 * same parameters in the same order as the default plan. */
#define ORBIT_PLAN_UNFUSED 1
/* ORBIT_PLAN_RES_POST_BACKWARD (may be combined with ORBIT_PLAN_UNFUSED; same ops, same parameters in the same order): the
 * training runtime accepts a plan that holds a convolution whose skip joins after the activation ("efficientnet_v2_s";
 * accepted and without effect for every other network). Such a plan trains in frozen form only: orbit_extractor_train_forward(_ex)
 * returns ORBIT_ERR_STATE for bn_train != 0 and orbit_extractor_backward for bn_train != 0 or filter_grads != 0, before any
 * launch - batch-statistics BatchNorm and filter gradients are not built for it. Without the flag the plan reports no training
 * path at all, as before. */
#define ORBIT_PLAN_RES_POST_BACKWARD 2
/* ORBIT_PLAN_RES_POST_TRAINING (implies ORBIT_PLAN_RES_POST_BACKWARD; same ops, same parameters in the same order; accepted and
 * without effect for every other network): the plan that holds a post-activation skip trains like the others -
 * orbit_extractor_train_forward(_ex) accepts bn_train != 0 (batch statistics, running-statistics updates, with
 * ORBIT_TRAIN_NO_BACKWARD and ORBIT_TRAIN_DEFER_RUNNING_STATS as well) and orbit_extractor_backward accepts bn_train != 0 and
 * filter_grads != 0 (reference: the LITE recipe of the efficientnet_v2_s checkpoints, --learn_extractor --with_lite,
 * few_shot_recognisers.py:176-183). A plan created with ORBIT_PLAN_RES_POST_BACKWARD alone keeps the refusals above. */
#define ORBIT_PLAN_RES_POST_TRAINING 4
int orbit_extractor_create_ex(const char* name, int H, int W, int flags, orbit_extractor_t** out);
void orbit_extractor_destroy(orbit_extractor_t* fe);

/* state_dict enumeration: parameter/buffer keys the extractor expects (torch state_dict names). */
int orbit_extractor_num_params(const orbit_extractor_t* fe);
const char* orbit_extractor_param_name(const orbit_extractor_t* fe, int i);
size_t orbit_extractor_param_numel(const orbit_extractor_t* fe, int i);

/* copy one tensor (host or device pointer, fp32, torch layout) into the extractor. */
int orbit_extractor_load(orbit_extractor_t* fe, const char* key, const float* data, size_t numel);
/* Same for a source already resident in HBM: stream-ordered device-to-device copy (no host synchronisation); how the
 * parameters follow optimizer steps during meta-training. */
int orbit_extractor_load_async(orbit_extractor_t* fe, const char* key, const float* device_data, size_t numel,
                               orbit_stream_t stream);
/* All parameters in one launch: device_ptrs[i] = device pointer of parameter i (orbit_extractor_param_name order, fp32,
 * contiguous, orbit_extractor_param_numel(i) elements). The pointer table is cached; one gather kernel copies every
 * tensor into the plan, stream-ordered (what optimizer.step() -> next forward needs every training step: one launch
 * instead of one hipMemcpyAsync per tensor). */
int orbit_extractor_load_all_async(orbit_extractor_t* fe, const float* const* device_ptrs, int n, orbit_stream_t stream);
/* repack conv weights for the kernels, precompute folded BN for the non-FiLM case. Call after loads. */
int orbit_extractor_finalize(orbit_extractor_t* fe, orbit_stream_t stream);

int orbit_extractor_output_size(const orbit_extractor_t* fe);
/* FiLM-tagged BatchNorms in module-traversal order: count, per-slot channel count and module name,
 * total channels (= length of film_gamma / film_beta). */
int orbit_extractor_film_slots(const orbit_extractor_t* fe);
int orbit_extractor_film_slot_channels(const orbit_extractor_t* fe, int slot);
const char* orbit_extractor_film_slot_name(const orbit_extractor_t* fe, int slot);
int orbit_extractor_film_size(const orbit_extractor_t* fe);

size_t orbit_extractor_workspace_bytes(const orbit_extractor_t* fe, int B);
/* multiply-accumulates per frame of the plan (for roofline accounting) */
double orbit_extractor_macs_per_frame(const orbit_extractor_t* fe);

/* frames [B][3][H][W] NCHW fp32 -> feats [B][D].
 * film_gamma/film_beta: NULL, or the per-task BatchNorm weight/bias of every FiLM slot concatenated in
 * slot order (the tensors the reference passes through functional_call). */
int orbit_extractor_forward(orbit_extractor_t* fe, const float* frames, int B,
                            const float* film_gamma, const float* film_beta,
                            float* feats, void* workspace, size_t workspace_bytes, orbit_stream_t stream);

/* ---- vision-transformer feature extractors (csrc/vit.hip) --------------------------------------- */
/* Reference model/feature_extractors.py:49-63 builds timm 0.6.12 `vit_small_patch32_224_in21k` ("vit_s_32"),
 * `vit_base_patch32_224_in21k` ("vit_b_32") and `vit_base_patch32_224_clip_laion2b` ("vit_b_32_clip") with num_classes=0;
 * the feature is LN_final(tokens)[:, 0] (timm forward_head, global_pool='token'). Same semantics as the orbit_extractor_*
 * family (orbit_extractor_create rejects these names). H = W = 224 only (reference utils/args.py: --frame_size 224 for
 * these backbones; the position table is fixed). Creation and enumeration do not touch the device. Inference only by default:
 * orbit_vit_train_forward / orbit_vit_backward below give the gradients of the FiLM vectors of the FROZEN network (the reference's
 * --adapt_features recipes), orbit_vit_backward_params those of every parameter as well (--learn_extractor).
 * Six models: the patch-16 members of the same families - "vit_s_16", "vit_b_16" (timm `vit_small_patch16_224_in21k`,
 * `vit_base_patch16_224_in21k`, named by analogy with the patch-32 ones) and "vit_b_16_clip" (the laion2b CLIP B/16) - have the
 * same module tree, state_dict keys and FiLM slots; patch_embed.proj.weight is [D][3][16][16], pos_embed [1][197][D], and a
 * frame is 196 patches + the class token. They are inference + FiLM only: orbit_vit_tape_bytes,
 * orbit_vit_backward_workspace_bytes and orbit_vit_backward_params_workspace_bytes return 0 and the three training entry points
 * return ORBIT_ERR_ARG naming the model, before any launch or allocation - until orbit_vit_enable_backward (below) opts a plan
 * into the taped forward and the FiLM gradients of the frozen network, and orbit_vit_enable_weight_backward (below) into the
 * gradients of every parameter; without the latter weight gradients stay refused. Batch cap: 1..8192 frames for the patch-32 plans,
 * 1..2048 for the patch-16 plans (B * 197 * 4 D stays below 2^31); beyond it orbit_vit_workspace_bytes returns 0 and
 * orbit_vit_forward ORBIT_ERR_ARG. */
int orbit_vit_create(const char* name, int H, int W, orbit_vit_t** out);
/* Opt-in: the same six models on square frames of another side S = H = W, a multiple of the model's patch size, 32 <= S <= 512
 * (ORBIT_ERR_ARG with the reason otherwise: non-square, not a multiple - naming the two nearest sizes -, below 32, above 512,
 * unknown name). The parameters, their order and their numels are those of orbit_vit_create: pos_embed keeps its checkpoint
 * shape [1][50 | 197][D]. With G = S / patch patches per side and g = 7 | 14, the table the forward adds is row 0 unchanged and
 * rows 1..G^2 = F.interpolate(pos_embed[1:] as [1][D][g][g], size=(G, G), mode="bicubic", align_corners=False): cubic
 * convolution with A = -0.75, source coordinate (i + 0.5) g / G - 0.5, four taps per axis clamped to [0, g - 1], no
 * antialiasing (timm 0.6.12 resize_pos_embed; transformers' interpolate_pos_encoding=True). It is made by the first forward
 * after a parameter upload in a plan-owned [G^2 + 1][D] buffer; every orbit_vit_load* invalidates it, orbit_vit_destroy frees
 * it. Tokens per frame N = G^2 + 1, orbit_vit_macs_per_frame by its formula at that N; batch cap: the largest B with
 * B * N <= 8192 * 50. At S = 224 the plan IS an orbit_vit_create plan: no resampled table, the same kernels with compile-time
 * geometry, the same caps, and the backward entry points on the same terms. At any other S the plan is inference + FiLM only
 * for good: orbit_vit_enable_backward, orbit_vit_enable_weight_backward, orbit_vit_train_forward, orbit_vit_backward and
 * orbit_vit_backward_params return ORBIT_ERR_ARG naming the frame size before any launch or allocation, and the tape / backward
 * workspace size queries return 0. orbit_vit_enable_bf16 is allowed. Attention runs on a streaming fp32 matrix-core kernel for
 * every token count but 50 and 197; a frame's features do not depend on the batch it is in. */
int orbit_vit_create_sized(const char* name, int H, int W, orbit_vit_t** out);
void orbit_vit_destroy(orbit_vit_t* v);
/* timm state_dict keys in timm's order: cls_token, pos_embed, patch_embed.proj.{weight,bias (not CLIP)}, norm_pre.* (CLIP),
 * blocks.{i}.{norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}.{weight,bias}, norm.{weight,bias} */
int orbit_vit_num_params(const orbit_vit_t* v);
const char* orbit_vit_param_name(const orbit_vit_t* v, int i);
size_t orbit_vit_param_numel(const orbit_vit_t* v, int i);
/* as orbit_extractor_load / _load_async / _load_all_async (torch layouts, fp32) */
int orbit_vit_load(orbit_vit_t* v, const char* key, const float* data, size_t numel);
int orbit_vit_load_async(orbit_vit_t* v, const char* key, const float* device_data, size_t numel, orbit_stream_t stream);
int orbit_vit_load_all_async(orbit_vit_t* v, const float* const* device_ptrs, int n, orbit_stream_t stream);
/* checks that every parameter was loaded (the kernels read the torch layouts: nothing is repacked); forward fails before it */
int orbit_vit_finalize(orbit_vit_t* v, orbit_stream_t stream);
int orbit_vit_output_size(const orbit_vit_t* v);
/* FiLM slots (reference model/film.py:57-66: every LayerNorm named norm / norm1 / norm2, not norm_pre): 25 in module order
 * blocks.0.norm1, blocks.0.norm2, ..., blocks.11.norm2, norm; D channels each; film_size = 25 D */
int orbit_vit_film_slots(const orbit_vit_t* v);
int orbit_vit_film_slot_channels(const orbit_vit_t* v, int slot);
const char* orbit_vit_film_slot_name(const orbit_vit_t* v, int slot);
int orbit_vit_film_size(const orbit_vit_t* v);
size_t orbit_vit_workspace_bytes(const orbit_vit_t* v, int B);
/* patch embedding + the four linear layers + QK^T and PV, per frame (N tokens, P = N - 1 patches of 3 p^2 values):
 * P * 3 p^2 * D + 12 * (12 D^2 N + 2 N^2 D) */
double orbit_vit_macs_per_frame(const orbit_vit_t* v);
/* frames [B][3][224][224] NCHW fp32 -> feats [B][D] (model/few_shot_recognisers.py:99-153 with a ViT extractor).
 * film_gamma / film_beta: NULL, or the LayerNorm weight / bias of every FiLM slot concatenated in slot order. */
int orbit_vit_forward(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                      float* feats, void* workspace, size_t workspace_bytes, orbit_stream_t stream);
/* Gradients of the FiLM vectors (LayerNorm gamma / beta of the 25 slots) through the frozen network, fp32, deterministic.
 * orbit_vit_train_forward = orbit_vit_forward (same kernels, same order, bitwise the same feats; workspace of
 * orbit_vit_workspace_bytes) that also fills the caller-owned tape: per block the input stream, qkv, the post-attention stream
 * and the fc1 pre-activation (9 * 50 B * D floats), then the stream entering the final norm (50 B * D floats); LayerNorm
 * statistics are recomputed. orbit_vit_backward: dfeats [B][D] -> dgamma, dbeta [25 D] in slot order (overwritten), with the
 * film vectors the forward was given (NULL = the plan's own LayerNorm parameters). The first backward after a parameter upload
 * transposes the qkv / proj / fc1 / fc2 weights into a plan-owned buffer (144 D^2 floats) on `stream`; inference never
 * allocates it. One stream per plan: a backward issued on another stream is not ordered behind those transposes (nor behind
 * the parameter upload), so the caller orders the streams itself. Tape and workspaces 256-byte aligned; byte counts are 0 for B outside 1..8192. */
size_t orbit_vit_tape_bytes(const orbit_vit_t* v, int B);
/* Opt a patch-16 plan into orbit_vit_train_forward / orbit_vit_backward: the same tape and workspace layouts at 197 tokens per
 * frame ((12 * 9 + 1) * align_up(197 B * D * 4, 256) tape bytes), for 1..2048 frames, 0 outside. orbit_vit_backward_params
 * still returns ORBIT_ERR_ARG before any launch (weight gradients are a second opt-in for the patch-16 models:
 * orbit_vit_enable_weight_backward, next) and its workspace size stays 0. A flag on this plan only: idempotent, allocates nothing, legal before or after orbit_vit_finalize and after
 * inference forwards. A no-op returning ORBIT_OK on a patch-32 plan; ORBIT_ERR_ARG for NULL. */
int orbit_vit_enable_backward(orbit_vit_t* v);
/* Opt a patch-16 plan into orbit_vit_backward_params as well (--learn_extractor): implies orbit_vit_enable_backward, and
 * orbit_vit_backward_params_workspace_bytes is then nonzero for 1..2048 frames, 0 outside. The reverse pass is the patch-32
 * one with the geometry of the plan: every Linear weight gradient at 197 B rows, the patch filter gradient [D][3][16][16] from
 * 196 B gathered 16-float patch rows (K = 768), dpos [197][D]; the promises of orbit_vit_backward_params below hold unchanged
 * (dgamma / dbeta bit for bit those of orbit_vit_backward, FiLM-slot entries of param_grads untouched, deterministic). A flag
 * on this plan only: idempotent, allocates nothing, legal before or after orbit_vit_finalize and after inference forwards. A
 * patch-16 plan that has not called it behaves as described above. A no-op returning ORBIT_OK on a patch-32 plan;
 * ORBIT_ERR_ARG for NULL. */
int orbit_vit_enable_weight_backward(orbit_vit_t* v);
/* Opt a plan (any of the six models) into bf16 token GEMMs for INFERENCE: orbit_vit_forward then runs qkv, proj, fc1 and fc2 of
 * all 12 blocks on v_mfma_f32_32x32x16_bf16 (vit_gemm_bf16_kernel), everything else - patch embedding, class-token row,
 * LayerNorm + FiLM, attention, the fp32 residual stream in HBM - on the fp32 kernels, unchanged. Workspace layout,
 * orbit_vit_workspace_bytes and orbit_vit_macs_per_frame do not change. A documented precision trade, off by default: without
 * this call a plan computes what it always did, bit for bit.
 * Numerics of a bf16 GEMM: x (fp32 token rows) and the weight are each rounded to bf16 once, round to nearest even; their
 * products are exact; every 64-deep K step is summed in the matrix unit from zero and added to the running fp32 sum with one
 * fp32 add per step, in ascending k; bias, GELU and the residual add follow in fp32. Deterministic, and a row's bits depend
 * neither on the number of rows nor on the tile height (so a frame's features do not depend on its batch). Nothing is promised
 * about subnormal inputs.
 * The bf16 weight copies (144 D^2 * 2 bytes, one plan-owned device buffer) are made on `stream` by the first bf16 forward after
 * a parameter upload; every orbit_vit_load* invalidates them, orbit_vit_destroy frees them, and a plan without the flag never
 * allocates them. A flag on this plan only: idempotent, allocates nothing, legal before or after orbit_vit_finalize and after
 * fp32 forwards. Training is fp32 only: on a bf16 plan orbit_vit_train_forward, orbit_vit_backward and orbit_vit_backward_params
 * return ORBIT_ERR_ARG naming orbit_vit_enable_bf16 before any launch or allocation, orbit_vit_enable_backward /
 * orbit_vit_enable_weight_backward are refused the same way, and so is this call on a plan that has either of them set.
 * ORBIT_ERR_ARG for NULL. */
int orbit_vit_enable_bf16(orbit_vit_t* v);
/* 1 after orbit_vit_enable_bf16, else 0 (0 for NULL) */
int orbit_vit_bf16_enabled(const orbit_vit_t* v);
size_t orbit_vit_backward_workspace_bytes(const orbit_vit_t* v, int B);
int orbit_vit_train_forward(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                            float* feats, void* tape, size_t tape_bytes, void* workspace, size_t workspace_bytes,
                            orbit_stream_t stream);
int orbit_vit_backward(orbit_vit_t* v, int B, const float* film_gamma, const float* film_beta, const float* dfeats,
                       const void* tape, size_t tape_bytes, float* dgamma, float* dbeta, void* workspace,
                       size_t workspace_bytes, orbit_stream_t stream);
/* Gradients of every parameter (--learn_extractor), on the tape of orbit_vit_train_forward (unchanged). The flat gradient buffer
 * follows the orbit_extractor_* convention: orbit_vit_grad_floats floats, parameter i (orbit_vit_param_name order) at
 * orbit_vit_param_offset(i) in its torch layout, every tensor 256-byte aligned.
 * orbit_vit_backward_params = orbit_vit_backward (same kernels, same order: dgamma / dbeta are bit for bit what it writes for the
 * same tape and arguments) that also WRITES param_grads for every parameter except the 50 FiLM-slot LayerNorm weights / biases:
 * their gradients are dgamma / dbeta, with or without film vectors (with film vectors the modules' own LayerNorm parameters
 * take no part in the forward), and their slots in param_grads are left untouched. frames: the batch the tape was recorded on
 * (16-byte aligned; the patch-embedding filter gradient reads it). Per block the X operands that are not on the tape are
 * recomputed by the forward's kernels; the Linear filter gradients dW [N][K] = dY^T X split their reduction over the token
 * rows into a number of partial tiles that depends on (rows, N, K) only, added in a fixed order: deterministic, no atomics.
 * param_grads 256-byte aligned; workspace of orbit_vit_backward_params_workspace_bytes (0 for B outside 1..8192; for a
 * patch-16 plan 0 until orbit_vit_enable_weight_backward, then 0 for B outside 1..2048). */
size_t orbit_vit_grad_floats(const orbit_vit_t* v);
size_t orbit_vit_param_offset(const orbit_vit_t* v, int i);
size_t orbit_vit_backward_params_workspace_bytes(const orbit_vit_t* v, int B);
int orbit_vit_backward_params(orbit_vit_t* v, const float* frames, int B, const float* film_gamma, const float* film_beta,
                              const float* dfeats, const void* tape, size_t tape_bytes, float* param_grads, float* dgamma,
                              float* dbeta, void* workspace, size_t workspace_bytes, orbit_stream_t stream);

/* ---- FiLM parameter generator ------------------------------------------------------------------ */
/* n_gen generators (sorted FiLM-name order). Generator i: Linear(z_dim,hid) -> LayerNorm(hid) -> ReLU ->
 * Linear(hid,out_size[i]); kind[i]: 0 = 'weight' (gamma' = g0*(o*r+1)), 1 = 'bias' (beta' = b0 + o*r);
 * dst_offset[i]: offset of its output inside film_gamma (kind 0) / film_beta (kind 1). */
int orbit_filmgen_create(int n_gen, int z_dim, int hidden, const int* out_size, const int* kind,
                         const int* dst_offset, orbit_filmgen_t** out);
void orbit_filmgen_destroy(orbit_filmgen_t* g);
/* tensor: "w1"[hid][z] "b1"[hid] "ln_w"[hid] "ln_b"[hid] "w2"[out][hid] "b2"[out] "reg"[out] "init"[out] */
int orbit_filmgen_load(orbit_filmgen_t* g, int gen, const char* tensor, const float* data, size_t numel);
/* Stream-ordered form for parameters that already live on the device (they follow optimizer steps): ONE gather kernel on
 * `stream` copies all 8 tensors of every generator; device_ptrs[8*gen + t], t in the order listed above. No host sync
 * unless the pointer table changed since the previous call. */
int orbit_filmgen_load_all_async(orbit_filmgen_t* g, const float* const* device_ptrs, int n, orbit_stream_t stream);
/* z [z_dim] -> film_gamma, film_beta (each film_size floats), l2[1] = Σ_i Σ reg_i^2 */
int orbit_filmgen_forward(orbit_filmgen_t* g, const float* z, float* film_gamma, float* film_beta,
                          float* l2, orbit_stream_t stream);

/* ---- single operators (NHWC activations), exposed for parity tests and reuse -------------------- */
/* General convolution as implicit GEMM on fp32 MFMA.
 *   x: NHWC [B][H][W][Cin]  (x_nchw != 0: NCHW [B][Cin][H][W], Cin <= 4 only — the network stems)
 *   w: torch OIHW [Cout][Cin][KH][KW];  y: NHWC [B][Ho][Wo][Cout]  (pool2: [B][Ho/2][Wo/2][Cout])
 *   y = act( conv(x*gate) * scale + shift + residual ), optional fused 2x2/2 max-pool (floor).
 *   scale/shift [Cout] (NULL = 1/0), residual NHWC like y or NULL, gate [B][Cin] or NULL. */
int orbit_op_conv2d(const float* x, int x_nchw, const float* w, float* y,
                    const float* scale, const float* shift, const float* residual, const float* gate,
                    int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad_top, int pad_left, int Ho, int Wo, int act, int pool2,
                    orbit_stream_t stream);
/* The same with flags. ORBIT_CONV_RESIDUAL_POST_ACT: y = act( conv(x) * scale + shift ) + residual - the skip joins AFTER the
 * activation (timm ConvBnAct with a skip, efficientnet_v2_s stage 0). Compiled for plain K x K NHWC convs only: a residual is
 * required, and x_nchw, pool2, a gate or a 1x1 unpadded filter with this flag are argument errors. flags = 0: orbit_op_conv2d.
 * ORBIT_CONV_EPILOGUE_GENERIC: the launch keeps the generic epilogue of conv_igemm_kernel (activation, residual, dual output,
 * statistics and split-K decided at run time) where conv_plan would choose one of the compile-time epilogue forms
 * (csrc/common.h ConvEpi: stride-1 pointwise launches that store one activated output). The two are bit-identical; the flag
 * is a property of this launch, for A/B runs (tools/conv_bench.py ab conv_epilogue) and the bitwise test - there is no
 * runtime option for it, and the network plans always take the compile-time form where one exists. */
#define ORBIT_CONV_RESIDUAL_POST_ACT 1
#define ORBIT_CONV_EPILOGUE_GENERIC 4  /* (2 is not assigned: refused as an unknown flag) */
int orbit_op_conv2d_ex(const float* x, int x_nchw, const float* w, float* y,
                       const float* scale, const float* shift, const float* residual, const float* gate,
                       int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                       int pad_top, int pad_left, int Ho, int Wo, int act, int pool2, int flags,
                       orbit_stream_t stream);
/* Gated 1x1 projection with its squeeze-excite gate (no activation):
 *   gate = sigmoid(W2 silu(W1 (sum over chunks of partial[b][chunk]) / (H*W) + b1) + b2),
 *   y = conv1x1(x * gate) * scale + shift (+ residual).
 * partial [B][chunks][Cin]; w1 [R][Cin]; w2t = W2 transposed [R][Cin]; gate_out [B][Cin] or NULL. Option conv_rgemm != 0 and
 * orbit_pw_stream_supported(): one kernel that computes the gate in its prologue; otherwise se_gate2 + the conv kernel. */
int orbit_op_pw_stream(const float* x, const float* w, const float* scale, const float* shift, const float* residual,
                       const float* partial, int chunks, const float* w1, const float* b1, const float* w2t, const float* b2,
                       int R, float* y, float* gate_out, int B, int H, int W, int Cin, int Cout, orbit_stream_t stream);
int orbit_pw_stream_supported(int Cin, int Cout, int H, int W);
/* depthwise KxK conv, NHWC, w torch [C][1][K][K]; y = act(dw(x)*scale+shift) */
int orbit_op_dwconv2d(const float* x, const float* w, float* y, const float* scale, const float* shift,
                      int B, int H, int W, int C, int K, int stride, int pad_top, int pad_left,
                      int Ho, int Wo, int act, orbit_stream_t stream);
/* Training forms of the two ops (single-operator entries of the parity tests, like the ones above): the convolution without
 * epilogue whose kernel also emits the train-mode BatchNorm statistics of its output (per-channel sums and sums of squares,
 * stats [2][Cout]; *stat_blocks = row blocks written, 0 when this launch shape does not emit them), optionally with the
 * squeeze-excite gate multiplied into x; and the depthwise convolution that applies the PRECEDING layer's BatchNorm +
 * activation to x as it loads it (in_scale / in_shift nullable) and emits the statistics of its own output. Reference: the
 * nn.Conv2d -> nn.BatchNorm2d (train()) pairs of the extractor under model/few_shot_recognisers.py:176-183. */
int orbit_op_conv2d_train(const float* x, int x_nchw, const float* w, float* y, const float* gate, int B, int H, int W,
                          int Cin, int Cout, int KH, int KW, int stride, int pad_top, int pad_left, int Ho, int Wo,
                          float* stats, int* stat_blocks, orbit_stream_t stream);
/* orbit_op_conv2d_plan (host only): what orbit_op_conv2d_ex / orbit_op_conv2d_train and the network plans launch for a conv
 *   under the current options - the one rule every dense conv launch follows. gated, residual != 0: the launch has a
 *   squeeze-excite gate / a residual input; flags as for orbit_op_conv2d_ex. stats_mode: 0 none, 1 BatchNorm statistics from the
 *   epilogue (orbit_op_conv2d_train), 2 the statistics sweep that stores nothing else; dual_output != 0: raw and activated
 *   outputs (the training forward under running statistics). With stats_mode = 0 and no dual output the launch is planned as
 *   orbit_op_conv2d_ex supplies it (fragment-packed filter where the filter has one, split-K workspace where the conv splits),
 *   otherwise as orbit_op_conv2d_train does (neither). row: buffer of 48 chars for the profiler row of the launch
 *   (conv_igemm<..>, conv_bf3<..> or conv_pw_rgemm<..>); *ksplit K-ranges (1: not split) of *kt_per_split K-tiles (0: not
 *   split); *m_tiles row blocks of statistics the launch emits (0: none). A form the launch refuses is refused here with the
 *   same error. */
int orbit_op_conv2d_plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_top, int pad_left, int Ho, int Wo,
                         int x_nchw, int pool2, int gated, int residual, int flags, int stats_mode, int dual_output, char* row,
                         int* ksplit, int* kt_per_split, int* m_tiles);
/* The same with the launch's activation (ORBIT_ACT_*), and in *epilogue the epilogue form of the conv_igemm launch: 0 generic,
 * 1 none, 2 ReLU, 3 SiLU, 4 none with a residual (the compile-time forms; ConvEpi of csrc/common.h). A compile-time form is
 * planned exactly for an inference launch (stats_mode = 0, no dual output, flags without ORBIT_CONV_EPILOGUE_GENERIC) of a
 * stride-1 pointwise conv with Cin % 16 == 0 on a whole 64x64 / 128x32 tile, not split over K, with one of those four
 * (activation, residual) pairs. The profiler row does not depend on the epilogue form. */
int orbit_op_conv2d_plan_ex(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_top, int pad_left, int Ho,
                            int Wo, int x_nchw, int pool2, int gated, int residual, int flags, int stats_mode, int dual_output, int act,
                            char* row, int* ksplit, int* kt_per_split, int* m_tiles, int* epilogue);
int orbit_op_dwconv2d_train(const float* x, const float* w, float* y, const float* in_scale, const float* in_shift,
                            int in_act, int B, int H, int W, int C, int K, int stride, int pad_top, int pad_left, int Ho,
                            int Wo, float* stats, orbit_stream_t stream);
/* The squeeze-excite chain of an MBConv block in inference, link by link (single-operator entries of the parity tests).
 * orbit_op_dwconv2d_se: orbit_op_dwconv2d with the pooling epilogue the plan runs, partial[b][chunk][c] = sum of y over the output
 *   rows of the chunk, [B][chunks][C]; the kernel form follows the options dw_window / dw_lds / dw_pipe.
 * orbit_op_dwconv2d_plan (host only): the form that launch takes under the current options, after the fallback of an LDS patch
 *   that cannot be laid out (*form: 0 streaming, 1 software-pipelined streaming, 2 register window, 3 LDS patch; train_form != 0:
 *   the rule of the statistics form), with *chunks and *rows_per_chunk of its pooling partials.
 * orbit_op_se_gate2: the gate kernel of the plans from pooling partials [B][chunks][C]: pooled = (sum over chunks) / hw,
 *   gate = sigmoid(W2 silu(W1 pooled + b1) + b2); W1 [R][C], W2 torch layout [C][R]; pooled_out [B][C] or NULL. */
int orbit_op_dwconv2d_se(const float* x, const float* w, const float* scale, const float* shift, int act, int B, int H, int W,
                         int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo, float* y, float* partial,
                         orbit_stream_t stream);
int orbit_op_dwconv2d_plan(int B, int C, int K, int stride, int Ho, int Wo, int train_form, int* form, int* chunks,
                           int* rows_per_chunk);
int orbit_op_se_gate2(const float* partial, int chunks, int hw, const float* w1, const float* b1, const float* w2,
                      const float* b2, int B, int C, int R, float* gate, float* pooled_out, orbit_stream_t stream);
/* max-pool NHWC, -inf padding */
int orbit_op_maxpool2d(const float* x, float* y, int B, int H, int W, int C, int K, int stride, int pad,
                       int Ho, int Wo, orbit_stream_t stream);
/* global average pool NHWC [B][HW][C] -> [B][C] */
int orbit_op_avgpool(const float* x, float* y, int B, int HW, int C, orbit_stream_t stream);
/* squeeze-excite gate: g[b][c] = sigmoid(W2 . silu(W1 . pooled[b] + b1) + b2);  W1 [R][C], W2 [C][R] */
int orbit_op_se_gate(const float* pooled, const float* w1, const float* b1, const float* w2,
                     const float* b2, float* gate, int B, int C, int R, orbit_stream_t stream);

/* The transformer extractors' kernels one by one (csrc/vit.hip), token rows row-major fp32.
 * y [M][N] = x [M][K] . w [N][K]^T + bias (NULL = 0); epilogue 0: nothing more, 1: erf-GELU, 2: + residual [M][N] (may alias y;
 * NULL unless epilogue 2). N % 128 == 0, K % 32 == 0, x and w 16-byte aligned. tile_rows: 0 = the forward's rule (128-row
 * tiles when they make at least 512 workgroups, else 64-row), 64 or 128 = that tile height. */
int orbit_op_vit_linear(const float* x, const float* w, const float* bias, const float* residual, float* y, int M, int N,
                        int K, int epilogue, int tile_rows, orbit_stream_t stream);
/* fp32 -> bf16, round to nearest even (ties to even), numel elements: the weight copies of a bf16 plan. w 4-byte aligned, out
 * 2-byte aligned (16-byte aligned buffers take the 8-elements-per-thread path); nothing is written past out[numel - 1]. */
int orbit_op_vit_pack_bf16(const float* w, uint16_t* out, size_t numel, orbit_stream_t stream);
/* orbit_op_vit_linear on the bf16 matrix cores (the numerics stated at orbit_vit_enable_bf16): x [M][K] fp32, rounded to bf16
 * inside the kernel; w_bf16 [N][K] bf16 (orbit_op_vit_pack_bf16); bias, residual (may alias y), y, epilogue and tile_rows as
 * above. N % 128 == 0 and K % 64 == 0, else ORBIT_ERR_ARG with the shape in the message; x and w_bf16 16-byte aligned. */
int orbit_op_vit_linear_bf16(const float* x, const uint16_t* w_bf16, const float* bias, const float* residual, float* y, int M,
                             int N, int K, int epilogue, int tile_rows, orbit_stream_t stream);
/* frames NCHW [B][3][224][224], w OIHW [D][3][32][32], pos_embed [50][D], cls_token [D] -> tokens [B][50][D]: row 0 =
 * cls_token + pos_embed[0], row 1+p = patch p (row-major 7x7) . w + bias + pos_embed[1+p]. D is 384 or 768. */
int orbit_op_vit_patch_embed(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                             const float* cls_token, float* tokens, int B, int D, int tile_rows, orbit_stream_t stream);
/* The same with the patch size: patch 32 is the call above; patch 16 (reference model/feature_extractors.py:49-63 with timm's
 * patch16 models: PatchEmbed = Conv2d(3, D, 16, stride 16), flatten, transpose) takes w OIHW [D][3][16][16], pos_embed [197][D]
 * and writes tokens [B][197][D], row 1+p = patch p (row-major 14x14). B at most 2048 at patch 16. */
int orbit_op_vit_patch_embed_p(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                               const float* cls_token, float* tokens, int B, int D, int patch, int tile_rows,
                               orbit_stream_t stream);
/* The same on square frames of side S (a multiple of `patch`, 32..512; the plans of orbit_vit_create_sized): frames NCHW
 * [B][3][S][S], pos_embed the table AT that grid [(S / patch)^2 + 1][D] (orbit_op_vit_pos_resample), tokens
 * [B][(S / patch)^2 + 1][D]. Always the runtime-geometry form of the GEMM: at S = 224 its result is bit for bit that of
 * orbit_op_vit_patch_embed_p. B * ((S / patch)^2 + 1) at most 8192 * 50. */
int orbit_op_vit_patch_embed_sized(const float* frames, const float* w, const float* bias_or_null, const float* pos_embed,
                                   const float* cls_token, float* tokens, int B, int D, int patch, int S, int tile_rows,
                                   orbit_stream_t stream);
/* The position table of orbit_vit_create_sized: pos [g^2 + 1][D] (g = 7 or 14) -> out [G^2 + 1][D] (1 <= G <= 32, out != pos),
 * row 0 copied, the rest torch's bicubic resample as stated there. D is 384 or 768. */
int orbit_op_vit_pos_resample(const float* pos, float* out, int g, int G, int D, orbit_stream_t stream);
/* LayerNorm over the D (384 or 768) values of each row; row r at x + r * x_stride / y + r * y_stride floats; y may alias x. */
int orbit_op_vit_layernorm(const float* x, size_t x_stride, float* y, size_t y_stride, int rows, int D, const float* gamma,
                           const float* beta, float eps, orbit_stream_t stream);
/* qkv [B][50][3][heads][64] -> out [B][50][heads][64] = softmax(q k^T / 8) v per (frame, head); D = 64 heads, 384 or 768. */
int orbit_op_vit_attention(const float* qkv, float* out, int B, int D, int heads, orbit_stream_t stream);
/* The same with the token count (timm Attention.forward, which reference model/feature_extractors.py:49-63 runs inside every
 * block): qkv [B][tokens][3][heads][64] -> out [B][tokens][heads][64]. tokens = 50 is the call above; tokens = 197 (the patch-16
 * models) runs QK^T and PV on the fp32 matrix cores with the padded keys 197..223 masked out of the softmax; qkv and out then
 * 16-byte aligned and B at most 2048. Any other token count is an argument error. */
int orbit_op_vit_attention_tokens(const float* qkv, float* out, int B, int tokens, int D, int heads, orbit_stream_t stream);
/* The same for ANY token count >= 1, always on the streaming kernel of the sized plans (at 50 and 197 too, where the plans keep
 * the two kernels above): K and V pass through LDS in tiles of 32 keys under a running softmax, keys past tokens - 1 masked; a
 * row's bits depend on the token count alone. qkv and out 16-byte aligned, B * tokens at most 8192 * 50. */
int orbit_op_vit_attention_n(const float* qkv, float* out, int B, int tokens, int D, int heads, orbit_stream_t stream);
/* The backward kernels of orbit_vit_backward one by one.
 * dx [M][K] = dy [M][N] . w [N][K] (w in the torch Linear layout; wt_scratch [K][N] receives its transpose, which the GEMM of
 * orbit_op_vit_linear then reads), optionally times GELU'(u) (u [M][K], the erf form: Phi(u) + u phi(u)) or plus residual [M][K]
 * (may alias dx) - not both. K % 128 == 0, N % 32 == 0; dy, w and wt_scratch 16-byte aligned; tile_rows as above. */
int orbit_op_vit_linear_dgrad(const float* dy, const float* w, float* wt_scratch, const float* u, const float* residual,
                              float* dx, int M, int N, int K, int tile_rows, orbit_stream_t stream);
/* LayerNorm backward over rows of D (384 or 768) values at x + r * x_stride, dy + r * dy_stride: dgamma / dbeta [D] summed over
 * ALL rows (overwritten) and, unless dx is NULL, dx + r * dx_stride = the data gradient (+ dres + r * dx_stride when dres is
 * given, contiguous rows only; it may alias dx). With dx_stride > D (the final norm: only token 0 of a frame's 50 carries a
 * gradient) the rows * dx_stride floats at dx are zeroed before the rows are written. partial: scratch of at least ceil(rows / 64) * 2 * D floats. */
int orbit_op_vit_layernorm_bwd(const float* x, size_t x_stride, const float* dy, size_t dy_stride, const float* gamma, float eps,
                               const float* dres, float* dx, size_t dx_stride, int rows, int D, float* dgamma, float* dbeta,
                               float* partial, size_t partial_floats, orbit_stream_t stream);
/* qkv [B][50][3][heads][64], dout [B][50][heads][64] -> dqkv in qkv's layout (gradients of q, k and v). */
int orbit_op_vit_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int D, int heads,
                               orbit_stream_t stream);
/* The same with the token count: tokens = 50 is the call above; tokens = 197 (the patch-16 models) recomputes S and P and runs
 * every product on the fp32 matrix cores, one workgroup per (frame, head), no atomics: a frame's dqkv does not depend on B and
 * two runs are bitwise equal. qkv, dout and dqkv then 16-byte aligned and B at most 2048. Any other token count is an
 * argument error; every refusal comes before any launch. */
int orbit_op_vit_attention_bwd_tokens(const float* qkv, const float* dout, float* dqkv, int B, int tokens, int D, int heads,
                                      orbit_stream_t stream);
/* The weight-gradient kernels of orbit_vit_backward_params one by one.
 * dw [N][K] = dy [M][N]^T . x [M][K] (gelu_on_x = 1: . GELU_erf(x), the fc2 layer, whose tape holds the pre-activation) and,
 * unless dbias is NULL, dbias [N] = the column sums of dy; both overwritten. N % 128 == 0, K % 32 == 0; every pointer 16-byte
 * aligned. The reduction over M is split into partial tiles in `workspace` (at least
 * orbit_op_vit_linear_wgrad_workspace_floats(M, N, K) floats - a function of the shape alone, 0 for a shape the entry point
 * refuses; NULL allowed when it is 0) that a second launch adds in a fixed order. */
size_t orbit_op_vit_linear_wgrad_workspace_floats(int M, int N, int K);
int orbit_op_vit_linear_wgrad(const float* dy, const float* x, float* dw, float* dbias_or_null, int M, int N, int K, int gelu_on_x,
                              float* workspace, size_t workspace_floats, orbit_stream_t stream);
/* Backward of orbit_op_vit_patch_embed: frames NCHW [B][3][224][224], dtokens [B][50][D] -> dw OIHW [D][3][32][32], dbias [D]
 * (NULL: the CLIP form has none) = the sum of token rows 1..49, dpos [50][D] = the sum over frames, dcls [D] = its row 0.
 * workspace: orbit_op_vit_linear_wgrad_workspace_floats(49 B, D, 3072) floats. */
int orbit_op_vit_patch_embed_bwd(const float* frames, const float* dtokens, float* dw, float* dbias_or_null, float* dpos,
                                 float* dcls, int B, int D, float* workspace, size_t workspace_floats, orbit_stream_t stream);
/* The same with the patch size as an argument (backward of orbit_op_vit_patch_embed_p). patch = 32: the call above. patch = 16:
 * dtokens [B][197][D] -> dw OIHW [D][3][16][16], dbias [D] (or NULL) = the sum of token rows 1..196, dpos [197][D], dcls [D];
 * workspace: orbit_op_vit_linear_wgrad_workspace_floats(196 B, D, 768) floats; B at most 2048. Any other patch size, width or
 * batch, a null pointer, a misaligned pointer or a short workspace is an argument error before any launch. */
int orbit_op_vit_patch_embed_bwd_p(const float* frames, const float* dtokens, float* dw, float* dbias_or_null, float* dpos,
                                   float* dcls, int B, int D, int patch, float* workspace, size_t workspace_floats,
                                   orbit_stream_t stream);

/* fused MBConv front half (EfficientNet InvertedResidual, Cin <= 40): y = silu(bn2(dw_KxK(silu(bn1(x . w1^T))))) with the
 * expanded tensor kept in LDS. x NHWC [B][H][W][Cin]; w1 torch [mid][Cin][1][1]; wdw torch [mid][1][K][K];
 * scale/shift = folded BatchNorms [mid]; y NHWC [B][Ho][Wo][mid]; pool_partial [B][tiles][mid] or NULL: partial sums
 * of y for the SE average pool, tiles = orbit_op_mbconv_front_partials(...) (the kernel form - tiled, whole-map or
 * row-streaming or not, option mbconv_rows - decides how many partial sums a frame has). */
int orbit_op_mbconv_front_partials(int H, int W, int Cin, int mid, int K, int stride);
int orbit_op_mbconv_front(const float* x, const float* w1, const float* scale1, const float* shift1,
                          const float* wdw, const float* scale2, const float* shift2, float* y, float* pool_partial,
                          int B, int H, int W, int Cin, int mid, int K, int stride, int pad_top, int pad_left,
                          int Ho, int Wo, orbit_stream_t stream);
/* The tiling of the row-streaming front on an H x W input map (host only; an argument error for every shape
 * orbit_op_mbconv_front refuses, for which orbit_op_mbconv_front_partials returns 0). The Ho x Wo output map is cut into
 * `bands` bands of `band_rows` output rows and `strips` strips of `strip_w` output columns; tiles = strips * bands, and tile t of a
 * frame covers band t / strips and strip t % strips, clipped to the map: rows [band * band_rows, min(Ho, (band + 1) * band_rows))
 * and columns [strip * strip_w, min(Wo, (strip + 1) * strip_w)). pool_partial[b][t] / stats_partial[b * tiles + t] hold the sums
 * over that rectangle. exact = 1: the launch takes a branch-free instantiation (strips tile Wo, every band is a whole number of
 * steps, mid % 32 is 0 or 16); 0: the predicated one. */
int orbit_op_mbconv_front_plan(int H, int W, int Cin, int mid, int K, int stride, int* strips, int* bands, int* strip_w,
                               int* band_rows, int* exact);
/* The train-mode BatchNorm form of orbit_op_mbconv_front: scale1 / shift1 are the first BatchNorm's batch-statistics fold, the second
 * BatchNorm is NOT applied: y_raw NHWC [B][Ho][Wo][mid] receives the depthwise outputs, and stats_partial [B * tiles][2][mid]
 * (required) the per-tile column sums ([.][0][c]) and sums of squares ([.][1][c]) of those outputs - the partial layout
 * orbit_op_bn_stats_from_partials reads with nblk = B * tiles, M = B * Ho * Wo. */
int orbit_op_mbconv_front_raw(const float* x, const float* w1, const float* scale1, const float* shift1, const float* wdw,
                              float* y_raw, float* stats_partial, int B, int H, int W, int Cin, int mid, int K, int stride,
                              int pad_top, int pad_left, int Ho, int Wo, orbit_stream_t stream);
/* The stem form of the same kernel (timm tf_efficientnet_b0: conv_stem -> bn1 -> SiLU -> blocks.0.0.conv_dw -> bn1 ->
 * SiLU, reached from model/feature_extractors.py:39-43): frames NCHW [B][3][FH][FW], w_stem torch [mid][3][3][3]
 * (3x3 stride 2, padding spad_top / spad_left before, the rest after), depthwise 3x3 stride 1 on the stem's H x W output
 * grid; y NHWC [B][Ho][Wo][mid]; pool_partial [B][ceil(Ho/8)*ceil(Wo/8)][mid] or NULL. The stem output never reaches HBM. */
int orbit_op_stem_dw_front_partials(int H, int W, int mid);  /* pool_partial rows per frame under the current options */
int orbit_op_stem_dw_front(const float* frames, const float* w_stem, const float* scale1, const float* shift1,
                           const float* wdw, const float* scale2, const float* shift2, float* y, float* pool_partial,
                           int B, int FH, int FW, int spad_top, int spad_left, int H, int W, int mid, int pad_top,
                           int pad_left, int Ho, int Wo, orbit_stream_t stream);
/* The tiling of orbit_op_stem_dw_front on the stem's H x W output grid (host only; an argument error for a shape that entry
 * refuses): strips, bands, tile rectangles and `exact` as orbit_op_mbconv_front_plan reports them, with Ho = H, Wo = W. */
int orbit_op_stem_dw_front_plan(int H, int W, int mid, int* strips, int* bands, int* strip_w, int* band_rows, int* exact);

/* ---- Versa / Mahalanobis heads -----------------------------------------------------------
 * y[r][o] = act(x[r] . W[o] + b[o]) (+ residual[r][o]) for a few rows r < R <= 16 (one row per class): the layers of
 * the Versa hyper-networks, model/mlps.py:33-50 DenseResidualBlock (linear -> ELU -> linear -> ELU -> linear (+ x)),
 * applied to the class means by VersaClassifier.configure, model/classifier_heads.py:158-180. W is torch [out][in]. */
int orbit_dense_rows(const float* x, int R, int in, const float* W, const float* b, int out, int act,
                     const float* residual, float* y, orbit_stream_t stream);
/* batched inverse of `batch` symmetric positive definite n x n matrices (in-place blocked Gauss-Jordan, no pivoting);
 * replaces torch.inverse in MahalanobisClassifier.configure (classifier_heads.py:288,311). A == Ainv allowed. */
int orbit_spd_inverse(const float* A, float* Ainv, int n, int batch, orbit_stream_t stream);
size_t orbit_mahalanobis_workspace_bytes(int N, int M, int D, int C);
/* MahalanobisClassifier.configure (classifier_heads.py:284-327): features [N][D], labels [N], class_ids [C] ascending
 * -> means [C][D], task_mean [D], precisions [C][D][D] = inverse(l cov_c + (1-l) cov_task + I), l = n_c/(n_c+1),
 * task_precision [D][D] = inverse(cov_task + I); covariances are torch.cov(correction=1), a single-example class takes
 * the reference's scalar branch (:361-364). */
int orbit_mahalanobis_configure(const float* features, const int64_t* labels, const int64_t* class_ids, int N, int D,
                                int C, float* means, float* task_mean, float* precisions, float* task_precision,
                                void* workspace, size_t workspace_bytes, orbit_stream_t stream);
/* MahalanobisClassifier.predict (:329-347): logits[m][c] = -scale * (mu_c - q_m)^T P_c (mu_c - q_m). D % 4 == 0. */
int orbit_mahalanobis_predict(const float* features, const float* means, const float* precisions, int M, int D, int C,
                              float logit_scale, float* logits, void* workspace, size_t workspace_bytes,
                              orbit_stream_t stream);

/* d(features) of orbit_mahalanobis_predict (means / precisions are constants, as in the reference :324-327):
 * dfeatures[m] = scale * sum_c dlogits[m][c] (P_c + P_c^T)(mu_c - q_m) */
int orbit_mahalanobis_predict_backward(const float* dlogits, const float* features, const float* means,
                                       const float* precisions, int M, int D, int C, float logit_scale, float* dfeatures,
                                       void* workspace, size_t workspace_bytes, orbit_stream_t stream);

/* ---- training (LITE meta-training step) -----------------------------------------------------
 * What `loss.backward()` runs in the reference (single-step-learner.py:234) for the graph recorded by
 * model/few_shot_recognisers.py:99-122 (_get_features, grad enabled), :345-356 (_get_task_embedding on the LITE
 * subset) and model/classifier_heads.py:202-230 (head). BatchNorm mode follows few_shot_recognisers.py:176-183.
 * Available for the resnet18, efficientnet_b0 and set_encoder plans (orbit_extractor_supports_training is 0 for a plan built
 * with the fused MBConv front op, and for efficientnet_v2_s unless its plan was created with ORBIT_PLAN_RES_POST_BACKWARD or
 * ORBIT_PLAN_RES_POST_TRAINING). */
int orbit_extractor_supports_training(const orbit_extractor_t* fe);
size_t orbit_extractor_tape_bytes(const orbit_extractor_t* fe, int B);
size_t orbit_extractor_backward_workspace_bytes(const orbit_extractor_t* fe, int B);
size_t orbit_extractor_grad_floats(const orbit_extractor_t* fe);          /* length of the flat gradient buffer */
size_t orbit_extractor_param_offset(const orbit_extractor_t* fe, int i);  /* offset of parameter i inside it */
size_t orbit_extractor_bn_stat_floats(const orbit_extractor_t* fe);
/* dst[0][.] running means, dst[1][.] running variances of every BatchNorm (in parameter order, each padded to a
 * multiple of 4 channels; row length = orbit_extractor_bn_stat_floats): how the caller's state_dict buffers follow the
 * running-stat updates of train-mode forwards */
int orbit_extractor_export_bn_stats(orbit_extractor_t* fe, float* dst, orbit_stream_t stream);
/* Forward that records the tape (raw convolution outputs, activations, pooling argmax; caller-owned, 256-B aligned).
 * bn_train != 0: batch statistics + running-stat update with `momentum` (nn.BatchNorm2d semantics);
 * bn_train == 0: running statistics. film_gamma/film_beta as in orbit_extractor_forward. */
int orbit_extractor_train_forward(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                                  const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                                  size_t tape_bytes, orbit_stream_t stream);
/* The same with flags. ORBIT_TRAIN_NO_BACKWARD: no backward will be run on this tape - the forwards the reference issues
 * under torch.no_grad() while the extractor is in train() (LITE's cache passes, few_shot_recognisers.py:134-146,388-437):
 * batch statistics and running-stat updates as above, but activations no later kernel of THIS forward needs are not
 * materialised (the depthwise convs apply the preceding BatchNorm + activation while loading the raw conv output). Features
 * are bit-identical to the flag-less call; orbit_extractor_backward on such a tape is undefined. */
#define ORBIT_TRAIN_NO_BACKWARD 1
/* ORBIT_TRAIN_DEFER_RUNNING_STATS (bn_train != 0): the running-statistics update is NOT applied; the batch mean / unbiased
 * variance of every BatchNorm stay on the tape and orbit_extractor_apply_deferred_bn_stats applies
 * running = (1 - momentum) * running + momentum * stat afterwards (same arithmetic, so the result equals the in-place update
 * made at that point of the sequence). Such a forward touches no mutable state of the plan: it may run on ANOTHER stream
 * while a forward of the same plan that does update the statistics is in flight - LITE re-encodes its H-clip subset (16
 * frames: launch-bound kernels) beside the cache pass over the whole context set (few_shot_recognisers.py:388-437), and the
 * reference's update order (cache pass, then subset) is kept by applying the subset's update after both. */
#define ORBIT_TRAIN_DEFER_RUNNING_STATS 2
int orbit_extractor_train_forward_ex(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                                     const float* film_beta, int bn_train, float momentum, float* feats, void* tape,
                                     size_t tape_bytes, int flags, orbit_stream_t stream);
int orbit_extractor_apply_deferred_bn_stats(orbit_extractor_t* fe, const void* tape, size_t tape_bytes, int B, float momentum,
                                            orbit_stream_t stream);
/* Reverse pass for the tape of one train_forward (same frames / B / film / bn_train).
 *   dfeats [B][D]: gradient w.r.t. the features.
 *   param_grads: NULL (frozen extractor) or orbit_extractor_grad_floats() floats; the gradient of parameter i is
 *     WRITTEN at orbit_extractor_param_offset(i) in the parameter's torch layout (OIHW filters). Slots of buffers
 *     (running statistics) and of BatchNorm weight/bias replaced by FiLM vectors are left untouched.
 *     filter_grads == 0: only the BatchNorm weight / bias gradients are computed (FiLM fine-tuning of a frozen
 *     extractor, few_shot_recognisers.py:196-199); != 0: every parameter.
 *   dfilm_gamma / dfilm_beta: NULL or film_size floats each, written.
 * Deterministic: fixed reduction order, no atomics. */
int orbit_extractor_backward(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                             const float* film_beta, int bn_train, const float* dfeats, const void* tape,
                             size_t tape_bytes, float* param_grads, int filter_grads, float* dfilm_gamma,
                             float* dfilm_beta, void* workspace, size_t workspace_bytes, orbit_stream_t stream);
/* filter_grads = ORBIT_FILTER_GRADS_SE_PER_BLOCK: as filter_grads = 1, with the parameter gradients of every squeeze-excite
 * block summed by a launch of its own instead of the batched launches of the reverse pass (A/B measurements and parity runs;
 * the two forms add the frames in different orders). */
#define ORBIT_FILTER_GRADS_SE_PER_BLOCK 2
/* Training entry points replay captured HIP graphs when a call repeats an earlier call's pointers and scalars exactly
 * (option train_graph = 1, off by default: it frees the host but the step is GPU-bound; the plan's own buffers never move). Diagnostics: calls that replayed / ran eagerly. */
int orbit_extractor_train_graph_stats(const orbit_extractor_t* fe, long* replays, long* eager);
/* Backward of orbit_filmgen_forward: given d(film_gamma), d(film_beta) (film_size floats each) and d(l2) ([1], NULL = 0)
 * writes the gradients of every generator parameter into `grads` (orbit_filmgen_grad_floats floats; tensor t of
 * generator i at orbit_filmgen_param_offset(g, i, t), same tensor names as orbit_filmgen_load except "init") and
 * d(z) [z_dim] (NULL to skip). Reference: autograd through model/feature_adapters.py:66-78, model/mlps.py:52-63. */
size_t orbit_filmgen_grad_floats(const orbit_filmgen_t* g);
size_t orbit_filmgen_param_offset(const orbit_filmgen_t* g, int gen, const char* tensor);
int orbit_filmgen_backward(orbit_filmgen_t* g, const float* z, const float* dfilm_gamma, const float* dfilm_beta,
                           const float* dl2, float* grads, float* dz, orbit_stream_t stream);
/* d(features) of orbit_proto_predict for ONE task: features [M*T][D] (frame features, pooled over T inside),
 * weight [C][D] (treated as a constant: the reference wraps it in nn.Parameter, classifier_heads.py:261-263),
 * dlogits [M][C] -> dfeatures [M*T][D]. C <= 64. */
int orbit_proto_predict_backward(const float* dlogits, const float* features, const float* weight, int M, int T, int D,
                                 int C, float logit_scale, int cosine, float* dfeatures, orbit_stream_t stream);

/* parameter gradients of a linear head logits = scale * (features . W^T + b) (LinearClassifier.predict,
 * classifier_heads.py:62-76, trained by the multi-step finetuner few_shot_recognisers.py:209-247): dweight [C][D],
 * dbias [C] (nullable). The feature gradient is orbit_proto_predict_backward (euclidean form). */
int orbit_linear_head_backward(const float* dlogits, const float* features, int M, int D, int C, float logit_scale,
                               float* dweight, float* dbias, orbit_stream_t stream);

/* Cross-entropy of logits [N][C] against int64 labels [N]: reference utils/optim.py:8-9 (F.cross_entropy, the `loss` of
 * single-step-learner.py:77,225-232 and of the FineTuner, few_shot_recognisers.py:231-236).
 * row_loss [N] = logsumexp(logits[i]) - logits[i][labels[i]] (NaN for a label outside [0, C)); softmax [N][C] is kept for
 * the backward (NULL to skip); loss [1] = mean / sum of the rows in one fixed order (ORBIT_REDUCE_MEAN / _SUM; unused for
 * ORBIT_REDUCE_NONE). N = 0 is allowed (mean = NaN, sum = 0, like torch). */
int orbit_cross_entropy_forward(const float* logits, const int64_t* labels, int N, int C, int reduction, float* row_loss,
                                float* softmax, float* loss, orbit_stream_t stream);
/* dlogits [N][C] = g_i * (softmax - onehot(labels)); g_i = grad[0] / N (mean), grad[0] (sum), grad[i] (none). `grad` is a
 * DEVICE pointer (the upstream gradient): nothing is read back to the host. */
int orbit_cross_entropy_backward(const float* softmax, const int64_t* labels, const float* grad, int N, int C,
                                 int reduction, float* dlogits, orbit_stream_t stream);

/* ---- multi-tensor optimizer step (csrc/optim.hip) ------------------------------------------------------------------
 * One launch updates every fp32 tensor of a model: reference utils/optim.py:11-33 (torch.optim.Adam / torch.optim.SGD over the
 * two parameter groups; stepped at single-step-learner.py:163 and few_shot_recognisers.py:216). The arithmetic is torch.optim's
 * (L2 weight decay added to the gradient, Adam's bias corrections computed on the host in double, no amsgrad; SGD with
 * dampening 0 and no Nesterov), with a correctly rounded square root and true divisions.
 *
 * A table has one row per tensor that has a gradient. `rows` is the table in DEVICE memory, `host_rows` the caller's HOST copy
 * of the same n_tensors rows: every check below reads the host copy, before any launch; the kernel reads the device copy. The
 * caller owns both and keeps the device table alive and unchanged until the step has run - two steps with two tables may be
 * issued back to back on one stream. Pointers are 4-byte aligned device pointers to numel contiguous floats; a row whose
 * pointers are all 16-byte aligned takes the vector path. */
#define ORBIT_OPTIM_MAX_GROUPS 8
#define ORBIT_OPTIM_FIRST_STEP 1 /* orbit_optim_row_t.flags, SGD with momentum: the tensor's first step, buf = g */
typedef struct orbit_optim_row {
    void* p;           /* parameter, updated in place */
    const void* grad;  /* its gradient, read only */
    void* state1;      /* Adam exp_avg / SGD momentum_buffer (may be NULL for SGD without momentum) */
    void* state2;      /* Adam exp_avg_sq (unused by SGD, may be NULL there) */
    uint64_t numel;
    int32_t group;     /* index into group_lr / group_weight_decay */
    int32_t flags;     /* ORBIT_OPTIM_* */
} orbit_optim_row_t;
/* Adam step number `step` (>= 1, the value torch keeps in state["step"] AFTER the step) of every row:
 *   g += wd p;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * Refused: a NULL table, host table, group array or row pointer; n_tensors <= 0; n_groups outside [1, 8]; a row's group outside
 * [0, n_groups); a pointer that is not 4-byte aligned; numel == 0; step < 1; a beta outside [0, 1); a negative eps, lr or
 * weight decay. Profiled as "optim_adam" (28 bytes per element). */
int orbit_optim_adam_step(const orbit_optim_row_t* rows, const orbit_optim_row_t* host_rows, int n_tensors,
                          const double* group_lr, const double* group_weight_decay, int n_groups, int64_t step, double beta1,
                          double beta2, double eps, orbit_stream_t stream);
/* SGD: g += wd p; momentum != 0: buf = g where the row carries ORBIT_OPTIM_FIRST_STEP, else buf = momentum buf + g, and
 * p -= lr buf; momentum == 0: p -= lr g, state1 is not touched. The same refusals (state1 is required only with momentum;
 * momentum must not be negative). Profiled as "optim_sgd" (12 bytes per element, 20 with momentum). */
int orbit_optim_sgd_step(const orbit_optim_row_t* rows, const orbit_optim_row_t* host_rows, int n_tensors,
                         const double* group_lr, const double* group_weight_decay, int n_groups, double momentum,
                         orbit_stream_t stream);

/* single training operators (NHWC, [M][C] = [B*H*W][C]), exposed for parity tests against torch autograd */
/* out = act(BN_train(y) + residual): batch mean / biased variance, saves mean and 1/sqrt(var+eps), updates the running
 * statistics in place when given (unbiased variance, momentum). gamma/beta NULL = 1/0. act: NONE or RELU. */
int orbit_op_bn_train_forward(const float* y, int M, int C, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, const float* residual, int act,
                              float* out, float* save_mean, float* save_invstd, orbit_stream_t stream);
/* Batch statistics (mean, 1/sqrt(biased var + eps)) of y = W x for a POINTWISE conv (W [C][Cin], torch's 1x1 filter layout;
 * x [P][Cin] NHWC pixels; Cin = 16 or 24) from the Gram matrix of x - without forming y (csrc/train_ops.hip): the first
 * sweep of the two-sweep fused MBConv front on the no-grad cache pass of the LITE step (few_shot_recognisers.py:404-408). */
int orbit_op_bn_stats_from_gram(const float* x, int P, int Cin, const float* w, int C, float eps, float* save_mean,
                                float* save_invstd, orbit_stream_t stream);
/* backward of out = act(BN(y) + residual): dy, dres (= dout * act', NULL to skip), dgamma, dbeta.
 * train != 0: batch-statistics form; train == 0: mean/invstd are running statistics (constants). */
int orbit_op_bn_backward(const float* dout, const float* out, const float* y, int M, int C, const float* gamma,
                         const float* mean, const float* invstd, int train, int act, float* dy, float* dres,
                         float* dgamma, float* dbeta, orbit_stream_t stream);
/* The same with the folded scale / shift of the forward (scale = gamma * invstd, shift = beta - mean * scale; needed for SiLU,
 * which this entry admits: its derivative is taken at scale * y + shift) and flags. ORBIT_BN_RESIDUAL_POST_ACT: backward of
 * out = act(BN(y)) + residual, the skip joining AFTER the activation (timm ConvBnAct): with g = dout * act'(scale * y + shift),
 * dres receives dout (not g), dgamma / dbeta are the sums of g * xhat / g and dy is formed from g as above.
 * dres_accumulate != 0: dres += instead of dres =. */
#define ORBIT_BN_RESIDUAL_POST_ACT 1
int orbit_op_bn_backward_ex(const float* dout, const float* out, const float* y, int M, int C, const float* gamma,
                            const float* mean, const float* invstd, const float* scale, const float* shift, int train, int act,
                            int flags, float* dy, float* dres, int dres_accumulate, float* dgamma, float* dbeta,
                            orbit_stream_t stream);
/* The activation pass of the training forward on its own: out = act(scale * y + shift + residual), or with
 * flags = ORBIT_BN_RESIDUAL_POST_ACT out = act(scale * y + shift) + residual. y, out, residual (nullable) [M][C]; scale, shift [C]. */
int orbit_op_scale_shift_act(const float* y, const float* scale, const float* shift, const float* residual, int act, int M, int C,
                             int flags, float* out, orbit_stream_t stream);
/* The train-mode BatchNorm chain link by link (single-operator entries of the parity tests, csrc/train_ops.hip).
 * orbit_op_bn_reduce_plan (host only): the layout of the per-channel reductions over an [M][C] tensor - *G channel-quad lanes
 *   and *R = 256 / G row lanes of a block, *ygroups column groups of G quads, *nblk row blocks of *rows_per_block rows.
 * orbit_op_se_pool_chunks (host only): *chunks per frame of the pooled apply pass below, *rows_per_chunk pixels each.
 * orbit_op_bn_stats_from_partials: the finalize behind a producer's partial[nblk][2][C] (sums of y and of y^2 over row blocks that
 *   tile the M rows): mean, invstd [C], and when given (NULL to skip) the folded scale / shift and the running statistics
 *   (conv_bias [C], nullable: the bias the producing convolution left out of y). Lists of more than 2048 blocks pass the
 *   compaction stage. The caller's partials are not modified.
 * orbit_op_bn_backward_reduced: the BatchNorm backward behind a producer's partial[nblk][2][C] of g and g * xhat (g = the
 *   gradient behind the activation, xhat = (y - mean) * invstd): dgamma, dbeta (NULL to skip), dy [M][C] (NULL to skip).
 * orbit_op_scale_shift_act_pool: out = act(scale * y + shift) on [B][HW][C] with pool[b][chunk][c] = the sum of out over the
 *   chunk's pixels, [B][chunks][C] - what orbit_op_se_gate2 reads. */
int orbit_op_bn_reduce_plan(int M, int C, int* G, int* R, int* ygroups, int* nblk, int* rows_per_block);
int orbit_op_se_pool_chunks(int B, int HW, int C, int* chunks, int* rows_per_chunk);
int orbit_op_bn_stats_from_partials(const float* partial, int nblk, int M, int C, const float* gamma, const float* beta,
                                    const float* conv_bias, float eps, float momentum, float* running_mean, float* running_var,
                                    float* mean, float* invstd, float* scale, float* shift, orbit_stream_t stream);
int orbit_op_bn_backward_reduced(const float* g, const float* y, const float* mean, const float* invstd, const float* gamma, int train,
                                 int M, int C, const float* partial, int nblk, float* dy, float* dgamma, float* dbeta,
                                 orbit_stream_t stream);
int orbit_op_scale_shift_act_pool(const float* y, const float* scale, const float* shift, int act, int B, int HW, int C, float* out,
                                  float* pool, orbit_stream_t stream);
/* dx of a convolution: dy NHWC [B][Ho][Wo][Cout], w OIHW, dx NHWC [B][H][W][Cin] (= accumulate + grad if given) */
int orbit_op_conv2d_dgrad(const float* dy, const float* w, const float* accumulate, float* dx, int B, int H, int W,
                          int Cin, int Cout, int KH, int KW, int stride, int pad_top, int pad_left, int Ho, int Wo,
                          orbit_stream_t stream);
/* dw (OIHW) of a convolution; x NHWC (or NCHW when x_nchw, Cin <= 4) */
int orbit_op_conv2d_wgrad(const float* x, int x_nchw, const float* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                          int KH, int KW, int stride, int pad_top, int pad_left, int Ho, int Wo, orbit_stream_t stream);
/* The filter gradient of a squeeze-excite-gated pointwise projection, dW[co][ci] = sum_m dy[m][co] * x[m][ci] * gate[b(m)][ci]
 * (timm InvertedResidual.conv_pwl behind the SE module; x NHWC [B][H][W][Cin], gate [B][Cin], dy [B][H][W][Cout]): the product
 * x * gate is never materialised. Single-operator entry for the parity tests. */
int orbit_op_conv2d_wgrad_gated(const float* x, const float* gate, const float* dy, float* dw, int B, int H, int W, int Cin,
                                int Cout, orbit_stream_t stream);
/* orbit_op_conv2d_wgrad_plan (host only): the kernel form the two entries above and the training plans run for a layer, and its
 *   split geometry. *form: 0 the 64x64-tile kernel on NHWC x, 1 the same on NCHW x, 2 the thin register form (pointwise, unpadded,
 *   >= 2^18 rows, the thinner side <= 32 channels). thin[7] = TF, TT (16-channel tiles of the fat / thin side a wave holds: the
 *   kernel instantiation), fat_is_co (1: the fat side is dy), groups and tiles_per_group of the fat side, blocks (row splits) and
 *   rows_per_wave; zeros for the tiled forms. tiled[4] = co_tiles, n_tiles, splits, steps_per_split (32-row steps); zeros for thin.
 *   gated != 0: the layer has a squeeze-excite gate (refused with x_nchw, as the launch refuses it).
 * orbit_op_conv2d_wgrad_batched: the filter gradients of n <= 48 layers as a network's reverse pass computes them - every layer's
 *   main kernel with its split reduction deferred, then the reductions of all layers in ONE launch. x, dy, dw: arrays of n device
 *   pointers; gate: array of n device pointers (entries nullable) or NULL; x_nchw: n flags; geom: n x 12 ints
 *   B, H, W, Cin, Cout, KH, KW, stride, pad_top, pad_left, Ho, Wo. Each dw has the bits of the same layer through
 *   orbit_op_conv2d_wgrad / _gated. Single-operator entries for the parity tests. */
int orbit_op_conv2d_wgrad_plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_top, int pad_left, int Ho,
                               int Wo, int x_nchw, int gated, int* form, int* thin, int* tiled);
int orbit_op_conv2d_wgrad_batched(int n, const float* const* x, const int* x_nchw, const float* const* dy, float* const* dw,
                                  const float* const* gate, const int* geom, orbit_stream_t stream);
/* max-pool that records the argmax (position inside the window, first maximum in scan order) and its backward */
int orbit_op_maxpool2d_train(const float* x, float* y, uint8_t* idx, int B, int H, int W, int C, int K, int stride,
                             int pad, int Ho, int Wo, orbit_stream_t stream);
int orbit_op_maxpool2d_backward(const float* dy, const uint8_t* idx, float* dx, int B, int H, int W, int C, int K,
                                int stride, int pad, int Ho, int Wo, orbit_stream_t stream);
int orbit_op_avgpool_backward(const float* dy, float* dx, int B, int HW, int C, orbit_stream_t stream);
/* depthwise KxK convolution backward (K in {3,5}): dx NHWC [B][H][W][C] and/or dw torch [C][1][K][K] (either may be NULL) */
int orbit_op_dwconv2d_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, int B, int H, int W,
                               int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo,
                               orbit_stream_t stream);
/* The depthwise data gradient continued through the producer's activation, with the first pass of that producer's BatchNorm
 * backward in its epilogue: g = dx * act'(y_raw * scale[c] + shift[c]) [B][H][W][C] and sums [2][C] = sum over (b,h,w) of g and
 * of g * (y_raw - mean[c]) * invstd[c] (reference: autograd through timm InvertedResidual's conv_dw <- act1 <- bn1,
 * few_shot_recognisers.py:99-122). dw (optional, [C][1][K][K]): the layer's filter gradient from the same pass - its input is
 * act(y_raw * scale + shift), rebuilt at the output pixels anyway (stride-2 layers). Fails with ORBIT_ERR_ARG where no kernel
 * form carries the epilogue / the filter gradient (the caller then runs the separate passes): decided on the host by the rules of
 * orbit_op_dwconv2d_backward_plan, before anything is launched or written. Single-operator entry for the parity tests. */
int orbit_op_dwconv2d_dgrad_bn(const float* dy, const float* w, const float* y_raw, const float* mean, const float* invstd,
                               const float* scale, const float* shift, int act, float* g, float* sums, float* dw, int B, int H,
                               int W, int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo, orbit_stream_t stream);
/* The depthwise filter gradient with the layer's input rebuilt on load: x_raw is the RAW output of the preceding convolution and
 * the layer's input is act(x_raw * in_scale[c] + in_shift[c]) (that convolution's batch-statistics BatchNorm + SiLU / ReLU;
 * reference: autograd through timm InvertedResidual's bn1 + act1 + conv_dw, few_shot_recognisers.py:99-122). The taped forward
 * of the LITE step never writes the activated tensor. dw [C][1][K][K]. Single-operator entry for the parity tests. */
int orbit_op_dwconv2d_wgrad_xf(const float* x_raw, const float* in_scale, const float* in_shift, int in_act, const float* dy,
                               float* dw, int B, int H, int W, int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo,
                               orbit_stream_t stream);
/* backward of the squeeze-excite product xg = x * gate(mean_hw(x)) (timm SqueezeExcite: conv_reduce -> SiLU ->
 * conv_expand -> sigmoid): given dxg writes dx and (all or none) dW1 [R][C], db1 [R], dW2 [C][R], db2 [C].
 * x NHWC [B][HW][C]; pooled [B][C] = mean over HW of x. */
int orbit_op_se_gate_backward(const float* dxg, const float* x, const float* pooled, const float* w1, const float* b1,
                              const float* w2, const float* b2, float* dx, float* dw1, float* db1, float* dw2,
                              float* db2, int B, int HW, int C, int R, orbit_stream_t stream);
/* The same with flags. ORBIT_SE_PARAMS_BATCHED: the four parameter gradients come from the kernel that sums them for all the
 * blocks of a network's reverse pass (here as a launch of one job; R <= 64) instead of the per-block kernel. The two add the
 * frames in different orders. */
#define ORBIT_SE_PARAMS_BATCHED 1
int orbit_op_se_gate_backward_ex(const float* dxg, const float* x, const float* pooled, const float* w1, const float* b1,
                                 const float* w2, const float* b2, float* dx, float* dw1, float* db1, float* dw2,
                                 float* db2, int B, int HW, int C, int R, int flags, orbit_stream_t stream);
/* Host only, launches nothing: what the depthwise backward launchers do for a layer under the current options - the rules the
 * launchers themselves ask. mode: which call is meant (the entries above pass the flipped-tap scratch, so stride-1 data
 * gradients run a forward kernel form over dy). A layer a mode's entry refuses reads epilogue = 0 (the _BN modes) or
 * wgrad = 0 (_BN_WGRAD, _WGRAD_XF). Single-operator entry for the parity tests. */
#define ORBIT_DWBWD_DGRAD 0          /* orbit_op_dwconv2d_backward, dx */
#define ORBIT_DWBWD_DGRAD_BN 1       /* orbit_op_dwconv2d_dgrad_bn, dw = NULL */
#define ORBIT_DWBWD_DGRAD_BN_WGRAD 2 /* orbit_op_dwconv2d_dgrad_bn with dw */
#define ORBIT_DWBWD_WGRAD 3          /* orbit_op_dwconv2d_backward, dw (the global-load form) */
#define ORBIT_DWBWD_WGRAD_XF 4       /* orbit_op_dwconv2d_wgrad_xf (the LDS form) */
/* family: 0 .. 3 = a forward kernel form as orbit_op_dwconv2d_plan numbers them, or one of: */
#define ORBIT_DWBWD_FAMILY_S2 4           /* the stride-2 kernel that owns 2x2 blocks of dx */
#define ORBIT_DWBWD_FAMILY_GATHER 5       /* the per-pixel gather fallback */
#define ORBIT_DWBWD_FAMILY_WGRAD_GLOBAL 6 /* filter gradient, taps loaded from global memory */
#define ORBIT_DWBWD_FAMILY_WGRAD_LDS 7    /* filter gradient from an LDS-staged patch (with the input transform) */
typedef struct orbit_dwconv_backward_plan {
    int family;
    int epilogue;   /* the BatchNorm-backward epilogue is carried */
    int wgrad;      /* the filter gradient is carried / computed */
    int blocks;     /* data gradient: row blocks of the launch (stride 2: blockIdx.x; forward forms: chunks * B) */
    int bn_rows;    /* [rows][2][C] BatchNorm partial rows written, 0 without the epilogue */
    int wgrad_rows; /* [rows][K*K][C] filter-gradient partial rows written, 0 when not carried */
    int chunks;     /* forward forms: row chunks per frame; global-load filter gradient: chunks of B * Ho rows; LDS: per frame */
    int rpc;        /* output rows per chunk */
    int cs4, tpb, groups; /* LDS filter gradient: channel quads per block, tiles per block, tile groups (= partial rows) */
} orbit_dwconv_backward_plan_t;
int orbit_op_dwconv2d_backward_plan(int B, int H, int W, int C, int K, int stride, int pad_top, int pad_left, int Ho, int Wo,
                                    int mode, orbit_dwconv_backward_plan_t* plan);
/* orbit_op_se_gate_backward with the producer's BatchNorm backward riding on it, as the reverse pass of an MBConv block runs the
 * two: x = act(y * scale[c] + shift[c]) [B][HW][C] is the activated output of a BatchNorm over the raw y (mean / invstd [C], the
 * batch or running statistics; scale = gamma * invstd, shift = beta - mean * scale). Step 1, the squeeze-excite backward, writes
 * g = d x * act'(.) (sums_only = 0; with sums_only != 0 pass g = NULL and nothing is written) and leaves the per-(frame, row chunk)
 * sums of g and g * xhat, which come back summed in sums [2][C]. Step 2 finishes the BatchNorm backward from them: dy [B][HW][C],
 * dgamma / dbeta [C] (nullable), train != 0 for batch statistics; with sums_only its apply pass rebuilds g from dxg, the gate and
 * the pooled-branch gradient. gamma nullable (= 1). dw1 .. db2: the SE parameter gradients, all or none. */
int orbit_op_se_gate_backward_bn(const float* dxg, const float* x, const float* y, const float* mean, const float* invstd,
                                 const float* scale, const float* shift, int act, const float* pooled, const float* w1,
                                 const float* b1, const float* w2, const float* b2, const float* gamma, int train, int sums_only,
                                 float* g, float* sums, float* dy, float* dgamma, float* dbeta, float* dw1, float* db1, float* dw2,
                                 float* db2, int B, int HW, int C, int R, orbit_stream_t stream);

/* ---- input side: 8-bit frames -> normalised fp32 NCHW ([B][3][H][W], what the extractors consume) -------------------
 * frames: device pointer, [B][H][W][3] when layout_hwc != 0 (decoded images) or [B][3][H][W]; mean3 / std3: HOST arrays.
 * out = ((u8 / 255) - mean) / std per channel: to_tensor + normalize of data/datasets.py:422-431, bit-identical. */
int orbit_frames_from_uint8(const uint8_t* frames, int layout_hwc, int B, int H, int W, const float* mean3,
                            const float* std3, float* out_nchw, orbit_stream_t stream);

/* The same for frames stored at another size than the extractor runs at: Pillow's 8-bit Image.resize((W_out, H_out), filter)
 * - the reference's offline scripts/resize_videos.py:46 pass, Image.LANCZOS - followed by the transform above, in one launch.
 * The resize is Pillow's integer arithmetic on Pillow's coefficient tables (orbit_resize_coeffs): horizontal pass, rounded and
 * clamped to 8 bits, then vertical pass, rounded and clamped; an axis whose size does not change is skipped. The resized
 * pixels equal Pillow's bit for bit, the output equals to_tensor + normalize of them. H and W take independent ratios, up or
 * down. The tables are built once per (device, in, out, filter) - a blocking upload on first use - and kept by the library;
 * calls may come from several threads.
 * Limits (ORBIT_ERR_ARG with a message, nothing launched): every side is at most ORBIT_RESIZE_MAX_SIZE, and a tile's working
 * set fits 64 KB of LDS: 96 bytes for every input row under the vertical window of one output row - min(H_in, 2 * ceil(S *
 * max(H_in / H_out, 1)) + 1) rows, S = 1 / 2 / 3 for bilinear / bicubic / lanczos - plus one input row of the columns under the
 * horizontal windows of 32 output columns (3 bytes per pixel). Lanczos 1080 -> 32 on both axes (a 205-row window, 1080 columns)
 * takes 23 KB of it, 32 -> 1080 under 1 KB; an 80-fold lanczos reduction of both axes of a 2560-pixel frame still fits (54 KB). */
#define ORBIT_RESIZE_BILINEAR 0
#define ORBIT_RESIZE_BICUBIC 1
#define ORBIT_RESIZE_LANCZOS 2
#define ORBIT_RESIZE_MAX_SIZE 16384
int orbit_frames_resize_from_uint8(const uint8_t* frames, int layout_hwc, int B, int H_in, int W_in, int H_out, int W_out,
                                   int filter /* ORBIT_RESIZE_* */, const float* mean3, const float* std3, float* out_nchw,
                                   orbit_stream_t stream);
/* Host only, no GPU: one axis' table of Pillow's 8-bit resampling from in_size to out_size pixels (Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc), the table the launcher above uploads. *ksize = 2 * ceil(S * max(in / out, 1)) + 1
 * is always written; with kk == NULL that is all (size the arrays with it), else output index i reads the inputs
 * xmin[i] .. xmin[i] + count[i] - 1 with the weights kk[i * ksize + 0 .. count[i]) (22 fractional bits; zero behind count[i]):
 * out = clamp(((1 << 21) + sum px * kk) >> 22, 0, 255) in 32-bit integers. */
int orbit_resize_coeffs(int in_size, int out_size, int filter, int* ksize, int32_t* kk /* [out][ksize] or NULL */,
                        int* xmin /* [out] */, int* count /* [out] */);

/* ---- JPEG decode on the device (csrc/jpeg.hip, csrc/jpeg_core.h) -------------------------------------------------------
 * Baseline sequential JPEG files -> 8-bit RGB frames [B][H][W][3], the layout the two launchers above take with layout_hwc = 1;
 * the pixels equal np.asarray(Image.open(f).convert("RGB")) of Pillow / libjpeg(-turbo) bit for bit: libjpeg's integer
 * "islow" inverse DCT, its triangle ("fancy") chroma upsampling and its YCbCr -> RGB tables. In scope: SOF0, 8-bit samples,
 * Huffman coding, one interleaved scan, 1 component or 3 components YCbCr with luma sampled 1x1, 2x1 or 2x2 and chroma 1x1,
 * 8-bit quantisation tables, any restart interval, sides up to ORBIT_RESIZE_MAX_SIZE. Everything else is the caller's to
 * decode on the host (orbit_jpeg_parse says which files).
 *
 * The descriptor of one file. orbit_jpeg_parse fills everything but file_offset, which the caller sets to the file's first byte
 * in the arena it uploads. Tables are in decode form: qt[c] is component c's quantisation table in natural (row-major) order;
 * huff[0..1] are the DC tables, huff[2..3] the AC tables the scan uses, dc_slot[c] / ac_slot[c] (0 or 1) select component c's.
 * A code of length l and value c <= maxcode[l] is the symbol huffval[(valptr[l] + c) & 255] (maxcode[l] = -1: no code of that
 * length); look[next 8 bits] = (length << 8) | symbol for the codes of at most 8 bits, 0 for longer ones. */
#define ORBIT_JPEG_STAGE_BYTES 1024 /* the entropy kernel stages the byte stream through LDS in tiles of this many bytes */
typedef struct orbit_jpeg_huff {
    int32_t maxcode[18];
    int32_t valptr[17];
    uint8_t huffval[256];
    uint16_t look[256];
} orbit_jpeg_huff_t;
typedef struct orbit_jpeg_desc {
    uint64_t file_offset;          /* of the file's first byte in the arena (set by the caller) */
    uint32_t ecs_offset;           /* of the entropy-coded segment in the file: the byte behind the SOS header */
    uint32_t ecs_bytes;            /* from there to the end of the file; the decoder stops at the EOI marker */
    int32_t status;                /* what orbit_jpeg_parse returned: 0 = decode on the device, > 0 = skip (host decode) */
    int32_t width, height, ncomp;
    int32_t hs[3], vs[3];          /* sampling factors of the components */
    int32_t dc_slot[3], ac_slot[3];
    int32_t restart_interval;      /* in MCUs, 0 = none */
    int32_t reserved;
    uint16_t qt[3][64];
    orbit_jpeg_huff_t huff[4];
} orbit_jpeg_desc_t;
/* orbit_jpeg_parse's positive return codes: why the file is out of the device path's scope */
#define ORBIT_JPEG_PROGRESSIVE 1   /* SOF2 */
#define ORBIT_JPEG_ARITHMETIC 2    /* SOF9 .. SOF15 */
#define ORBIT_JPEG_SOF_OTHER 3     /* extended sequential, lossless, hierarchical */
#define ORBIT_JPEG_PRECISION 4     /* not 8-bit samples */
#define ORBIT_JPEG_COMPONENTS 5    /* neither 1 nor 3 components (CMYK / YCCK) */
#define ORBIT_JPEG_COLORSPACE 6    /* an Adobe marker without JFIF, or components named R, G, B */
#define ORBIT_JPEG_SAMPLING 7      /* sampling factors other than 4:4:4, 4:2:2, 4:2:0 */
#define ORBIT_JPEG_DQT16 8         /* a 16-bit quantisation table */
#define ORBIT_JPEG_MULTISCAN 9     /* the first scan does not hold all components in frame order, or is not 0..63 */
#define ORBIT_JPEG_TABLES 10       /* a table the scan names is missing or malformed, or it uses more than 2 + 2 Huffman tables */
#define ORBIT_JPEG_SIZE 11         /* a side is 0 or exceeds ORBIT_RESIZE_MAX_SIZE */
/* Host only, no GPU: parse the headers of one file up to its first scan into *desc (desc_bytes = sizeof(orbit_jpeg_desc_t),
 * checked). Returns 0 when the device path decodes the file, one of the codes above when the host has to (width, height and
 * ncomp are filled in once the frame header was seen, 0 before), ORBIT_ERR_ARG with a message when the buffer is not a JPEG
 * file or a header runs past its end. Every length in the file is checked against `bytes`. Reentrant. */
int orbit_jpeg_parse(const uint8_t* data, size_t bytes, orbit_jpeg_desc_t* desc, size_t desc_bytes);
/* bits of a frame's decode status (0 = the frame was decoded and equals libjpeg's output) */
#define ORBIT_JPEG_ST_OVERRUN 1    /* the stream ended, or a marker came, before the last block */
#define ORBIT_JPEG_ST_CODE 2       /* no Huffman code within 16 bits */
#define ORBIT_JPEG_ST_INDEX 4      /* a coefficient index past 63 */
#define ORBIT_JPEG_ST_RESTART 8    /* not the expected restart marker, or bytes in front of it */
#define ORBIT_JPEG_ST_RANGE 16     /* a value outside the range in which libjpeg's variants agree with each other */
#define ORBIT_JPEG_ST_TRAILING 32  /* the last block is not followed by EOI */
#define ORBIT_JPEG_ST_DESC 64      /* the descriptor contradicts itself, the call's H x W or the arena */
/* Workspace of one launch of B frames of H x W: coefficients (2 bytes) and component planes (1 byte) of every frame at the
 * largest block count a sampling in scope gives. orbit_frames_from_jpeg works in chunks of frames when handed less, down to
 * orbit_jpeg_workspace_bytes(1, H, W). 0 for bad sizes. */
size_t orbit_jpeg_workspace_bytes(int B, int H, int W);
/* arena: device buffer of arena_bytes holding the files; descs: device copy of the B descriptors; out_u8_hwc [B][H][W][3];
 * status [B] int32, written for every frame: 0, ORBIT_JPEG_ST_* bits, or -code for a frame whose descriptor's status is a
 * non-zero code (skipped: its pixels are left untouched). All frames are H x W; one that is not gets ORBIT_JPEG_ST_DESC.
 * Three kernels per chunk: entropy decode (one wave per frame), dequantisation + inverse DCT, upsampling + colour
 * conversion. A frame written with restart markers (Pillow's restart_marker_rows / restart_marker_blocks, tools/resize_videos.py
 * --restart_rows) is entropy-decoded with one lane per restart interval, 64 intervals at a time, when its markers are exactly
 * the ones its geometry calls for: RST0, RST1, .. between the ceil(MCUs / restart_interval) intervals, then EOI, 2 to 1024
 * intervals. Every other frame - no markers, one interval, more than 1024, a marker missing, doubled or out of order - is
 * walked by one lane from the first byte to the last, and so is a frame any of whose intervals ends with a status: pixels and
 * status do not depend on which way a frame went. A frame without restart markers takes the subsequence-parallel form by its
 * production rule (orbit_op_jpeg_entropy_sub below, a second launch behind the first), with the same guarantee. No read leaves the arena, no write leaves the frame's own slice of the
 * workspace and of the output, whatever the file holds. */
int orbit_frames_from_jpeg(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W,
                           uint8_t* out_u8_hwc, int32_t* status, void* workspace, size_t workspace_bytes, orbit_stream_t stream);
/* The entropy kernel of orbit_frames_from_jpeg on its own, for parity tests: arena, descs, B, H, W and status as above.
 * form 0 walks every frame serially, form 1 applies the rule above. coef_out: the quantised coefficients as int16, per frame
 * 3 * (2 * ceil(W / 16)) * (2 * ceil(H / 16)) blocks of 64 in natural order (the frame's component planes of whole blocks one
 * behind the other, the rest of the slice untouched), 16-byte aligned; coef_bytes is checked against B, H and W before anything
 * is launched. taken [B] int32: 0 = walked serially, 1 = one lane per restart interval, 2 = that was tried, an interval ended
 * with a status, and the frame was walked serially again. */
int orbit_op_jpeg_entropy(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W, int form,
                          int16_t* coef_out, size_t coef_bytes, int32_t* status, int32_t* taken, orbit_stream_t stream);
/* The entropy stage as orbit_frames_from_jpeg launches it, for parity tests: the kernel above with form 1, which leaves the
 * frames of the subsequence-parallel form alone, and behind it the kernel of that form. A frame WITHOUT restart markers whose
 * entropy-coded segment makes N = ceil(ecs_bytes / S) subsequences of S bytes, 2 <= N <= 1024, is decoded by one block of 256
 * threads, one thread per subsequence at a time: every subsequence is walked from a guessed state (its first byte, first
 * block of the MCU, DC next), the exit of each replaces the entry of the next in rounds until nothing changes - at most N
 * rounds, in practice few, since Huffman streams self-synchronise - and a last pass writes the coefficients from the final
 * entries, block ordinals and DC predictors coming from an exclusive scan (csrc/jpeg_core.h). When a check fails - block
 * total, block index at an entry, EOI behind the last block, any status - the frame is walked serially again: status and
 * coefficients never depend on the form. sub_bytes: 0 = the production rule (S = 128, doubled until N <= 256, the
 * threads of the block; segments under 512 bytes and frames of fewer than 64 MCUs are walked serially), >= 4 = that S; 1 .. 3 and negative values are refused.
 * Arguments as above, all checked before anything is launched. taken [B] int32: 0 .. 2 as above, 3 = one walker per
 * subsequence, 4 = that was tried, a check failed, and the frame was walked serially again. rounds [B] int32: the rounds the
 * frame took (1 .. N; they depend on the file and on S alone), 0 when the form was not taken. */
int orbit_op_jpeg_entropy_sub(const uint8_t* arena, size_t arena_bytes, const orbit_jpeg_desc_t* descs, int B, int H, int W, int sub_bytes,
                              int16_t* coef_out, size_t coef_bytes, int32_t* status, int32_t* taken, int32_t* rounds,
                              orbit_stream_t stream);

/* ---- JPEG encode on the device (csrc/jpeg_enc.hip, csrc/jpeg_enc_core.h) --------------------------------------------------
 * 8-bit RGB frames [B][H][W][3] -> the files Pillow's Image.save(quality = q[, restart_marker_rows = r]) writes for them, byte
 * for byte: JFIF 1.01 header, an optional COM segment, 3-component YCbCr baseline SOF0 at 4:2:0, one interleaved scan, the
 * Annex-K Huffman tables; libjpeg's integer colour conversion, 2 x 2 chroma averaging, "islow" forward DCT and quantiser. With
 * orbit_frames_resize_u8 and orbit_frames_from_jpeg this is the reference's offline scripts/resize_videos.py pass on the device
 * (tools/resize_videos.py).
 *
 * The parameters of one encoding: quantisation tables in natural (row-major) order (0 luma, 1 chroma) with the reciprocals
 * ceil(2^32 / (8 qt)) the quantiser multiplies by, and the code tables of the four Huffman tables, indexed by DC category and
 * by AC run/size symbol: code << 5 | length, 0 where a symbol has no code. */
typedef struct orbit_jpeg_enc {
    int32_t quality, restart_rows; /* restart_rows: MCU rows per restart interval, 0 = no restart markers */
    uint16_t qt[2][64];
    uint32_t qrecip[2][64];
    uint32_t dc[2][16];
    uint32_t ac[2][256];
} orbit_jpeg_enc_t;
/* Host only: fill *p (p_bytes = sizeof(orbit_jpeg_enc_t), checked) for libjpeg's jpeg_set_quality(quality, force_baseline).
 * ORBIT_ERR_ARG for a quality outside 1 .. 100 or negative restart_rows. */
int orbit_jpeg_encode_params(int quality, int restart_rows, orbit_jpeg_enc_t* p, size_t p_bytes);
/* Host only: the header of an H x W file - SOI, APP0, COM (comment_bytes > 0 only), DQT x 2, SOF0, DHT x 4, DRI (restart_rows
 * > 0 only; rows x MCUs per row must fit 16 bits), SOS - into out [cap]. Returns its length, or ORBIT_ERR_ARG (a comment of
 * more than 65533 bytes, a short `out`, bad sizes). */
int orbit_jpeg_encode_header(const orbit_jpeg_enc_t* p, int H, int W, const uint8_t* comment, size_t comment_bytes, uint8_t* out,
                             size_t cap);
/* A file size no H x W frame can exceed, whatever its pixels (0 for bad sizes): a block codes to at most 22 + 63 * 26 = 1660
 * bits and is given 1664, which also pays for the fill bits of every restart interval; byte stuffing at most doubles the
 * scan; 3 bytes per restart interval; the header with a comment of comment_bytes; EOI. */
size_t orbit_jpeg_encode_bound(int H, int W, int restart_rows, size_t comment_bytes);
/* Workspace of one launch of B frames: planes, coefficients, bit sums, the unstuffed bit buffer (about 2.6 KB per 16 x 16
 * pixels). orbit_frames_to_jpeg works in chunks of frames when handed less, down to the workspace of one frame. 0 for bad sizes. */
size_t orbit_jpeg_encode_workspace_bytes(int B, int H, int W);
/* frames_u8_hwc [B][H][W][3], out, out_bytes [B] and workspace (16-byte aligned) are device pointers; params is a HOST
 * pointer, read before the call returns. Frame b's file is written to out + b * out_stride and its length to out_bytes[b].
 * Comments: frame b carries the COM segment comments[comment_offsets[b] .. comment_offsets[b + 1]) when that range is not empty;
 * `comments` is a DEVICE buffer, comment_offsets a HOST array of B + 1 nondecreasing offsets (both NULL: no comments).
 * out_stride must be at least orbit_jpeg_encode_bound(H, W, restart_rows, longest comment): with that no frame can overflow
 * its slice, so there is no device-side overflow path. Sides up to ORBIT_RESIZE_MAX_SIZE, and 6 * ceil(H / 16) * ceil(W / 16)
 * * 1664 bits must fit 32 bits (about 10 000 x 10 000 pixels). Seven kernels per chunk of at most 512 frames: colour
 * conversion + chroma downsampling, forward DCT + quantisation, bits per block, their prefix sum per frame, bit packing,
 * FF count + prefix sum, byte stuffing + file assembly. No read leaves the frames, no write leaves a frame's own slice of the
 * workspace and of `out`. */
int orbit_frames_to_jpeg(const uint8_t* frames_u8_hwc, int B, int H, int W, const orbit_jpeg_enc_t* params,
                         const uint8_t* comments, const uint32_t* comment_offsets, uint8_t* out, size_t out_stride,
                         uint32_t* out_bytes, void* workspace, size_t workspace_bytes, orbit_stream_t stream);
/* The B files of such a call one behind the other, so that the host fetches the compressed bytes and not B slices: packed
 * (device, packed_cap >= the sum of the lengths; B * out_stride always suffices) receives them, offsets (device, [B + 1]) the
 * first byte of each and, last, the total. A file that would run past packed_cap is not copied (its offset is still written). */
int orbit_jpeg_compact(const uint8_t* out, size_t out_stride, const uint32_t* out_bytes, int B, uint8_t* packed,
                       size_t packed_cap, uint32_t* offsets, orbit_stream_t stream);
/* orbit_frames_resize_from_uint8's resize with an 8-bit store: out_u8_hwc [B][H_out][W_out][3] equals
 * np.asarray(Image.resize((W_out, H_out), filter)) of every frame. Same tables, same limits. */
int orbit_frames_resize_u8(const uint8_t* frames, int layout_hwc, int B, int H_in, int W_in, int H_out, int W_out,
                           int filter /* ORBIT_RESIZE_* */, uint8_t* out_u8_hwc, orbit_stream_t stream);

/* ---- measurement: per-launch HIP-event timing of the dominant kernel (conv_igemm, all variants) ---- */
int orbit_prof_enable(int on);   /* on: reset and start recording an event pair per launch on its stream */
/* waits for the recorded launches, returns summed duration, summed ALGORITHMIC flops and launch count */
int orbit_prof_collect(double* total_ms, double* total_flops, long* launches);
int orbit_prof_num_variants(void);
/* one row per kernel instantiation: launches, summed duration, summed algorithmic flops and algorithmic HBM bytes */
int orbit_prof_variant(int i, char* name48, long* launches, double* ms, double* flops, double* bytes);
/* The roofs a launch's floor is priced on (defaults: 6.3e12 B/s achievable HBM, 157.3e12 FLOP/s fp32 MFMA, 5.93e12 SiLU
 * evaluations/s = 11.06 ns of a SIMD per 64 of them x 1024 SIMDs; set before orbit_prof_collect) and, per row, the sum over
 * its launches of max(bytes / HBM rate, FLOP / matrix rate), the same with the SiLU evaluations' VALU time added to the
 * matrix time (a gfx950 SIMD issues either an MFMA or VALU instructions, never both), and the SiLU count. Round 6: every
 * launch of the inference path - depthwise, squeeze-excite gate, pooling, head kernels included - records a row (bench.py
 * roofline.families). */
int orbit_prof_set_roofs(double hbm_bytes_per_s, double matrix_flop_per_s, double silu_evals_per_s);
int orbit_prof_variant_floor(int i, double* floor_ms, double* floor_simd_ms, double* silu_evals);

/* ---- RCCL over xGMI (one process per GPU) ------------------------------------------------------- */
/* The reference has no collectives; this is the exchange step of the support-sharded variant: the
 * all-reduce(SUM) of orbit_proto_configure's sums/counts (and of set-encoder embedding sums). */
#define ORBIT_COMM_ID_BYTES 128
int orbit_comm_unique_id(void* out128);                       /* rank 0: create the rendezvous id */
int orbit_comm_init(int rank, int world, const void* unique_id);
int orbit_comm_world(void);
int orbit_comm_rank(void);
int orbit_allreduce_sum(float* buf, size_t n, orbit_stream_t stream);  /* in place */
void orbit_comm_destroy(void);

/* ---- one-shot peer-to-peer all-reduce(SUM) over xGMI for the SMALL exchange steps (csrc/comm.hip) -----------------
 * The prototype payload of a support-sharded task is 25.6 KB: a latency-bound message. Every rank pushes its payload
 * into a slot of every peer's inbox (IPC-mapped device memory, all xGMI links in parallel), raises a flag and sums the
 * world slots of its own inbox in rank order: one hop, bit-identical result on every rank. orbit_allreduce_sum (RCCL)
 * stays the baseline and the path for large buffers.
 *   create (every rank) -> export 64-byte IPC handle -> exchange handles (host side) -> connect -> allreduce ... */
#define ORBIT_P2P_HANDLE_BYTES 64
typedef struct orbit_p2p orbit_p2p_t;
int orbit_p2p_create(int rank, int world, size_t max_floats, orbit_p2p_t** out);
int orbit_p2p_export(orbit_p2p_t* c, void* handle64);
int orbit_p2p_connect(orbit_p2p_t* c, const void* handles /* [world][64], own entry ignored */);
int orbit_p2p_allreduce_sum(orbit_p2p_t* c, float* buf, size_t n, orbit_stream_t stream); /* in place, n <= max_floats */
/* Large payloads (the flat gradient bucket of the task-parallel LITE step, reference single-step-learner.py:162-166,231
 * under data parallelism): direct reduce-scatter + all-gather over the point-to-point mesh, every element
 * summed once in rank order (bit-identical on all ranks). In place; n <= world * max_floats / 2. */
int orbit_p2p_allreduce_sum_sharded(orbit_p2p_t* c, float* buf, size_t n, orbit_stream_t stream);
/* 0 ok; k > 0: a wait for rank (k-1) % 100's flag timed out (~4 s) and that all-reduce's buffer was filled with NaN instead
 * of a partial sum. Reads a host-mapped word, does not synchronise the device: it covers the all-reduces that have completed. */
int orbit_p2p_error(orbit_p2p_t* c);
/* How the inbox was allocated. Peers write it and the owner polls it while kernels run, so it must be uncached or
 * fine-grained device memory (coarse-grained memory is only coherent at kernel boundaries); orbit_p2p_create fails rather
 * than fall back to coarse-grained memory unless ORBIT_P2P_ALLOW_COARSE=1. */
#define ORBIT_P2P_MEM_UNCACHED 1
#define ORBIT_P2P_MEM_FINEGRAINED 2
#define ORBIT_P2P_MEM_COARSE 3
int orbit_p2p_memory_kind(orbit_p2p_t* c);
void orbit_p2p_destroy(orbit_p2p_t* c);

#ifdef __cplusplus
}
#endif
#endif /* ORBIT_HIP_H */
