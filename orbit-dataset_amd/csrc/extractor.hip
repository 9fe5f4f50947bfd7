// Network runtime: builds a static launch plan for "resnet18", "efficientnet_b0", "efficientnet_v2_s" or "set_encoder" at a
// given frame size, owns the parameters (loaded by torch state_dict key), repacks conv weights for the
// MFMA kernel, folds BatchNorm (+ per-task FiLM gamma/beta) into per-channel scale/shift, and replays the
// plan on a HIP stream. This is the native counterpart of
//   model/feature_extractors.py:37-79   create_feature_extractor (timm tf_efficientnet_b0 and tf_efficientnetv2_s_in21k;
//                                        resnet18 is the torchvision-layout network BASELINE.json's configs name)
//   model/set_encoders.py:81-120        SimplePrePoolNet
//   model/few_shot_recognisers.py:99-153 _get_features[_in_batches] (one call = one mini-batch of frames)
//   model/film.py:38-74                 which BatchNorms are FiLM-modulated
// Activations are NHWC fp32 and live in caller-provided workspace (three rotating buffers); frames come
// in as NCHW (the reference's clip layout) and are consumed directly by the stem convolution.
#include <chrono>
#include <cstdlib>

#include "extractor.h"

using namespace orbit;

static int conv_out(int H, int K, int stride, int pad) { return (H + 2 * pad - K) / stride + 1; }
static void same_pad(int H, int K, int stride, int& Ho, int& pad_before) {  // TF "SAME"
    Ho = (H + stride - 1) / stride;
    const int total = std::max((Ho - 1) * stride + K - H, 0);
    pad_before = total / 2;
}

// ---- resnet18 (torchvision layout, pooled 512-d features; every BatchNorm is a FiLM slot) -------
static int build_resnet18(orbit_extractor* fe, int H, int W) {
    fe->out_size = 512;
    int h = conv_out(H, 7, 2, 3), w = conv_out(W, 7, 2, 3);
    int bn = fe->add_bn("bn1", 64, 1e-5f, true);
    fe->add_conv("conv1.weight", bn, -1, 0, -1, H, W, 3, 64, 7, 2, 3, 3, h, w, ORBIT_ACT_RELU, 0, 1, 0);
    {
        Op o;
        o.kind = OP_MAXPOOL, o.in = 0, o.out = 1, o.H = h, o.W = w, o.Cin = 64, o.Cout = 64;
        o.pool_k = 3, o.stride = 2, o.pool_pad = 1;
        o.Ho = conv_out(h, 3, 2, 1), o.Wo = conv_out(w, 3, 2, 1);
        h = o.Ho, w = o.Wo;
        fe->note_buf(1, (size_t)h * w * 64);
        fe->ops.push_back(o);
    }
    int cur = 1, cin = 64;
    const int widths[4] = {64, 128, 256, 512};
    for (int L = 0; L < 4; ++L) {
        for (int blk = 0; blk < 2; ++blk) {
            const int cout = widths[L];
            const int stride = (L > 0 && blk == 0) ? 2 : 1;
            const std::string p = "layer" + std::to_string(L + 1) + "." + std::to_string(blk);
            const int ho = conv_out(h, 3, stride, 1), wo = conv_out(w, 3, stride, 1);
            const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
            // module registration order: conv1, bn1, conv2, bn2, downsample.{0,1}
            const int bn1 = fe->add_bn(p + ".bn1", cout, 1e-5f, true);
            fe->add_conv(p + ".conv1.weight", bn1, cur, t1, -1, h, w, cin, cout, 3, stride, 1, 1, ho, wo,
                         ORBIT_ACT_RELU, 0, 0, 0);
            const int bn2 = fe->add_bn(p + ".bn2", cout, 1e-5f, true);
            int res = cur;
            if (stride != 1 || cin != cout) {
                const int bnd = fe->add_bn(p + ".downsample.1", cout, 1e-5f, true);
                // conv2 is emitted after the downsample so the plan order is ds -> conv2; param order
                // (state_dict) is irrelevant to execution
                fe->add_conv(p + ".downsample.0.weight", bnd, cur, t2, -1, h, w, cin, cout, 1, stride, 0, 0, ho,
                             wo, ORBIT_ACT_NONE, 0, 0, 0);
                res = t2;
            }
            // out = relu(bn2(conv2(t1)) + res); write into the buffer that is neither t1 nor res
            const int outb = (res == cur) ? t2 : cur;
            fe->add_conv(p + ".conv2.weight", bn2, t1, outb, res, ho, wo, cout, cout, 3, 1, 1, 1, ho, wo,
                         ORBIT_ACT_RELU, 0, 0, 0);
            cur = outb, cin = cout, h = ho, w = wo;
        }
    }
    Op o;
    o.kind = OP_AVGPOOL, o.in = cur, o.out = BUF_FEATS, o.H = h, o.W = w, o.Cin = 512, o.Cout = 512;
    fe->ops.push_back(o);
    return ORBIT_OK;
}

// ---- MBConv pieces shared by the EfficientNet builders ---------------------------------------------
static int param_of(orbit_extractor* fe, const std::string& key, size_t numel) {  // (a builder may have registered it already)
    const int k = fe->pool.find(key);
    return k >= 0 ? k : fe->add_param(key, numel);
}
// depthwise K x K (TF "SAME") + BatchNorm + SiLU, emitting the squeeze-excite pooling partials
static void add_dw(orbit_extractor* fe, const std::string& wkey, int bnidx, int in, int out, int C, int K, int stride, int hh,
                   int ww, int& ho, int& wo) {
    Op o;
    o.kind = OP_DWCONV, o.in = in, o.out = out, o.H = hh, o.W = ww, o.Cin = C, o.Cout = C;
    o.KH = o.KW = K, o.stride = stride, o.act = ORBIT_ACT_SILU, o.bn = bnidx;
    same_pad(hh, K, stride, o.Ho, o.pad_t);
    same_pad(ww, K, stride, o.Wo, o.pad_l);
    o.weight = param_of(fe, wkey, (size_t)C * K * K);
    o.packed_off = fe->packed_floats;
    fe->packed_floats += (size_t)(C * K * K + 3) / 4 * 4;
    o.pool_partial = 1;
    fe->max_partial = std::max(fe->max_partial, (size_t)dwconv_se_chunks(o.Ho) * C);
    ho = o.Ho, wo = o.Wo;
    fe->note_buf(out, (size_t)ho * wo * C);
    fe->macs += (double)ho * wo * C * K * K;
    fe->ops.push_back(o);
}
// squeeze-excite gate of C channels through R hidden units; the pooled sums come from the depthwise kernel's partials
// (BUF_POOLED), not from a re-read of the tensor
static void add_se(orbit_extractor* fe, const std::string& p, int C, int R, int hh, int ww, int chunks) {
    Op s;
    s.kind = OP_SE, s.in = BUF_POOLED, s.out = BUF_GATE, s.Cin = C, s.R = R;
    s.se_chunks = chunks, s.se_hw = hh * ww;
    s.packed_off = fe->packed_floats;  // W2 transposed to [R][C]
    fe->packed_floats += (size_t)(C * R + 3) / 4 * 4;
    s.se_w1 = fe->add_param(p + ".conv_reduce.weight", (size_t)R * C);
    s.se_b1 = fe->add_param(p + ".conv_reduce.bias", R);
    s.se_w2 = fe->add_param(p + ".conv_expand.weight", (size_t)C * R);
    s.se_b2 = fe->add_param(p + ".conv_expand.bias", C);
    fe->macs += 2.0 * C * R;
    fe->max_se_c = std::max(fe->max_se_c, C);
    fe->ops.push_back(s);
}

// ---- efficientnet_b0, timm `tf_` variant (SAME padding, BN eps 1e-3), num_classes=0 --------------
static int build_efficientnet_b0(orbit_extractor* fe, int H, int W, bool unfused) {
    fe->out_size = 1280;
    const float eps = 1e-3f;
    // expand 1x1 + BatchNorm + SiLU + depthwise + BatchNorm + SiLU as ONE row-streaming kernel (csrc/mbconv_rows.hip; option
    // mbconv_rows, default on) for the 112x112 .. 28x28 stages, where the 6x-expanded tensor would otherwise make an HBM round
    // trip; the 14x14 / 7x7 stages run the MFMA conv + LDS-patch depthwise pair
    // (a plan that records a tape - `unfused` - keeps the pair everywhere: the fused kernels have no backward form)
    const int rows_opt = unfused ? 0 : get_option("mbconv_rows");
    auto fuse_front_ok = [&](int hh, int ww, int cin, int mid, int K, int stride) {
        return rows_opt != 0 && mbconv_rows_supported(hh, ww, cin, mid, K, stride);
    };
    int h, w, pt, pl;
    same_pad(H, 3, 2, h, pt);
    same_pad(W, 3, 2, w, pl);
    int bn = fe->add_bn("bn1", 32, eps, true);  // root bn1 is FiLM-tagged (film.py:45-46)
    // row-streaming stem + first depthwise (csrc/mbconv_rows.hip, option stem_rows): the stem's 112x112x32 output stays in LDS
    const bool fuse_stem = rows_opt != 0 && get_option("stem_rows") != 0 && stem_rows_supported(h, w, 32, 3, 1);
    size_t stem_weight = 0;
    if (fuse_stem) stem_weight = fe->add_param("conv_stem.weight", (size_t)32 * 27);
    else fe->add_conv("conv_stem.weight", bn, -1, 0, -1, H, W, 3, 32, 3, 2, pt, pl, h, w, ORBIT_ACT_SILU, 0, 1, 0);
    int cur = 0, cin = 32;

    // stage 0: DepthwiseSeparableConv (not FiLM-tagged, film.py:41-48)
    {
        const std::string p = "blocks.0.0";
        int ho, wo;
        const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
        // registration order: conv_dw, bn1, se, conv_pw, bn2
        // conv_dw param is registered inside add_dw, bn1 after it: keep state_dict order cosmetic only
        const int bn1 = fe->add_bn(p + ".bn1", 32, eps, false);
        int se_chunks0;
        if (fuse_stem) {
            Op o;
            o.kind = OP_MBFRONT, o.stem = true, o.in = -1, o.out = t1, o.H = h, o.W = w, o.Cin = 32, o.Cout = 32;
            o.KH = o.KW = 3, o.stride = 1, o.bn = bn, o.bn2 = bn1;
            o.stem_h = H, o.stem_w = W, o.stem_pt = pt, o.stem_pl = pl;
            same_pad(h, 3, 1, o.Ho, o.pad_t);
            same_pad(w, 3, 1, o.Wo, o.pad_l);
            o.weight = stem_weight;
            o.weight2 = fe->add_param(p + ".conv_dw.weight", (size_t)32 * 9);
            o.packed_off = fe->packed_floats;   // depthwise taps [3][3][32]
            fe->packed_floats += (size_t)32 * 9;
            o.packed_off2 = fe->packed_floats;  // stem filter [32][32]
            fe->packed_floats += (size_t)32 * 32;
            ho = o.Ho, wo = o.Wo;
            o.rows = true;
            se_chunks0 = stem_rows_tiles(h, w);
            o.se_chunks = se_chunks0;  // what the pooling buffer and the gate were sized for (checked at launch)
            fe->max_partial = std::max(fe->max_partial, (size_t)se_chunks0 * 32);
            fe->note_buf(t1, (size_t)ho * wo * 32);
            fe->macs += (double)h * w * 27 * 32 + (double)ho * wo * 32 * 9;
            fe->ops.push_back(o);
        } else {
            add_dw(fe, p + ".conv_dw.weight", bn1, cur, t1, 32, 3, 1, h, w, ho, wo);
            se_chunks0 = dwconv_se_chunks(ho);
        }
        add_se(fe, p + ".se", 32, 8, ho, wo, se_chunks0);
        const int bn2 = fe->add_bn(p + ".bn2", 16, eps, false);
        fe->add_conv(p + ".conv_pw.weight", bn2, t1, t2, -1, ho, wo, 32, 16, 1, 1, 0, 0, ho, wo, ORBIT_ACT_NONE,
                     0, 0, 1);
        cur = t2, cin = 16, h = ho, w = wo;
    }
    // stages 1..6: InvertedResidual  {repeats, kernel, stride, out channels}, expansion 6, SE 0.25 of block input
    const int cfg[6][4] = {{2, 3, 2, 24}, {2, 5, 2, 40}, {3, 3, 2, 80}, {3, 5, 1, 112}, {4, 5, 2, 192}, {1, 3, 1, 320}};
    for (int s = 0; s < 6; ++s) {
        for (int r = 0; r < cfg[s][0]; ++r) {
            const int K = cfg[s][1], stride = r == 0 ? cfg[s][2] : 1, cout = cfg[s][3];
            const int mid = cin * 6;
            const int rd = (int)(cin * 0.25 + 0.5);  // timm: round(in_chs * se_ratio)
            const std::string p = "blocks." + std::to_string(s + 1) + "." + std::to_string(r);
            const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
            const bool skip = stride == 1 && cin == cout;
            int ho, wo;
            const int bn1 = fe->add_bn(p + ".bn1", mid, eps, false);
            int se_chunks;
            if (fuse_front_ok(h, w, cin, mid, K, stride)) {
                // expand + depthwise in one kernel: the 6x-expanded tensor never leaves LDS
                Op o;
                o.kind = OP_MBFRONT, o.in = cur, o.out = t2, o.H = h, o.W = w, o.Cin = cin, o.Cout = mid;
                o.KH = o.KW = K, o.stride = stride, o.bn = bn1;
                same_pad(h, K, stride, o.Ho, o.pad_t);
                same_pad(w, K, stride, o.Wo, o.pad_l);
                o.weight = fe->add_param(p + ".conv_pw.weight", (size_t)mid * cin);
                o.bn2 = fe->add_bn(p + ".bn2", mid, eps, true);  // InvertedResidual.bn2 is FiLM-tagged
                o.weight2 = fe->add_param(p + ".conv_dw.weight", (size_t)mid * K * K);
                o.packed_off = fe->packed_floats;
                fe->packed_floats += (size_t)(mid * K * K + 3) / 4 * 4;
                ho = o.Ho, wo = o.Wo;
                o.rows = true;
                se_chunks = mbconv_rows_tiles(h, w, cin, mid, K, stride);
                o.se_chunks = se_chunks;  // what the pooling buffer and the gate were sized for (checked at launch)
                fe->max_partial = std::max(fe->max_partial, (size_t)se_chunks * mid);
                fe->note_buf(t2, (size_t)ho * wo * mid);
                fe->macs += (double)h * w * cin * mid + (double)ho * wo * mid * K * K;
                fe->ops.push_back(o);
            } else {
                fe->add_conv(p + ".conv_pw.weight", bn1, cur, t1, -1, h, w, cin, mid, 1, 1, 0, 0, h, w, ORBIT_ACT_SILU,
                             0, 0, 0);
                const int bn2 = fe->add_bn(p + ".bn2", mid, eps, true);  // InvertedResidual.bn2 is FiLM-tagged
                add_dw(fe, p + ".conv_dw.weight", bn2, t1, t2, mid, K, stride, h, w, ho, wo);
                se_chunks = dwconv_se_chunks(ho);
            }
            add_se(fe, p + ".se", mid, rd, ho, wo, se_chunks);
            const int bn3 = fe->add_bn(p + ".bn3", cout, eps, false);
            // project: reads t2 (gated), residual from cur, writes t1 (free again)
            fe->add_conv(p + ".conv_pwl.weight", bn3, t2, t1, skip ? cur : -1, ho, wo, mid, cout, 1, 1, 0, 0, ho, wo,
                         ORBIT_ACT_NONE, 0, 0, 1);
            cur = t1, cin = cout, h = ho, w = wo;
        }
    }
    const int t1 = (cur + 1) % 3;
    bn = fe->add_bn("bn2", 1280, eps, true);  // root bn2 is FiLM-tagged
    fe->add_conv("conv_head.weight", bn, cur, t1, -1, h, w, cin, 1280, 1, 1, 0, 0, h, w, ORBIT_ACT_SILU, 0, 0, 0);
    Op o;
    o.kind = OP_AVGPOOL, o.in = t1, o.out = BUF_FEATS, o.H = h, o.W = w, o.Cin = 1280, o.Cout = 1280;
    fe->ops.push_back(o);
    return ORBIT_OK;
}

// ---- efficientnet_v2_s, timm `tf_efficientnetv2_s_in21k` (SAME padding, BN eps 1e-3), num_classes=0 -----------------
// stem 3 -> 24 /2 | cn_r2_k3_s1_e1_c24_skip | er_r4_k3_s2_e4_c48 | er_r4_k3_s2_e4_c64 | ir_r6_k3_s2_e4_c128_se0.25 |
// ir_r9_k3_s1_e6_c160_se0.25 | ir_r15_k3_s2_e6_c256_se0.25 | head 256 -> 1280, global average pool.
// Parameters are registered in timm's module order (conv before its BatchNorm), so the enumeration IS the checkpoint's
// state_dict order. FiLM slots (model/film.py:38-56): root bn1 / bn2, bn1 of every ConvBnAct and EdgeResidual, bn2 of every
// InvertedResidual. Every block is the plain conv (+ depthwise + squeeze-excite) sequence of the kernels efficientnet_b0 runs
// at 14x14 / 7x7; the one new device form is ConvBnAct's skip, which joins AFTER the activation (Op::res_post). The training
// runtime walks it only on a plan created with ORBIT_PLAN_RES_POST_BACKWARD - then in frozen form only: running statistics, no
// filter gradients - or with ORBIT_PLAN_RES_POST_TRAINING, which opens batch statistics and every parameter gradient
// (plan_trainable / plan_frozen_only, csrc/extractor_train.hip).
static int build_efficientnet_v2_s(orbit_extractor* fe, int H, int W) {
    fe->out_size = 1280;
    const float eps = 1e-3f;
    int h, w, pt, pl;
    same_pad(H, 3, 2, h, pt);
    same_pad(W, 3, 2, w, pl);
    fe->add_param("conv_stem.weight", (size_t)24 * 27);
    int bn = fe->add_bn("bn1", 24, eps, true);  // root bn1 is FiLM-tagged
    fe->add_conv("conv_stem.weight", bn, -1, 0, -1, H, W, 3, 24, 3, 2, pt, pl, h, w, ORBIT_ACT_SILU, 0, 1, 0);
    int cur = 0, cin = 24;
    // dense 3x3 conv (TF "SAME") + BatchNorm (+ SiLU) (+ skip, before or after the activation)
    auto conv3 = [&](const std::string& wkey, int bnidx, int in, int out, int res, int ci, int co, int stride, int act,
                     int res_post, int& ho, int& wo) {
        int ptt, pll;
        same_pad(h, 3, stride, ho, ptt);
        same_pad(w, 3, stride, wo, pll);
        fe->add_conv(wkey, bnidx, in, out, res, h, w, ci, co, 3, stride, ptt, pll, ho, wo, act, 0, 0, 0, -1, res_post);
    };
    // {kind (0 ConvBnAct, 1 EdgeResidual, 2 InvertedResidual), repeats, stride, expansion, out channels}
    const int cfg[6][5] = {{0, 2, 1, 1, 24}, {1, 4, 2, 4, 48}, {1, 4, 2, 4, 64}, {2, 6, 2, 4, 128}, {2, 9, 1, 6, 160}, {2, 15, 2, 6, 256}};
    for (int s = 0; s < 6; ++s) {
        for (int r = 0; r < cfg[s][1]; ++r) {
            const int kind = cfg[s][0], stride = r == 0 ? cfg[s][2] : 1, cout = cfg[s][4];
            const int mid = cin * cfg[s][3];
            const std::string p = "blocks." + std::to_string(s) + "." + std::to_string(r);
            const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
            const bool skip = stride == 1 && cin == cout;
            int ho, wo;
            if (kind == 0) {
                // ConvBnAct: x + silu(bn1(conv(x))) - the skip joins after the activation
                fe->add_param(p + ".conv.weight", (size_t)cout * cin * 9);
                const int bn1 = fe->add_bn(p + ".bn1", cout, eps, true);
                conv3(p + ".conv.weight", bn1, cur, t1, skip ? cur : -1, cin, cout, stride, ORBIT_ACT_SILU, skip ? 1 : 0, ho, wo);
                cur = t1;
            } else if (kind == 1) {
                // EdgeResidual: conv_exp 3x3 (carries the stride), bn1 + SiLU, conv_pwl 1x1, bn2 (+ x)
                fe->add_param(p + ".conv_exp.weight", (size_t)mid * cin * 9);
                const int bn1 = fe->add_bn(p + ".bn1", mid, eps, true);
                conv3(p + ".conv_exp.weight", bn1, cur, t1, -1, cin, mid, stride, ORBIT_ACT_SILU, 0, ho, wo);
                fe->add_param(p + ".conv_pwl.weight", (size_t)cout * mid);
                const int bn2 = fe->add_bn(p + ".bn2", cout, eps, false);
                fe->add_conv(p + ".conv_pwl.weight", bn2, t1, t2, skip ? cur : -1, ho, wo, mid, cout, 1, 1, 0, 0, ho, wo,
                             ORBIT_ACT_NONE, 0, 0, 0);
                cur = t2;
            } else {
                // InvertedResidual: conv_pw, bn1 + SiLU, conv_dw 3x3, bn2 + SiLU, squeeze-excite, gated conv_pwl, bn3 (+ x)
                const int rd = (int)(cin * 0.25 + 0.5);  // timm: round(in_chs * se_ratio)
                fe->add_param(p + ".conv_pw.weight", (size_t)mid * cin);
                const int bn1 = fe->add_bn(p + ".bn1", mid, eps, false);
                fe->add_conv(p + ".conv_pw.weight", bn1, cur, t1, -1, h, w, cin, mid, 1, 1, 0, 0, h, w, ORBIT_ACT_SILU, 0, 0, 0);
                fe->add_param(p + ".conv_dw.weight", (size_t)mid * 9);
                const int bn2 = fe->add_bn(p + ".bn2", mid, eps, true);  // InvertedResidual.bn2 is FiLM-tagged
                add_dw(fe, p + ".conv_dw.weight", bn2, t1, t2, mid, 3, stride, h, w, ho, wo);
                add_se(fe, p + ".se", mid, rd, ho, wo, dwconv_se_chunks(ho));
                fe->add_param(p + ".conv_pwl.weight", (size_t)cout * mid);
                const int bn3 = fe->add_bn(p + ".bn3", cout, eps, false);
                fe->add_conv(p + ".conv_pwl.weight", bn3, t2, t1, skip ? cur : -1, ho, wo, mid, cout, 1, 1, 0, 0, ho, wo,
                             ORBIT_ACT_NONE, 0, 0, 1);
                cur = t1;
            }
            cin = cout, h = ho, w = wo;
        }
    }
    const int t1 = (cur + 1) % 3;
    fe->add_param("conv_head.weight", (size_t)1280 * cin);
    bn = fe->add_bn("bn2", 1280, eps, true);  // root bn2 is FiLM-tagged
    fe->add_conv("conv_head.weight", bn, cur, t1, -1, h, w, cin, 1280, 1, 1, 0, 0, h, w, ORBIT_ACT_SILU, 0, 0, 0);
    Op o;
    o.kind = OP_AVGPOOL, o.in = t1, o.out = BUF_FEATS, o.H = h, o.W = w, o.Cin = 1280, o.Cout = 1280;
    fe->ops.push_back(o);
    return ORBIT_OK;
}

// ---- set encoder: 5 x (conv3x3 p1 + bias -> BN -> ReLU -> maxpool 2x2) -> global avg -> 64 ---------
static int build_set_encoder(orbit_extractor* fe, int H, int W) {
    fe->out_size = 64;
    int h = H, w = W, cur = -1, cin = 3;
    for (int L = 1; L <= 5; ++L) {
        if (h < 2 || w < 2) return set_err(ORBIT_ERR_ARG, "set_encoder: frame %dx%d too small for 5 poolings", H, W);
        const std::string p = "encoder.layer" + std::to_string(L);
        const int out = cur < 0 ? 0 : (cur + 1) % 3;
        const int wparam = fe->add_param(p + ".0.weight", (size_t)64 * cin * 9);
        (void)wparam;
        const int bias = fe->add_param(p + ".0.bias", 64);
        const int bn = fe->add_bn(p + ".1", 64, 1e-5f, false, bias);
        fe->add_conv(p + ".0.weight", bn, cur, out, -1, h, w, cin, 64, 3, 1, 1, 1, h, w, ORBIT_ACT_RELU, 1,
                     cur < 0 ? 1 : 0, 0, bias);
        cur = out, cin = 64, h /= 2, w /= 2;
    }
    Op o;
    o.kind = OP_AVGPOOL, o.in = cur, o.out = BUF_FEATS, o.H = h, o.W = w, o.Cin = 64, o.Cout = 64;
    fe->ops.push_back(o);
    return ORBIT_OK;
}

// ---- workspace layout ------------------------------------------------------------------------------
struct WsLayout {
    size_t buf[3], pooled, gate, fold, splitk, total;
};
static WsLayout ws_layout(const orbit_extractor* fe, int B) {
    WsLayout L;
    size_t off = 0;
    for (int i = 0; i < 3; ++i) {
        L.buf[i] = off;
        off += align_up(fe->buf_elems[i] * (size_t)B * sizeof(float), 256);
    }
    L.pooled = off;
    off += align_up(std::max<size_t>(std::max<size_t>(fe->max_partial, fe->max_se_c), 1) * B * sizeof(float), 256);
    L.gate = off;
    off += align_up((size_t)std::max(fe->max_se_c, 1) * B * sizeof(float), 256);
    L.fold = off;
    off += align_up(2 * fe->fold_floats * sizeof(float), 256);
    L.splitk = off;  // partial tiles of the largest split-K conv at this batch size
    size_t skf = 0;
    for (const Op& o : fe->ops)
        if (o.kind == OP_CONV) skf = std::max(skf, conv_splitk_floats(o.conv_desc(B)));
    off += align_up(skf * sizeof(float), 256);
    L.total = off;
    return L;
}

extern "C" {

int orbit_extractor_create(const char* name, int H, int W, orbit_extractor_t** out) {
    return orbit_extractor_create_ex(name, H, W, 0, out);
}

int orbit_extractor_create_ex(const char* name, int H, int W, int flags, orbit_extractor_t** out) {
    ORBIT_REQUIRE(name && out, "extractor_create: null pointer");
    ORBIT_REQUIRE(H >= 8 && W >= 8 && H <= 4096 && W <= 4096, "extractor_create: bad frame size %dx%d", H, W);
    orbit_extractor* fe = new orbit_extractor();
    fe->name = name, fe->pool.owner = name, fe->H = H, fe->W = W;
    // (same ops, same parameter order under either flag; the second implies the first)
    fe->res_post_training = (flags & ORBIT_PLAN_RES_POST_TRAINING) != 0;
    fe->res_post_backward = fe->res_post_training || (flags & ORBIT_PLAN_RES_POST_BACKWARD) != 0;
    int rc;
    if (fe->name == "resnet18") rc = build_resnet18(fe, H, W);
    else if (fe->name == "efficientnet_b0") rc = build_efficientnet_b0(fe, H, W, (flags & ORBIT_PLAN_UNFUSED) != 0);
    else if (fe->name == "efficientnet_v2_s") rc = build_efficientnet_v2_s(fe, H, W);  // (no fused ops: one op list for every flag)
    else if (fe->name == "set_encoder") rc = build_set_encoder(fe, H, W);
    else rc = set_err(ORBIT_ERR_ARG, "Invalid feature_extractor_name: %s", name);
    if (rc != ORBIT_OK) {
        delete fe;
        return rc;
    }
    fe->bn_dev.resize(fe->bns.size());
    for (size_t i = 0; i < fe->bns.size(); ++i) {
        const BNDesc& b = fe->bns[i];
        BNDev& d = fe->bn_dev[i];
        d.gamma = fe->pool.off(b.gamma), d.beta = fe->pool.off(b.beta);
        d.mean = fe->pool.off(b.mean), d.var = fe->pool.off(b.var);
        d.conv_bias = b.conv_bias >= 0 ? fe->pool.off(b.conv_bias) : (size_t)-1;
        d.fold_off = b.fold_off, d.C = b.C, d.film_off = b.film_off, d.eps = b.eps;
    }
    *out = fe;
    return ORBIT_OK;
}

void orbit_extractor_destroy(orbit_extractor_t* fe) {
    if (!fe) return;
    (void)hipFree(fe->d_dgrad);
    (void)hipFree(fe->d_dgrad_jobs);
    fe->graphs.clear();
    fe->train_graphs.clear();
    if (fe->cap_stream) (void)hipStreamDestroy(fe->cap_stream);
    fe->pool.free_device();
    (void)hipFree(fe->d_packed);
    (void)hipFree(fe->d_pack_jobs);
    (void)hipFree(fe->d_fold);
    (void)hipFree(fe->d_bn);
    delete fe;
}

int orbit_extractor_num_params(const orbit_extractor_t* fe) { return fe ? fe->pool.size() : 0; }
const char* orbit_extractor_param_name(const orbit_extractor_t* fe, int i) { return fe ? fe->pool.name(i) : nullptr; }
size_t orbit_extractor_param_numel(const orbit_extractor_t* fe, int i) { return fe ? fe->pool.numel(i) : 0; }

// every upload invalidates what finalize derived from the parameters and the dgrad filters of the training runtime
int orbit_extractor_load(orbit_extractor_t* fe, const char* key, const float* data, size_t numel) {
    ORBIT_REQUIRE(fe && key && data, "extractor_load: null pointer");
    if (int rc = fe->pool.load("extractor_load", key, data, numel)) return rc;
    fe->finalized = false, fe->dgrad_packed = false;
    return ORBIT_OK;
}

int orbit_extractor_load_async(orbit_extractor_t* fe, const char* key, const float* device_data, size_t numel,
                               orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && key && device_data, "extractor_load_async: null pointer");
    if (int rc = fe->pool.load_async("extractor_load_async", key, device_data, numel, (hipStream_t)stream)) return rc;
    fe->finalized = false, fe->dgrad_packed = false;
    return ORBIT_OK;
}

int orbit_extractor_load_all_async(orbit_extractor_t* fe, const float* const* device_ptrs, int n, orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && device_ptrs, "extractor_load_all_async: null pointer");
    if (int rc = fe->pool.load_all_async("extractor_load_all_async", device_ptrs, n, 32, (hipStream_t)stream)) return rc;
    fe->finalized = false, fe->dgrad_packed = false;
    return ORBIT_OK;
}

int orbit_extractor_finalize(orbit_extractor_t* fe, orbit_stream_t stream) {
    ORBIT_REQUIRE(fe, "extractor_finalize: null pointer");
    const char* missing = nullptr;
    ORBIT_REQUIRE(fe->pool.all_loaded(&missing), "extractor_finalize: parameter '%s' was never loaded", missing);
    if (int rc = fe->ensure_device()) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (fe->pack_jobs_bk != get_option("conv_bk")) {  // (tuning sweeps change the K-tile width, i.e. the packed geometry)
        fe->pack_jobs.clear();
        (void)hipFree(fe->d_pack_jobs);
        fe->d_pack_jobs = nullptr;
        fe->pack_jobs_bk = get_option("conv_bk");
    }
    if (fe->pack_jobs.empty()) {
        auto job = [&](int kind, const float* src, float* dst, int Cin, int Cout, int KH, int KW, int cin_pad, int KT,
                       int cout_pad, size_t total) {
            PackJob j;
            j.src = src, j.dst = dst, j.kind = kind, j.Cin = Cin, j.Cout = Cout, j.KH = KH, j.KW = KW;
            j.cin_pad = cin_pad, j.KT = KT, j.cout_pad = cout_pad, j.total = (unsigned)total;
            fe->pack_jobs.push_back(j);
        };
        for (const Op& o : fe->ops) {
            if (o.kind == OP_CONV) {
                const ConvPackGeom g = conv_pack_geom(o.Cin, o.Cout, o.KH, o.KW, o.x_nchw);
                job(o.x_nchw ? 1 : 0, fe->param(o.weight), fe->d_packed + o.packed_off, o.Cin, o.Cout, o.KH,
                    o.KW, g.cin_pad, g.kt, g.cout_pad, (size_t)g.cout_pad * g.kt);
                if (o.frag_off != SIZE_MAX)
                    job(5, fe->param(o.weight), fe->d_packed + o.frag_off, o.Cin, o.Cout, 1, 1, 0, o.Cin / 16,
                        0, conv_frag_floats(o.Cin, o.Cout, 1, 1, 0));
            } else if (o.kind == OP_DWCONV) {
                job(2, fe->param(o.weight), fe->d_packed + o.packed_off, o.Cin, 0, o.KH, o.KH, 0, 0, 0,
                    (size_t)o.Cin * o.KH * o.KH);
            } else if (o.kind == OP_MBFRONT) {
                job(2, fe->param(o.weight2), fe->d_packed + o.packed_off, o.Cout, 0, o.KH, o.KH, 0, 0, 0,
                    (size_t)o.Cout * o.KH * o.KH);
            } else if (o.kind == OP_SE) {
                job(3, fe->param(o.se_w2), fe->d_packed + o.packed_off, o.Cin, o.R, 0, 0, 0, 0, 0,
                    (size_t)o.Cin * o.R);
            }
        }
    }
    if (int rc = run_pack_jobs(fe->pack_jobs, &fe->d_pack_jobs, s)) return rc;
    for (const Op& o : fe->ops)  // (the fused stem's [mid][32] filter layout has its own kernel; inference plans only)
        if (o.kind == OP_MBFRONT && o.stem)
            if (int rc = stem_pack_weights(fe->param(o.weight), fe->d_packed + o.packed_off2, o.Cout, s))
                return rc;
    dim3 grid((unsigned)fe->bns.size(), 2);
    bn_fold_all_kernel<<<grid, 256, 0, s>>>(fe->d_bn, fe->pool.d_pool, nullptr, nullptr, fe->d_fold,
                                            fe->d_fold + fe->fold_floats);
    ORBIT_LAUNCH_CHECK();
    fe->graphs.clear();
    fe->finalized = true;
    return ORBIT_OK;
}

int orbit_extractor_output_size(const orbit_extractor_t* fe) { return fe ? fe->out_size : 0; }
int orbit_extractor_film_slots(const orbit_extractor_t* fe) { return fe ? (int)fe->film_slots.size() : 0; }
int orbit_extractor_film_slot_channels(const orbit_extractor_t* fe, int slot) {
    return (fe && slot >= 0 && slot < (int)fe->film_slots.size()) ? fe->bns[fe->film_slots[slot]].C : 0;
}
const char* orbit_extractor_film_slot_name(const orbit_extractor_t* fe, int slot) {
    return (fe && slot >= 0 && slot < (int)fe->film_slots.size()) ? fe->bns[fe->film_slots[slot]].name.c_str()
                                                                  : nullptr;
}
int orbit_extractor_film_size(const orbit_extractor_t* fe) { return fe ? fe->film_size : 0; }
double orbit_extractor_macs_per_frame(const orbit_extractor_t* fe) { return fe ? fe->macs : 0.0; }

size_t orbit_extractor_workspace_bytes(const orbit_extractor_t* fe, int B) {
    if (!fe || B <= 0) return 0;
    return ws_layout(fe, B).total;
}

static int run_plan(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma, const float* film_beta,
                    float* feats, void* workspace, hipStream_t s);

int orbit_extractor_forward(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma,
                            const float* film_beta, float* feats, void* workspace, size_t workspace_bytes,
                            orbit_stream_t stream) {
    ORBIT_REQUIRE(fe && frames && feats && workspace, "extractor_forward: null pointer");
    ORBIT_REQUIRE(B > 0, "extractor_forward: empty batch");
    if (!fe->finalized) return set_err(ORBIT_ERR_STATE, "extractor_forward: call orbit_extractor_finalize first");
    ORBIT_REQUIRE((film_gamma == nullptr) == (film_beta == nullptr),
                  "extractor_forward: film_gamma and film_beta must be given together");
    const WsLayout L = ws_layout(fe, B);
    ORBIT_REQUIRE(workspace_bytes >= L.total, "extractor_forward: workspace too small (%zu < %zu bytes)",
                  workspace_bytes, L.total);
    ORBIT_REQUIRE(((uintptr_t)workspace & 255) == 0, "extractor_forward: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    // graph = 0 never, 1 always, 2 (default) adaptive. Measured on MI355X: with a fast host, replaying the graph of a
    // forward is SLOWER than the eager launch sequence (resnet18@84: 5.3 vs 4.5 ms per task), but pool hosts differ 4x
    // in launch cost and on the slow ones the eager sequence (~170 launches per efficientnet task) makes the default
    // workload host-bound. Adaptive: time the host side of the eager sequence; replay graphs only while a launch costs
    // more than ~12 us of host time on average.
    const int graph_opt = get_option("graph");
    bool want_graph = graph_opt == 1;
    if (graph_opt == 2 && fe->eager_samples >= 3 && fe->eager_us_per_launch > 12.0) want_graph = true;
    if (!want_graph || conv_prof_enabled()) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = run_plan(fe, frames, B, film_gamma, film_beta, feats, workspace, s);
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() /
                          (double)(fe->ops.size() + 1);
        fe->eager_us_per_launch = fe->eager_samples == 0 ? us : 0.7 * fe->eager_us_per_launch + 0.3 * us;
        fe->eager_samples++;
        return rc;
    }

    // graph path: 1st sight of a pointer tuple runs eagerly, the 2nd captures + instantiates, later ones replay
    orbit_extractor::GraphKey key;
    memset(&key, 0, sizeof(key));
    key.frames = frames, key.gamma = film_gamma, key.beta = film_beta, key.feats = feats, key.ws = workspace, key.B = B;
    bool replayed = false;
    return fe->graphs.run(
        key, s, &fe->cap_stream,
        [&](hipStream_t rs) { return run_plan(fe, frames, B, film_gamma, film_beta, feats, workspace, rs); }, &replayed);
}

// the squeeze-excite op at index i is computed by its consumer, the gated projection right after it (csrc/pw_stream.hip):
// a function of the layer (and of option conv_rgemm, != 0: the register-GEMM family), never of the batch
static bool se_in_projection(const orbit_extractor_t* fe, size_t i) {
    if (!get_option("conv_rgemm") || i + 1 >= fe->ops.size() || fe->ops[i].kind != OP_SE) return false;
    const Op& c = fe->ops[i + 1];
    return c.kind == OP_CONV && c.use_gate && c.Cin == fe->ops[i].Cin && c.KH == 1 && c.KW == 1 && c.stride == 1 &&
           c.pad_t == 0 && c.pad_l == 0 && !c.x_nchw && !c.pool2 && c.act == ORBIT_ACT_NONE && c.bn >= 0 &&
           c.Ho == c.H && c.Wo == c.W && pw_stream_supported(c.Cin, c.Cout, c.H, c.W);
}

// What serves op `oi` of the inference plan where the op kind leaves a choice (OP_CONV, OP_SE); `prev` is the answer for op
// oi - 1, so a squeeze-excite block asks se_in_projection once
enum ServedBy {
    BY_OWN_LAUNCHER,  // launch_conv / launch_se_gate2, and every other op kind
    BY_STEM_DIRECT,   // EfficientNet stem: LDS-staged input rows + VALU (csrc/stem.hip) instead of the element-wise gather
    BY_PW_STREAM,     // gated projection that computes the gate of the OP_SE before it in its prologue (csrc/pw_stream.hip)
    BY_PROJECTION     // OP_SE skipped: the projection after it is BY_PW_STREAM
};
static ServedBy served_by(const orbit_extractor_t* fe, size_t oi, ServedBy prev) {
    const Op& o = fe->ops[oi];
    if (o.kind == OP_SE) return se_in_projection(fe, oi) ? BY_PROJECTION : BY_OWN_LAUNCHER;
    if (o.kind != OP_CONV) return BY_OWN_LAUNCHER;
    if (o.x_nchw && !o.pool2 && o.res < 0 && o.bn >= 0 && stem_direct_supported(o.Cin, o.Cout, o.KH, o.stride, o.W, o.act) &&
        o.KH == o.KW)
        return BY_STEM_DIRECT;
    return prev == BY_PROJECTION ? BY_PW_STREAM : BY_OWN_LAUNCHER;
}

static int run_plan(orbit_extractor_t* fe, const float* frames, int B, const float* film_gamma, const float* film_beta,
                    float* feats, void* workspace, hipStream_t s) {
    const WsLayout L = ws_layout(fe, B);
    char* ws = static_cast<char*>(workspace);
    auto buf = [&](int id) -> float* {
        if (id == -1) return const_cast<float*>(frames);
        if (id == BUF_FEATS) return feats;
        if (id == BUF_POOLED) return reinterpret_cast<float*>(ws + L.pooled);
        if (id == BUF_GATE) return reinterpret_cast<float*>(ws + L.gate);
        return reinterpret_cast<float*>(ws + L.buf[id]);
    };
    const float* scale = fe->d_fold;
    const float* shift = fe->d_fold + fe->fold_floats;
    if (film_gamma && fe->film_size > 0) {
        float* fs = reinterpret_cast<float*>(ws + L.fold);
        dim3 grid((unsigned)fe->bns.size(), 2);
        const int rec = prof_start("bn_fold_film", 0.0, 4.0 * 6.0 * fe->fold_floats, s);
        bn_fold_all_kernel<<<grid, 256, 0, s>>>(fe->d_bn, fe->pool.d_pool, film_gamma, film_beta, fs, fs + fe->fold_floats);
        prof_stop(rec, s);
        ORBIT_LAUNCH_CHECK();
        scale = fs, shift = fs + fe->fold_floats;
    }
    ServedBy by = BY_OWN_LAUNCHER;
    for (size_t oi = 0; oi < fe->ops.size(); ++oi) {
        const Op& o = fe->ops[oi];
        by = served_by(fe, oi, by);
        int rc = ORBIT_OK;
        switch (o.kind) {
            case OP_CONV: {
                if (by == BY_STEM_DIRECT) {
                    rc = launch_stem_direct(buf(o.in), fe->param(o.weight), scale + fe->bns[o.bn].fold_off,
                                            shift + fe->bns[o.bn].fold_off, buf(o.out), B, o.H, o.W, o.pad_t, o.pad_l, o.Ho,
                                            o.Wo, s);
                    break;
                }
                if (by == BY_PW_STREAM) {
                    const Op& se = fe->ops[oi - 1];
                    PwStreamDesc d;
                    d.x = buf(o.in), d.w_packed = fe->d_packed + o.packed_off, d.y = buf(o.out);
                    d.scale = scale + fe->bns[o.bn].fold_off, d.shift = shift + fe->bns[o.bn].fold_off;
                    d.residual = o.res >= 0 ? buf(o.res) : nullptr;
                    d.partial = buf(BUF_POOLED), d.chunks = se.se_chunks, d.se_hw = se.se_hw;
                    d.w1 = fe->param(se.se_w1), d.b1 = fe->param(se.se_b1);
                    d.w2t = fe->d_packed + se.packed_off, d.b2 = fe->param(se.se_b2), d.R = se.R;
                    d.B = B, d.H = o.H, d.W = o.W, d.Cin = o.Cin, d.Cout = o.Cout;
                    rc = launch_pw_stream(d, s);
                    break;
                }
                ConvDesc d = o.conv_desc(B);
                d.x = buf(o.in), d.w_packed = fe->d_packed + o.packed_off, d.y = buf(o.out);
                d.w_frag = o.frag_off != SIZE_MAX ? fe->d_packed + o.frag_off : nullptr;
                d.scale = o.bn >= 0 ? scale + fe->bns[o.bn].fold_off : nullptr;
                d.shift = o.bn >= 0 ? shift + fe->bns[o.bn].fold_off : nullptr;
                d.residual = o.res >= 0 ? buf(o.res) : nullptr;
                d.gate = o.use_gate ? buf(BUF_GATE) : nullptr;
                d.splitk_ws = reinterpret_cast<float*>(ws + L.splitk);
                d.lean_epilogue = true;  // inference: one activated output per launch
                rc = launch_conv(d, s);
                break;
            }
            case OP_DWCONV:
                rc = launch_dwconv_se(buf(o.in), fe->d_packed + o.packed_off, buf(o.out),
                                      scale + fe->bns[o.bn].fold_off, shift + fe->bns[o.bn].fold_off,
                                      o.pool_partial ? buf(BUF_POOLED) : nullptr, o.geom(B), o.act, s);
                break;
            case OP_MBFRONT:
                if (o.stem)
                    rc = launch_stem_rows(buf(o.in), fe->d_packed + o.packed_off2, scale + fe->bns[o.bn].fold_off,
                                          shift + fe->bns[o.bn].fold_off, fe->d_packed + o.packed_off,
                                          scale + fe->bns[o.bn2].fold_off, shift + fe->bns[o.bn2].fold_off, buf(o.out),
                                          buf(BUF_POOLED), B, o.stem_h, o.stem_w, o.stem_pt, o.stem_pl, o.H, o.W, s, o.se_chunks);
                else
                    rc = launch_mbconv_rows(buf(o.in), fe->param(o.weight),
                                            scale + fe->bns[o.bn].fold_off, shift + fe->bns[o.bn].fold_off,
                                            fe->d_packed + o.packed_off, scale + fe->bns[o.bn2].fold_off,
                                            shift + fe->bns[o.bn2].fold_off, buf(o.out), buf(BUF_POOLED), B, o.H, o.W, o.Cin,
                                            o.Cout, o.KH, o.stride, o.pad_t, o.pad_l, o.Ho, o.Wo, s, o.se_chunks);
                break;
            case OP_MAXPOOL:
                rc = launch_maxpool(buf(o.in), buf(o.out), o.geom(B), s);
                break;
            case OP_AVGPOOL:
                rc = launch_avgpool(buf(o.in), buf(o.out), B, o.H * o.W, o.Cin, s);
                break;
            case OP_SE:
                if (by == BY_PROJECTION) break;  // the projection computes the gate in its prologue
                rc = launch_se_gate2(buf(BUF_POOLED), o.se_chunks, o.se_hw, fe->param(o.se_w1),
                                     fe->param(o.se_b1), fe->d_packed + o.packed_off,
                                     fe->param(o.se_b2), buf(BUF_GATE), B, o.Cin, o.R, s);
                break;
        }
        if (rc != ORBIT_OK) return rc;
    }
    return ORBIT_OK;
}

}  // extern "C"
