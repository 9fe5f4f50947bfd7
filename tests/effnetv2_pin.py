"""Independent pin for the efficientnet_v2_s extractor.

The reference builds timm 0.6.12 `tf_efficientnetv2_s_in21k` with num_classes=0 (reference `model/feature_extractors.py:31-48`);
timm is not installed offline. This module restates that network as plain torch modules in timm's module layout - the class
names `ConvBnAct`, `EdgeResidual`, `InvertedResidual`, `SqueezeExcite`, the attribute names and their registration order, hence
the state_dict keys and their order - so that the reference's FiLM tagging rule (`model/film.py:38-56`) can be restated over
it (`film_slot_names`) and the module can stand in as the CPU oracle of the native plan, in float64 or float32.

timm 0.6.12 details this rests on (efficientnet.py, efficientnet_blocks.py, efficientnet_builder.py):
  * arch `cn_r2_k3_s1_e1_c24_skip | er_r4_k3_s2_e4_c48 | er_r4_k3_s2_e4_c64 | ir_r6_k3_s2_e4_c128_se0.25 |
    ir_r9_k3_s1_e6_c160_se0.25 | ir_r15_k3_s2_e6_c256_se0.25`, stem 24, head 1280, the stride on the first repeat of a stage;
  * the `tf_` variants pad every convolution TF-"SAME" (asymmetric for stride 2: the extra row / column goes to the bottom /
    right) and use BatchNorm eps 1e-3; activations are SiLU;
  * `ConvBnAct.forward` is `bn1(conv(x))` (BatchNormAct2d applies the activation) and, with a skip, `+ x` AFTER it;
  * `EdgeResidual`: conv_exp (k3, carries the stride) -> bn1+SiLU -> conv_pwl 1x1 -> bn2 (+ x); mid = in * e;
  * `InvertedResidual`: conv_pw -> bn1+SiLU -> conv_dw k3 -> bn2+SiLU -> se -> conv_pwl -> bn3 (+ x);
  * `SqueezeExcite`: x * sigmoid(conv_expand(silu(conv_reduce(mean_hw(x))))), both 1x1 with bias, reduced width
    round(block input channels * 0.25);
  * a skip exists where stride == 1 and in == out; the feature is the global average of silu(bn2(conv_head(x))).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

EPS = 1e-3
STEM, HEAD = 24, 1280
# (block kind, repeats, stride of the first repeat, expansion, out channels, se ratio)
ARCH = (("cn", 2, 1, 1, 24, 0.0), ("er", 4, 2, 4, 48, 0.0), ("er", 4, 2, 4, 64, 0.0), ("ir", 6, 2, 4, 128, 0.25),
        ("ir", 9, 1, 6, 160, 0.25), ("ir", 15, 2, 6, 256, 0.25))


class Conv2dSame(nn.Conv2d):
    """TF "SAME": output ceil(in / stride); total padding max((out - 1) * stride + k - in, 0), the smaller half first."""

    def __init__(self, cin, cout, k, stride=1, groups=1, bias=False):
        super().__init__(cin, cout, k, stride, 0, 1, groups, bias)

    def forward(self, x):
        k, s = self.kernel_size[0], self.stride[0]
        ph = max((-(-x.shape[2] // s) - 1) * s + k - x.shape[2], 0)
        pw = max((-(-x.shape[3] // s) - 1) * s + k - x.shape[3], 0)
        return F.conv2d(F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]), self.weight, self.bias, self.stride, 0, 1,
                        self.groups)


class SqueezeExcite(nn.Module):
    def __init__(self, chs, rd):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, rd, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd, chs, 1, bias=True)

    def forward(self, x):
        s = x.mean((2, 3), keepdim=True)
        return x * torch.sigmoid(self.conv_expand(F.silu(self.conv_reduce(s))))


class ConvBnAct(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout
        self.conv = Conv2dSame(cin, cout, 3, stride)
        self.bn1 = nn.BatchNorm2d(cout, eps=EPS)

    def forward(self, x):
        y = F.silu(self.bn1(self.conv(x)))
        return y + x if self.has_skip else y


class EdgeResidual(nn.Module):
    def __init__(self, cin, cout, stride, exp):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout
        mid = cin * exp
        self.conv_exp = Conv2dSame(cin, mid, 3, stride)
        self.bn1 = nn.BatchNorm2d(mid, eps=EPS)
        self.conv_pwl = Conv2dSame(mid, cout, 1)
        self.bn2 = nn.BatchNorm2d(cout, eps=EPS)

    def forward(self, x):
        y = self.bn2(self.conv_pwl(F.silu(self.bn1(self.conv_exp(x)))))
        return y + x if self.has_skip else y


class InvertedResidual(nn.Module):
    def __init__(self, cin, cout, stride, exp, se_ratio):
        super().__init__()
        self.has_skip = stride == 1 and cin == cout
        mid = cin * exp
        self.conv_pw = Conv2dSame(cin, mid, 1)
        self.bn1 = nn.BatchNorm2d(mid, eps=EPS)
        self.conv_dw = Conv2dSame(mid, mid, 3, stride, groups=mid)
        self.bn2 = nn.BatchNorm2d(mid, eps=EPS)
        self.se = SqueezeExcite(mid, int(round(cin * se_ratio)))
        self.conv_pwl = Conv2dSame(mid, cout, 1)
        self.bn3 = nn.BatchNorm2d(cout, eps=EPS)

    def forward(self, x):
        y = F.silu(self.bn1(self.conv_pw(x)))
        y = self.se(F.silu(self.bn2(self.conv_dw(y))))
        y = self.bn3(self.conv_pwl(y))
        return y + x if self.has_skip else y


class EfficientNet(nn.Module):
    """tf_efficientnetv2_s_in21k, num_classes=0: frames [B,3,H,W] (or clips [N,T,3,H,W]) -> features [B,1280]."""

    output_size = HEAD

    def __init__(self):
        super().__init__()
        self.conv_stem = Conv2dSame(3, STEM, 3, 2)
        self.bn1 = nn.BatchNorm2d(STEM, eps=EPS)
        stages, cin = [], STEM
        for kind, repeats, stride, exp, cout, se in ARCH:
            blocks = []
            for r in range(repeats):
                s = stride if r == 0 else 1
                if kind == "cn":
                    blocks.append(ConvBnAct(cin, cout, s))
                elif kind == "er":
                    blocks.append(EdgeResidual(cin, cout, s, exp))
                else:
                    blocks.append(InvertedResidual(cin, cout, s, exp, se))
                cin = cout
            stages.append(nn.Sequential(*blocks))
        self.blocks = nn.Sequential(*stages)
        self.conv_head = Conv2dSame(cin, HEAD, 1)
        self.bn2 = nn.BatchNorm2d(HEAD, eps=EPS)

    def film_slot_names(self):
        return film_slot_names(self)

    def forward(self, x):
        if x.dim() == 5:
            x = x.flatten(end_dim=1)
        x = F.silu(self.bn1(self.conv_stem(x)))
        x = self.blocks(x)
        return F.silu(self.bn2(self.conv_head(x))).mean((2, 3))


def film_slot_names(model):
    """The reference rule (model/film.py:38-56) over the class names: bn1 of every EdgeResidual and ConvBnAct, bn2 of every
    InvertedResidual, bn1 and bn2 of the root; in named_modules() order, as get_film_parameter_names lists them."""
    tagged = set()
    for name, m in model.named_modules():
        kind = type(m).__name__
        want = {"EdgeResidual": ["bn1"], "ConvBnAct": ["bn1"], "InvertedResidual": ["bn2"], "EfficientNet": ["bn1", "bn2"]}.get(kind, [])
        for child in want:
            if isinstance(getattr(m, child, None), nn.BatchNorm2d):
                tagged.add((name + "." if name else "") + child)
    return [n for n, _ in model.named_modules() if n in tagged]


def count_macs(model, H, W):
    """Multiply-accumulates of one H x W frame through every nn.Conv2d / nn.Linear of the model, counted by forward hooks."""
    total = [0]

    def hook(m, inp, out):
        if isinstance(m, nn.Conv2d):
            total[0] += out[0].numel() * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
        elif isinstance(m, nn.Linear):
            total[0] += out[0].numel() * m.in_features

    handles = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]
    was = model.training
    model.eval()
    with torch.no_grad():
        model(torch.zeros(1, 3, H, W, dtype=next(model.parameters()).dtype))
    model.train(was)
    for h in handles:
        h.remove()
    return total[0]
