"""YOLOX, the reference's fourth detector, from the image to the detections.

`YOLOXTRT.forward_trt` (det2trt/models/detector/yolox.py; configs/yolox/yolox_x_8x8_300e_coco.py) re-hosted without
mmcv / mmdet, every BatchNorm (eps 1e-3) folded into the convolution in front of it:

  image [B, 3, H, W] -> CSPDarknet P5 (det2trt/models/backbones/csp_darknet.py:61-67: Focus stem; four stages of a
  3x3 / 2 convolution, an SPPBottleneck in the last one, and a CSPLayer of max(round(n deepen), 1) DarknetBottlenecks,
  det2trt/models/utils/scp_layer.py) -> YOLOXPAFPN (reduce layers, nearest up-sampling, top-down CSP layers, 3x3 / 2
  down-samples, bottom-up CSP layers, out convolutions; add_identity False) -> YOLOXHead (per level two towers of two
  3x3 convolutions, then conv_cls / conv_reg / conv_obj: plain 1x1 with bias, det2trt/models/dense_heads/yolox_head.py)
  -> (cls_score_1..3, bbox_pred_1..3, objectness_1..3), all logits.

Every ConvModule is convolution + BN + Swish (x * sigmoid(x)); DarknetBottleneck adds its input AFTER the activation.

Two data paths through the same weights, chosen like CenterNet's (centernet.py):
  * fast: fp16 CUDA tensors on the default operator set.  Channels-last on functions/yolox_ops.py only -- NO
    concatenation and no library call.  Every concatenated tensor is allocated once per forward as one channels-last
    buffer; its producers write their channel slices through `out=` and its consumers read slices through the input
    pitch: a CSP layer's short_conv and its last bottleneck write the two halves; SPP's conv1 writes slice 0 and the
    pool kernel slices 1-3 of one buffer; in the PAFPN the up-sampler or the down-sample convolution writes one half
    and the layer that produced the other operand writes the other half.  The head per level: the towers' first
    convolutions stacked to one launch, their second convolutions on the two halves, the three predictors as one
    block-diagonal 1x1 whose packed [B, H, W, 88] output holds the level's three outputs as channel slices.
    Layers whose width is no multiple of 32 (YOLOX-x: the 80-channel stem output and stage-1 bottlenecks) run at the
    next multiple with zero weight rows / columns (yolox_ops.pad_channels); pad channels stay exact zeros.
  * plain: any dtype, or an operator set without the fast entries: F.conv2d, x * sigmoid(x), F.max_pool2d,
    F.interpolate(mode="nearest"), torch.cat -- the reference op sequence, and the reference of the model's tests.

CSPLayer, DarknetBottleneck, the CSPDarknet stage list and the head's predictors are written from the reference's
files; Focus, SPPBottleneck, YOLOXPAFPN and YOLOXHead.forward_single from mmdet 2.x's published modules.  Neither mmdet
nor a YOLOX checkpoint is available to this repository's tests, so parity with the library's own forward is unpinned
(as for centernet.py and functions/decode2d.py)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functions as _hip_ops
from .functions import yolox_ops as _Y
from .functions.multi_scale_deformable_attn import _TensorCache
from .functions.image import yolox_test_geometry
from .graph_runner import Detect2DRunner

# configs/yolox/yolox_x_8x8_300e_coco.py (deepen 1.33, widen 1.25); YOLOX_S: yolox_s_8x8_300e_coco.py (0.33 / 0.5), a
# narrow architecture without padded layers (Cin 32 / 64, the 64-column tiles)
YOLOX_X = dict(deepen=1.33, widen=1.25, in_channels=(320, 640, 1280), out_channels=320, num_csp_blocks=4, num_classes=80,
               feat_channels=320, strides=(8, 16, 32), test_cfg=dict(score_thr=0.01, nms=dict(iou_threshold=0.65)))
YOLOX_S = dict(deepen=0.33, widen=0.5, in_channels=(128, 256, 512), out_channels=128, num_csp_blocks=1, num_classes=80,
               feat_channels=128, strides=(8, 16, 32), test_cfg=dict(score_thr=0.01, nms=dict(iou_threshold=0.65)))
# in_channels, out_channels, num_blocks, add_identity, use_spp (csp_darknet.py:61-67, "P5")
ARCH_P5 = ((64, 128, 3, True, False), (128, 256, 9, True, False), (256, 512, 9, True, False), (512, 1024, 3, False, True))
SPP_KERNELS = (5, 9, 13)
BN_EPS = 1e-3
HEAD_PACK_MULTIPLE = 8
NMS_MAX_ROWS = 16384
INIT_PREACT_STD = 16.0  # _init_weights: the standard deviation of a SiLU layer's pre-activations for the fixed image
_FAST_OPS = ("conv_slice_taps", "focus_nhwc", "spp_maxpool_nhwc", "upsample_nearest2x_nhwc")


def csp_blocks(n, deepen):
    return max(round(n * deepen), 1)


def silu(x):
    return x * torch.sigmoid(x)


class ConvAct(nn.Conv2d):
    """mmcv's ConvModule(conv, BN, Swish) with the BN folded: convolution (pad k // 2) + bias + activation.
    groups_in: the sizes of the tensors the input is a concatenation of (the fast path pads each to a multiple of 32)."""

    def __init__(self, cin, cout, k, stride=1, act="silu", groups_in=None):
        super().__init__(cin, cout, k, stride, k // 2)
        self.act = act
        self.groups_in = (cin,) if groups_in is None else tuple(groups_in)
        assert sum(self.groups_in) == cin

    def forward(self, x):
        y = F.conv2d(x, self.weight, self.bias, self.stride, self.padding)
        return silu(y) if self.act == "silu" else y


class DarknetBottleneck(nn.Module):
    """scp_layer.py:9-79 with expansion 1 (as CSPLayer builds it): 1x1, 3x3, + input behind the activation."""

    def __init__(self, c, add_identity):
        super().__init__()
        self.conv1, self.conv2 = ConvAct(c, c, 1), ConvAct(c, c, 3)
        self.add_identity = add_identity

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return out + x if self.add_identity else out


class CSPLayer(nn.Module):
    """scp_layer.py:82-166: final_conv(cat(blocks(main_conv(x)), short_conv(x)))."""

    def __init__(self, cin, cout, num_blocks, add_identity, groups_in=None):
        super().__init__()
        mid = int(cout * 0.5)
        self.mid = mid
        self.main_conv, self.short_conv = ConvAct(cin, mid, 1, groups_in=groups_in), ConvAct(cin, mid, 1, groups_in=groups_in)
        self.final_conv = ConvAct(2 * mid, cout, 1, groups_in=(mid, mid))
        self.blocks = nn.ModuleList([DarknetBottleneck(mid, add_identity) for _ in range(num_blocks)])

    def forward(self, x):
        short = self.short_conv(x)
        main = self.main_conv(x)
        for blk in self.blocks:
            main = blk(main)
        return self.final_conv(torch.cat((main, short), dim=1))

    def forward_fast(self, x, run, out=None):
        """x: a channel slice; -> the layer's output, written to `out` when given.  One buffer holds the concatenation:
        the last bottleneck's second convolution writes its first half, short_conv the second."""
        pm = _Y.padded_width(self.mid)
        B, _, H, W = x.shape
        cat = _Y.nhwc_empty(B, 2 * pm, H, W, x.device)
        run(self.short_conv, x, out=cat[:, pm:])
        main = run(self.main_conv, x)
        for j, blk in enumerate(self.blocks):
            hidden = run(blk.conv1, main)
            main = run(blk.conv2, hidden, residual=main if blk.add_identity else None,
                       out=cat[:, :pm] if j == len(self.blocks) - 1 else None)
        return run(self.final_conv, cat, out=out)


class Focus(nn.Module):
    """mmdet's Focus: the four pixel-parity patches (top-left, bottom-left, top-right, bottom-right) concatenated on
    the channels, then a 3x3 ConvModule."""

    def __init__(self, cout):
        super().__init__()
        self.conv = ConvAct(12, cout, 3)

    def forward(self, x):
        tl, tr = x[..., ::2, ::2], x[..., ::2, 1::2]
        bl, br = x[..., 1::2, ::2], x[..., 1::2, 1::2]
        return self.conv(torch.cat((tl, bl, tr, br), dim=1))

    def forward_fast(self, image, run, ops):
        return run(self.conv, ops.focus_nhwc(image))


class SPPBottleneck(nn.Module):
    """mmdet's SPPBottleneck: conv1 (1x1 to half the channels), cat(x, max-pools 5 / 9 / 13), conv2 (1x1)."""

    def __init__(self, cin, cout, kernel_sizes=SPP_KERNELS):
        super().__init__()
        mid = cin // 2
        self.mid, self.kernel_sizes = mid, tuple(kernel_sizes)
        self.conv1 = ConvAct(cin, mid, 1)
        self.conv2 = ConvAct(mid * (len(kernel_sizes) + 1), cout, 1, groups_in=(mid,) * (len(kernel_sizes) + 1))

    def forward(self, x):
        x = self.conv1(x)
        return self.conv2(torch.cat([x] + [F.max_pool2d(x, k, 1, k // 2) for k in self.kernel_sizes], dim=1))

    def forward_fast(self, x, run, ops):
        pm = _Y.padded_width(self.mid)
        B, _, H, W = x.shape
        cat = _Y.nhwc_empty(B, 4 * pm, H, W, x.device)
        run(self.conv1, x, out=cat[:, :pm])
        ops.spp_maxpool_nhwc(cat[:, :pm], out=cat[:, pm:], kernel_sizes=self.kernel_sizes)
        return run(self.conv2, cat)


class CSPDarknet(nn.Module):
    """csp_darknet.py's CSPDarknetQ, arch P5, out_indices (2, 3, 4): -> the outputs of stages 2, 3, 4."""

    def __init__(self, deepen, widen):
        super().__init__()
        self.stem = Focus(int(ARCH_P5[0][0] * widen))
        self.stages = nn.ModuleList()
        for cin, cout, n, add_identity, use_spp in ARCH_P5:
            cin, cout = int(cin * widen), int(cout * widen)
            stage = [ConvAct(cin, cout, 3, 2)]
            if use_spp:
                stage.append(SPPBottleneck(cout, cout))
            stage.append(CSPLayer(cout, cout, csp_blocks(n, deepen), add_identity))
            self.stages.append(nn.Sequential(*stage))

    def forward(self, x):
        x = self.stem(x)
        outs = []
        for stage in self.stages:
            x = stage(x)
            outs.append(x)
        return tuple(outs[1:])

    def forward_fast(self, image, run, ops, dests=(None, None, None)):
        """dests: where the outputs of stages 2, 3, 4 go (channel slices of the PAFPN's concatenation buffers)."""
        x = self.stem.forward_fast(image, run, ops)
        outs = []
        for i, stage in enumerate(self.stages):
            x = run(stage[0], x)
            if len(stage) == 3:
                x = stage[1].forward_fast(x, run, ops)
            x = stage[-1].forward_fast(x, run, out=dests[i - 1] if i >= 1 else None)
            outs.append(x)
        return tuple(outs[1:])


class YOLOXPAFPN(nn.Module):
    """mmdet's YOLOXPAFPN (add_identity False in its CSP layers)."""

    def __init__(self, in_channels, out_channels, num_csp_blocks):
        super().__init__()
        c = tuple(in_channels)
        self.in_channels = c
        n = len(c)
        self.reduce_layers = nn.ModuleList([ConvAct(c[i], c[i - 1], 1) for i in range(n - 1, 0, -1)])
        self.top_down_blocks = nn.ModuleList([CSPLayer(2 * c[i - 1], c[i - 1], num_csp_blocks, False, (c[i - 1], c[i - 1]))
                                              for i in range(n - 1, 0, -1)])
        self.downsamples = nn.ModuleList([ConvAct(c[i], c[i], 3, 2) for i in range(n - 1)])
        self.bottom_up_blocks = nn.ModuleList([CSPLayer(2 * c[i], c[i + 1], num_csp_blocks, False, (c[i], c[i]))
                                               for i in range(n - 1)])
        self.out_convs = nn.ModuleList([ConvAct(ci, out_channels, 1) for ci in c])

    def forward(self, inputs):
        n = len(self.in_channels)
        inner = [inputs[-1]]
        for idx in range(n - 1, 0, -1):
            high = self.reduce_layers[n - 1 - idx](inner[0])
            inner[0] = high
            up = F.interpolate(high, scale_factor=2, mode="nearest")
            inner.insert(0, self.top_down_blocks[n - 1 - idx](torch.cat([up, inputs[idx - 1]], 1)))
        outs = [inner[0]]
        for idx in range(n - 1):
            down = self.downsamples[idx](outs[-1])
            outs.append(self.bottom_up_blocks[idx](torch.cat([down, inner[idx + 1]], 1)))
        return tuple(conv(o) for conv, o in zip(self.out_convs, outs))

    def buffers(self, B, H8, W8, device):
        """The four concatenation buffers of one forward for a stride-8 map of H8 x W8 pixels (three levels):
        (top-down 0 [up(reduce 0) | c4], top-down 1 [up(reduce 1) | c3], bottom-up 0 [down 0 | reduce 1],
        bottom-up 1 [down 1 | reduce 0])."""
        c = self.in_channels
        h16, w16, h32, w32 = H8 // 2, W8 // 2, H8 // 4, W8 // 4
        return (_Y.nhwc_empty(B, 2 * c[1], h16, w16, device), _Y.nhwc_empty(B, 2 * c[0], H8, W8, device),
                _Y.nhwc_empty(B, 2 * c[0], h16, w16, device), _Y.nhwc_empty(B, 2 * c[1], h32, w32, device))

    def forward_fast(self, c5, bufs, run, ops):
        """c5: the backbone's last output; the other two already sit in the second halves of bufs[0] (c4) and bufs[1]
        (c3), written there by the backbone."""
        c = self.in_channels
        td0, td1, bu0, bu1 = bufs
        high5 = run(self.reduce_layers[0], c5, out=bu1[:, c[1]:])
        ops.upsample_nearest2x_nhwc(high5, out=td0[:, :c[1]])
        inner4 = self.top_down_blocks[0].forward_fast(td0, run)
        high4 = run(self.reduce_layers[1], inner4, out=bu0[:, c[0]:])
        ops.upsample_nearest2x_nhwc(high4, out=td1[:, :c[0]])
        out0 = self.top_down_blocks[1].forward_fast(td1, run)
        run(self.downsamples[0], out0, out=bu0[:, :c[0]])
        out1 = self.bottom_up_blocks[0].forward_fast(bu0, run)
        run(self.downsamples[1], out1, out=bu1[:, :c[1]])
        out2 = self.bottom_up_blocks[1].forward_fast(bu1, run)
        return tuple(run(conv, o) for conv, o in zip(self.out_convs, (out0, out1, out2)))


class YOLOXHead(nn.Module):
    """mmdet's YOLOXHead.forward_single per level: cls_convs / reg_convs (two 3x3 ConvModules each), conv_cls on the
    first tower, conv_reg and conv_obj on the second."""

    def __init__(self, num_classes, cin, feat, levels):
        super().__init__()
        self.num_classes, self.feat = num_classes, feat
        tower = lambda: nn.Sequential(ConvAct(cin, feat, 3), ConvAct(feat, feat, 3))   # noqa: E731
        self.cls_convs = nn.ModuleList([tower() for _ in range(levels)])
        self.reg_convs = nn.ModuleList([tower() for _ in range(levels)])
        self.conv_cls = nn.ModuleList([nn.Conv2d(feat, num_classes, 1) for _ in range(levels)])
        self.conv_reg = nn.ModuleList([nn.Conv2d(feat, 4, 1) for _ in range(levels)])
        self.conv_obj = nn.ModuleList([nn.Conv2d(feat, 1, 1) for _ in range(levels)])

    def forward(self, feats):
        cls, reg, obj = [], [], []
        for l, x in enumerate(feats):
            cf, rf = self.cls_convs[l](x), self.reg_convs[l](x)
            cls.append(self.conv_cls[l](cf))
            reg.append(self.conv_reg[l](rf))
            obj.append(self.conv_obj[l](rf))
        return tuple(cls + reg + obj)


def merge_yolox_predictors(conv_cls, conv_reg, conv_obj):
    """The three 1x1 predictors of one level as ONE block-diagonal 1x1 convolution over the stacked tower features
    [cls_feat | reg_feat] (2 feat channels).  Each argument: (weight [c, feat, 1, 1], bias [c] or None).
    -> (weight [P, 2 feat, 1, 1], bias [P], slices): conv_cls on input channels 0 .. feat - 1, conv_reg and conv_obj on
    feat .. 2 feat - 1; slices[i] = (start, stop) of the outputs of cls / reg / obj; P = their sum rounded up to a
    multiple of 8, zero rows behind it.  A zero weight adds an exact zero to the fp32 sum, so every output is what its
    own predictor gives."""
    feat = conv_cls[0].shape[1]
    n_out = sum(w.shape[0] for w, _ in (conv_cls, conv_reg, conv_obj))
    padded = (n_out + HEAD_PACK_MULTIPLE - 1) // HEAD_PACK_MULTIPLE * HEAD_PACK_MULTIPLE
    w0 = conv_cls[0].detach()
    w, b = w0.new_zeros((padded, 2 * feat, 1, 1)), w0.new_zeros((padded,))
    slices, at = [], 0
    for i, (wi, bi) in enumerate((conv_cls, conv_reg, conv_obj)):
        if tuple(wi.shape[1:]) != (feat, 1, 1):
            raise ValueError("merge_yolox_predictors: every predictor is 1x1 from `feat` channels")
        c, col = wi.shape[0], 0 if i == 0 else feat
        w[at:at + c, col:col + feat].copy_(wi.detach())
        if bi is not None:
            b[at:at + c].copy_(bi.detach())
        slices.append((at, at + c))
        at += c
    return w, b, slices


def _taps(weight):
    return weight.detach().permute(0, 2, 3, 1).contiguous()


class YOLOX(nn.Module):
    """forward(image [B, 3, H, W]) -> (cls_score_1..3 [B, 80, H/s, W/s], bbox_pred_1..3 [B, 4, ..], objectness_1..3
    [B, 1, ..]) for s = 8, 16, 32, all logits -- YOLOXTRT.forward_trt.  H and W are multiples of 32."""

    def __init__(self, cfg=None, ops=None, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        cfg = cfg or YOLOX_X
        self.cfg = cfg
        self.ops = ops if ops is not None else _hip_ops
        if any(c % 32 for c in cfg["in_channels"]) or cfg["out_channels"] % 32 or cfg["feat_channels"] % 32:
            raise ValueError("YOLOX: the PAFPN and head widths are multiples of 32")
        self.backbone = CSPDarknet(cfg["deepen"], cfg["widen"])
        self.neck = YOLOXPAFPN(cfg["in_channels"], cfg["out_channels"], cfg["num_csp_blocks"])
        self.bbox_head = YOLOXHead(cfg["num_classes"], cfg["out_channels"], cfg["feat_channels"], len(cfg["strides"]))
        self._init_weights(seed)
        self.eval()

    def _init_weights(self, seed=0):
        """A synthetic model whose activations keep their scale from the image to the head (timing and tests; a
        checkpoint overwrites every value).  SiLU-aware He scaling: a fixed gain cannot hold the scale through a
        hundred SiLU layers without normalisation -- E[silu(s z)^2] / s^2 rises from 1 / 4 (small s) to 1 / 2 (large
        s), so the scale at which a gain balances is an unstable one, and the logits of YOLOX-x ended at 1e5 or 1e-2
        depending on the image size.  So every convolution starts He-normal (std (2 / fan_in)^0.5) and is then scaled,
        layer by layer in forward order, to a chosen standard deviation of its output for one fixed unit-normal image
        of 96 x 96 pixels: INIT_PREACT_STD = 16 for a SiLU layer (half of it for the second convolution of a bottleneck
        with an identity, so that a chain of identity sums grows slowly) and 1 for the nine predictors.  At 16 a layer
        works where SiLU is nearly homogeneous (one value in eight still lies in |v| < 2.5, where it is not).  That is
        what keeps a perturbation from growing with the depth: where the scale of a layer's input decides its gain, a
        rounding error early in the network changes the gains behind it, and the library's fp16 convolutions put the
        plain fp16 path of YOLOX-x at 1.1 - 2.9 times the model tests' bar with pre-activations of 1.5 - 6; at 16 it is
        at 0.36 - 0.57 of it (the fast path: 0.06 - 0.17), and a map of another size -- other border shares in every
        3 x 3 layer -- changes the logits' scale by a small factor: on random images from 64 x 64 to 96 x 128 every
        logit map keeps a standard deviation above 0.2 and a maximum below 6.  Zero shifts."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=(2.0 / (m.in_channels * m.kernel_size[0] * m.kernel_size[1])) ** 0.5)
                nn.init.zeros_(m.bias)
        half = {id(m.conv2): 0.5 for m in self.modules() if isinstance(m, DarknetBottleneck) and m.add_identity}

        def scale(m, inputs):
            y = F.conv2d(inputs[0], m.weight, None, m.stride, m.padding)
            target = half.get(id(m), 1.0) * (INIT_PREACT_STD if isinstance(m, ConvAct) else 1.0)
            m.weight.data.mul_(target / float(y.std().clamp_min(1e-12)))

        hooks = [m.register_forward_pre_hook(scale) for m in self.modules() if isinstance(m, nn.Conv2d)]
        image = torch.randn((1, 3, 96, 96), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            self.bbox_head(self.neck(self.backbone(image)))
        for h in hooks:
            h.remove()

    # ---- the fast path's cached operands
    def _fast_on(self, x):
        return x.is_cuda and x.dtype == torch.float16 and all(hasattr(self.ops, f) for f in _FAST_OPS) \
            and next(self.parameters()).dtype == torch.float16

    def _build_operands(self):
        """{module or ("first" | "pred", level): (taps-major weight, bias)}: every ConvAct padded per channel group to a
        multiple of 32 (the stem's 12 input channels to Focus' 32), the head's stacked first tower convolutions and
        block-diagonal predictors."""
        ops = {}
        head = self.bbox_head
        for m in self.modules():
            if isinstance(m, ConvAct):
                w, b = _Y.pad_channels(m.weight, m.bias, groups_in=m.groups_in)
                ops[m] = (_taps(w), b.contiguous())
        for l in range(len(head.cls_convs)):
            a, r = head.cls_convs[l][0], head.reg_convs[l][0]
            ops[("first", l)] = (_taps(torch.cat([a.weight.detach(), r.weight.detach()], 0)),
                                 torch.cat([a.bias.detach(), r.bias.detach()], 0).contiguous())
            w, b, slices = merge_yolox_predictors(*((c[l].weight, c[l].bias) for c in (head.conv_cls, head.conv_reg,
                                                                                      head.conv_obj)))
            ops[("pred", l)] = (_taps(w), b)
            ops["slices"] = slices
        return ops

    def operands(self, build=True):
        """The fast path's merged, padded and packed operands on the device of the weights; cached, stamped with every
        parameter's version and rebuilt when one changes.  build=False: None when missing or stale."""
        stamp = tuple(_TensorCache._stamp(p) for p in self.parameters())
        hit = self.__dict__.get("_operands")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if not build:
            return None
        ops = self._build_operands()
        self.__dict__["_operands"] = (stamp, ops)
        return ops

    def prepare(self):
        """Build (or refresh) the fast path's operands.  Allocates and copies, so it must run OUTSIDE stream capture;
        `forward` calls it itself when an operand is missing or a weight changed, and raises RuntimeError when that
        happens on a capturing stream."""
        p = next(self.parameters())
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("YOLOX.prepare() allocates: call it before the capture begins")
        self.operands()
        return self

    def _forward_fast(self, image):
        ops, table = self.ops, self.operands(build=False)

        def run(conv, x, residual=None, out=None):
            w, b = table[conv]
            return ops.conv_slice_taps(x, w, b, conv.act, residual, conv.stride[0], out)

        B, _, H, W = image.shape
        c = self.neck.in_channels
        bufs = self.neck.buffers(B, H // 8, W // 8, image.device)
        dests = (bufs[1][:, c[0]:], bufs[0][:, c[1]:], None)
        c5 = self.backbone.forward_fast(image.contiguous(), run, ops, dests)[2]
        feats = self.neck.forward_fast(c5, bufs, run, ops)
        head, feat = self.bbox_head, self.bbox_head.feat
        cls, reg, obj = [], [], []
        for l, x in enumerate(feats):
            first = ops.conv_slice_taps(x, *table[("first", l)], "silu")
            second = _Y.nhwc_empty(B, 2 * feat, x.shape[2], x.shape[3], x.device)
            run(head.cls_convs[l][1], first[:, :feat], out=second[:, :feat])
            run(head.reg_convs[l][1], first[:, feat:], out=second[:, feat:])
            packed = ops.conv_slice_taps(second, *table[("pred", l)], "none")
            for lst, (a, b) in zip((cls, reg, obj), table["slices"]):
                lst.append(packed[:, a:b])
        return tuple(cls + reg + obj)

    @torch.no_grad()
    def forward(self, image):
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] % 32 or image.shape[3] % 32:
            raise ValueError(f"YOLOX: image [B, 3, H, W] with H and W multiples of 32, got {tuple(image.shape)}")
        if self._fast_on(image):
            if self.operands(build=False) is None:   # (first: under capture a missing operand raises before any launch)
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("YOLOX: a merged or packed operand is missing or stale and the stream is "
                                       "capturing; call prepare() (or the model once, eagerly) before the capture")
                self.prepare()
            return self._forward_fast(image)
        return self.bbox_head(self.neck(self.backbone(image)))

    def get_bboxes(self, outputs, img_metas, rescale=True):
        """YOLOXHead.get_bboxes on `forward`'s nine outputs with the config's test_cfg (score_thr 0.01, NMS IoU 0.65):
        [(det_bboxes [n, 5], det_labels [n] int64)] per image (postprocess.yolox_get_bboxes)."""
        from .postprocess import yolox_get_bboxes
        cfg, n = self.cfg["test_cfg"], len(self.cfg["strides"])
        return yolox_get_bboxes(list(outputs[:n]), list(outputs[n:2 * n]), list(outputs[2 * n:]), img_metas,
                                rescale=rescale, score_thr=cfg["score_thr"], iou_threshold=cfg["nms"]["iou_threshold"],
                                strides=self.cfg["strides"])


def num_priors(height, width, strides=(8, 16, 32)):
    return sum((height // s) * (width // s) for s in strides)


class YOLOXRunner(Detect2DRunner):
    """`forward` + `yolox_decode` + `box_nms(padded=True)` captured once for images of one shape: `step(image)` copies
    the image into the static input buffer (unless it IS that buffer), replays the graph and returns the fixed-size
    (boxes [B, P, 4], scores [B, P], labels [B, P] int32, count [B] int32) with no host synchronisation; the boxes are
    in the network input's pixels (no rescale).  box_nms takes at most 16 384 rows: a size with more priors than that
    raises ValueError here.

    raw_size=(H0, W0) adds `step_raw`: the frame from RAW uint8 BGR camera images of that size.  The config's test
    pipeline (functions.image.yolox_test_geometry: keep-ratio resize to `img_scale`, 114 padding at the bottom / right
    to a square) is the FIRST launch of a second graph (functions.image_letterbox), reading the static uint8
    `raw_buffer` and writing `image_buffer`; `height` and `width` must be that pipeline's padded size.  Its boxes are in
    the RAW image's pixels: the geometry's scale_factor goes to yolox_decode, before the NMS as in mmdet."""

    _detector, _heads, _pipeline = "YOLOX", -4, "yolox"        # (the nine head outputs, then the four of the NMS)
    _geometry = staticmethod(yolox_test_geometry)

    def _check_size(self, model, height, width):
        if num_priors(height, width, model.cfg["strides"]) > NMS_MAX_ROWS:
            raise ValueError(f"YOLOXRunner: {num_priors(height, width, model.cfg['strides'])} priors at {height} x {width}; "
                             f"box_nms takes at most {NMS_MAX_ROWS} rows")

    def _forward(self, raw=False):
        from .functions.decode2d import box_nms, yolox_decode
        cfg, n = self.model.cfg, len(self.model.cfg["strides"])
        if raw:
            from .functions.image import image_letterbox
            image_letterbox(self.raw_buffer, self.geometry, self.pipeline, out=self.image_buffer)
        outs = self.model(self.image_buffer)
        boxes, scores, labels = yolox_decode(list(outs[:n]), list(outs[n:2 * n]), list(outs[2 * n:]), cfg["strides"],
                                             self.geometry["scale_factor"] if raw else None)
        kept = box_nms(boxes, scores, labels, score_threshold=cfg["test_cfg"]["score_thr"],
                       iou_threshold=cfg["test_cfg"]["nms"]["iou_threshold"], class_aware=True, padded=True)
        return tuple(outs) + tuple(kept[:4])
