"""CenterNet-R18-DCNv2, the reference's third detector, from the image to the detections.

`CenterNetTRT.forward_trt` (det2trt/models/detector/centernet.py:11-18; configs/centernet/
centernet_resnet18_dcnv2_140e_coco.py:9-36) re-hosted without mmcv / mmdet, every BatchNorm folded into the layer in
front of it:

  image [B, 3, H, W] -> ResNet-18 (mmdet BasicBlock: 3x3 / s + ReLU, 3x3, + identity, ReLU; 1x1 / s downsample;
  blocks (2, 2, 2, 2); 7x7 / 2 stem + max-pool) -> CTResNetNeck(512, (256, 128, 64), (4, 4, 4), use_dcn=True): three
  times DCNv2 pack + ReLU, ConvTranspose2d(c, c, 4, 2, 1) + ReLU -> CenterNetHead(80, 64, 64): three branches of 3x3
  64 -> 64 + ReLU, 1x1 64 -> {80, 2, 2}; the heat map through a sigmoid -> (center_heatmap_preds [B, 80, H/4, W/4],
  wh_preds [B, 2, H/4, W/4], offset_preds [B, 2, H/4, W/4]).

Two data paths through the same weights, chosen like BEVDet's (bevdet.py):
  * fast: fp16 CUDA tensors on the default operator set.  Channels-last on this package's kernels under the rule
    dispatch -- the fused stem, the tiled / LDS-resident 3x3 convolutions, the strided 1x1 as an implicit GEMM, the
    channels-last DCNv2 pack, `conv_transpose2d_nhwc` (csrc/deconv.hip), the head as TWO launches (first convolutions
    stacked to 64 -> 192, final ones block-diagonal 192 -> 88) whose packed output `centernet_decode` reads in place.
    No measurement at run time and no library convolution, so the frame is capturable and bit-reproducible.
  * plain: any dtype, or an operator set without the fast entries: F.conv2d, F.conv_transpose2d, F.max_pool2d and the
    package's `modulated_deformable_conv2d` -- the reference op sequence, and the reference of the model's tests.

The layer list is written from mmdet 2.x's published modules; neither mmdet nor a CenterNet checkpoint is available to
this repository's tests, so parity with the library's own forward is unpinned (as for functions/decode2d.py)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import bevformer as _B
from . import functions as _hip_ops
from .functions import dispatch as _dispatch
from .functions.deconv import deconv_packed_weight
from .functions.multi_scale_deformable_attn import _TensorCache
from .functions.image import centernet_test_geometry
from .graph_runner import Detect2DRunner

# model / test_cfg of configs/centernet/centernet_resnet18_dcnv2_140e_coco.py:9-36
CENTERNET_R18 = dict(blocks=(2, 2, 2, 2), neck_channels=(256, 128, 64), num_classes=80, feat_channel=64,
                     test_cfg=dict(topk=100, local_maximum_kernel=3, max_per_img=100))
HEADS = ("heatmap", "wh", "offset")
_FAST_OPS = ("conv3x3_auto", "conv_nhwc", "conv_transpose2d_nhwc", "modulated_deformable_conv2d_nhwc", "conv_offset_nhwc",
             "stem_conv_pool", "bias_act_nhwc_")


class BasicBlock(nn.Module):
    """mmdet's ResNet BasicBlock (two 3x3 convolutions, the stride on the first; the downsample of a stage's first
    block is a 1x1 convolution at that stride), BN folded."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(cin, cout, 3, stride, 1), nn.Conv2d(cout, cout, 3, 1, 1)
        self.downsample = nn.Conv2d(cin, cout, 1, stride) if stride != 1 or cin != cout else None

    def forward(self, x):
        ds = self.downsample
        idt = x if ds is None else F.conv2d(x, ds.weight, ds.bias, ds.stride)
        out = F.relu(F.conv2d(x, self.conv1.weight, self.conv1.bias, self.conv1.stride, 1))
        return F.relu(F.conv2d(out, self.conv2.weight, self.conv2.bias, 1, 1) + idt)

    def forward_nhwc(self, x, ops):
        idt = x if self.downsample is None else _B._conv1x1_nhwc(ops, x, self.downsample, False)
        return _B._conv_nhwc(ops, _B._conv_nhwc(ops, x, self.conv1, True), self.conv2, True, idt)


class ResNet18(_B.ResNet):
    """ResNet-18 of basic blocks with bevformer.ResNet's stem, stage loop and data paths (`forward`: the library
    statements; `forward_nhwc`: the fused stem and the channels-last kernels)."""

    def __init__(self, blocks=(2, 2, 2, 2), out_indices=(3,)):
        nn.Module.__init__(self)
        self.out_indices = out_indices
        self.stem = nn.Conv2d(3, 64, 7, 2, 3)
        cin, stages = 64, []
        for i, n in enumerate(blocks):
            planes = 64 * 2 ** i
            stages.append(nn.Sequential(*[BasicBlock(cin if j == 0 else planes, planes, 2 if i > 0 and j == 0 else 1)
                                          for j in range(n)]))
            cin = planes
        self.stages = nn.ModuleList(stages)


class CTResNetNeck(nn.Module):
    """mmdet's CTResNetNeck with use_dcn=True: per level a DCNv2 pack (3x3, deform_groups 1) + BN + ReLU and a
    ConvTranspose2d(c, c, 4, stride 2, padding 1) + BN + ReLU; each BN folded (the layers' biases carry its shift)."""

    def __init__(self, cin, channels, ops):
        super().__init__()
        self.dcn = nn.ModuleList()
        self.deconv = nn.ModuleList()
        for c in channels:
            self.dcn.append(_B.DCNv2Pack(cin, c, ops))
            self.deconv.append(nn.ConvTranspose2d(c, c, 4, 2, 1))
            cin = c

    def forward(self, x):
        for dcn, up in zip(self.dcn, self.deconv):
            x = F.relu(dcn(x))
            x = F.relu(F.conv_transpose2d(x, up.weight, up.bias, 2, 1))
        return x

    def forward_nhwc(self, x, ops):
        for dcn, up in zip(self.dcn, self.deconv):
            x = dcn.forward_nhwc(x, True)
            x = ops.conv_transpose2d_nhwc(x, up.weight, up.bias, relu=True)
        return x


HEAD_PACK_MULTIPLE = 8   # the packed head output is padded to a multiple of 8 channels (whole 16-byte vectors)


def merge_centernet_heads(first, final):
    """The three two-convolution branches as two convolutions.  first / final: lists of (weight, bias) in branch order,
    weight [mid, Cs, 3, 3] and [c_i, mid, 1, 1].  -> (w1 [3 mid, Cs, 3, 3], b1, w2 [P, 3 mid, 1, 1], b2, slices) with
    P = sum(c_i) rounded up to a multiple of 8: w1 / b1 are the first convolutions stacked along the output channels; w2
    is block-diagonal -- branch i's final weights on input channels mid i .. mid i + mid - 1, its c_i output channels
    at slices[i] = (start, stop), zero rows behind channel sum(c_i).  A zero weight adds an exact zero to the fp32
    accumulator, so every branch's output is what its own two convolutions give."""
    mid = first[0][0].shape[0]
    n_out = sum(w.shape[0] for w, _ in final)
    padded = (n_out + HEAD_PACK_MULTIPLE - 1) // HEAD_PACK_MULTIPLE * HEAD_PACK_MULTIPLE
    w0 = first[0][0].detach()
    w1 = w0.new_zeros((len(first) * mid,) + tuple(w0.shape[1:]))
    b1 = w0.new_zeros((len(first) * mid,))
    w2 = w0.new_zeros((padded, len(first) * mid, 1, 1))
    b2 = w0.new_zeros((padded,))
    slices, at = [], 0
    for i, ((wa, ba), (wb, bb)) in enumerate(zip(first, final)):
        if wa.shape[0] != mid or tuple(wb.shape[1:]) != (mid, 1, 1):
            raise ValueError("merge_centernet_heads: every branch is 3x3 to `mid` channels, then 1x1 from them")
        w1[i * mid:(i + 1) * mid].copy_(wa.detach())
        if ba is not None:
            b1[i * mid:(i + 1) * mid].copy_(ba.detach())
        c = wb.shape[0]
        w2[at:at + c, i * mid:(i + 1) * mid].copy_(wb.detach())
        if bb is not None:
            b2[at:at + c].copy_(bb.detach())
        slices.append((at, at + c))
        at += c
    return w1, b1, w2, b2, slices


class CenterNet(nn.Module):
    """forward(image [B, 3, H, W]) -> (center_heatmap_preds [B, 80, H/4, W/4] after the sigmoid, wh_preds [B, 2, H/4,
    W/4], offset_preds [B, 2, H/4, W/4]) -- CenterNetTRT.forward_trt.  H and W are multiples of 32."""

    def __init__(self, cfg=None, ops=None, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        cfg = cfg or CENTERNET_R18
        self.cfg = cfg
        self.ops = ops = ops if ops is not None else _hip_ops
        self.backbone = ResNet18(cfg["blocks"])
        self.neck = CTResNetNeck(512, cfg["neck_channels"], ops)
        cin, mid = cfg["neck_channels"][-1], cfg["feat_channel"]
        widths = dict(heatmap=cfg["num_classes"], wh=2, offset=2)
        self.heads = nn.ModuleDict({k: nn.ModuleList([nn.Conv2d(cin, mid, 3, 1, 1), nn.Conv2d(mid, widths[k], 1)])
                                    for k in HEADS})
        self._init_weights()
        self.eval()

    def _init_weights(self):
        """A synthetic model whose activations keep their scale from the image to the head (timing and tests; a
        checkpoint overwrites every value): He-normal convolutions (a transposed 4x4 / 2 convolution sums 4 taps per
        output; a block's second convolution at half that, so that the identity sums do not double the variance per
        block; a DCN pack at twice that, its untrained mask being sigmoid(0) = 1 / 2), zero shifts, mmdet's
        bias_init_with_prob(0.1) on the heat map."""
        for m in self.modules():
            if isinstance(m, nn.ConvTranspose2d):
                nn.init.normal_(m.weight, std=(2.0 / (4 * m.in_channels)) ** 0.5)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Conv2d) and m.out_channels != 27:      # (the DCN packs initialise their own layers)
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                nn.init.zeros_(m.bias)
        for m in self.modules():
            if isinstance(m, BasicBlock):
                m.conv2.weight.data.mul_(0.5)
            elif isinstance(m, _B.DCNv2Pack):
                nn.init.normal_(m.weight, std=2.0 * (2.0 / (9 * m.weight.shape[1])) ** 0.5)
        for k in HEADS:
            nn.init.normal_(self.heads[k][1].weight, std=self.heads[k][1].in_channels ** -0.5)
        nn.init.constant_(self.heads["heatmap"][1].bias, -2.19)

    # ---- the fast path's cached operands
    def _fast_on(self, x):
        """The fast path takes fp16 CUDA tensors on an operator set that has every entry it calls and plain layers (an
        INT8 build's quantised layers keep the plain statements)."""
        return x.is_cuda and x.dtype == torch.float16 and all(hasattr(self.ops, f) for f in _FAST_OPS) \
            and next(self.parameters()).dtype == torch.float16 \
            and all(type(c) is nn.Conv2d for h in self.heads.values() for c in h)

    def _head_sources(self):
        return [t for k in HEADS for c in self.heads[k] for t in (c.weight, c.bias) if t is not None]

    def heads_merged(self, build=True):
        """(w1, b1, w2, b2, slices) of `merge_centernet_heads` on the device of the head's weights; cached and rebuilt
        when a source weight or bias changes.  build=False: None when missing or stale."""
        stamp = tuple(_TensorCache._stamp(t) for t in self._head_sources())
        hit = self.__dict__.get("_heads_merged")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if not build:
            return None
        hs = [self.heads[k] for k in HEADS]
        merged = merge_centernet_heads([(h[0].weight, h[0].bias) for h in hs], [(h[1].weight, h[1].bias) for h in hs])
        self.__dict__["_heads_merged"] = (stamp, merged)
        return merged

    def _operands_ready(self):
        return self.heads_merged(build=False) is not None and \
            all(deconv_packed_weight(up.weight, build=False) is not None for up in self.neck.deconv)

    def prepare(self):
        """Build (or refresh) the fast path's derived operands on the device the weights live on: the merged head and
        the parity-major packed deconvolution weights.  Allocates and copies, so it must run OUTSIDE stream capture;
        `forward` calls it itself when an operand is missing or a source weight changed, and raises RuntimeError when
        that happens on a capturing stream."""
        p = next(self.parameters())
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("CenterNet.prepare() allocates: call it before the capture begins")
        self.heads_merged()
        for up in self.neck.deconv:
            deconv_packed_weight(up.weight)
        return self

    def _head_fast(self, feat):
        """The head as two launches of the tiled implicit GEMM.  -> three channel slices of the packed [B, H, W, 88]
        result (no copy), the heat map's sigmoid applied in place on its slice."""
        ops = self.ops
        w1, b1, w2, b2, slices = self.heads_merged(build=False)
        packed = ops.conv_nhwc(ops.conv_nhwc(feat, w1, b1, True), w2, b2, False)
        heat, wh, off = (packed[:, a:b] for a, b in slices)
        heat.sigmoid_()
        return heat, wh, off

    @torch.no_grad()
    def forward(self, image):
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] % 32 or image.shape[3] % 32:
            raise ValueError(f"CenterNet: image [B, 3, H, W] with H and W multiples of 32, got {tuple(image.shape)}")
        if self._fast_on(image):
            if not self._operands_ready():      # (first: under capture a missing operand raises before anything is launched)
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("CenterNet: a merged or packed operand is missing or stale and the stream is "
                                       "capturing; call prepare() (or the model once, eagerly) before the capture")
                self.prepare()
            with _dispatch.using(rule=True):
                x = self.backbone.forward_nhwc(image.contiguous(), self.ops)[0]
                return self._head_fast(self.neck.forward_nhwc(x, self.ops))
        x = self.neck(self.backbone(image)[0])
        outs = []
        for k in HEADS:
            a, b = self.heads[k]
            outs.append(F.conv2d(F.relu(F.conv2d(x, a.weight, a.bias, 1, 1)), b.weight, b.bias))
        return torch.sigmoid(outs[0]), outs[1], outs[2]

    def get_bboxes(self, outputs, img_metas, rescale=True):
        """CenterNetHead.get_bboxes on `forward`'s outputs with the reference's test_cfg (topk 100, local maximum kernel
        3): [(det_bboxes [n, 5], det_labels [n] int64)] per image (postprocess.centernet_get_bboxes)."""
        from .postprocess import centernet_get_bboxes
        cfg = self.cfg["test_cfg"]
        return centernet_get_bboxes(*outputs, img_metas, rescale=rescale, topk=cfg["topk"],
                                    local_maximum_kernel=cfg["local_maximum_kernel"])


class CenterNetRunner(Detect2DRunner):
    """`forward` + `centernet_decode(padded=True)` captured once for images of one shape: `step(image)` copies the image
    into the static input buffer (unless it IS that buffer), replays the graph and returns the fixed-size (boxes
    [B, topk, 4], scores [B, topk], labels [B, topk] int32, count [B] int32) with no host synchronisation; the boxes are
    in the network input's pixels (no border, no rescale).  The BEVDetRunner of this detector.

    raw_size=(H0, W0) adds `step_raw`: the frame from RAW uint8 BGR camera images of that size.  The config's test
    pipeline (functions.image.centernet_test_geometry: keep-ratio resize to `img_scale`, the CENTRED paste of
    RandomCenterCropPad's test mode, zero padding to a square, normalisation last) is the FIRST launch of a second graph
    (functions.image_letterbox), reading the static uint8 `raw_buffer` and writing `image_buffer`; `height` and `width`
    must be that pipeline's padded size.  Its boxes are in the RAW image's pixels: the geometry's border and
    scale_factor go to centernet_decode."""

    _detector, _heads, _pipeline = "CenterNet", 3, "centernet"   # (heat, wh, off, then the four of the decode)
    _geometry = staticmethod(centernet_test_geometry)

    def _forward(self, raw=False):
        from .functions.decode2d import centernet_decode
        cfg = self.model.cfg["test_cfg"]
        border = scale = None
        if raw:
            from .functions.image import image_letterbox
            image_letterbox(self.raw_buffer, self.geometry, self.pipeline, out=self.image_buffer)
            b = self.geometry["border"]
            border, scale = (float(b[2]), float(b[0])), self.geometry["scale_factor"]     # mmdet: border[2], border[0]
        heat, wh, off = self.model(self.image_buffer)
        return (heat, wh, off) + tuple(centernet_decode(heat, wh, off, cfg["topk"], self.image_buffer.shape[2:],
                                                        cfg["local_maximum_kernel"], border, scale, padded=True))
