"""The INT8 build of CenterNet-R18-DCNv2 (centernet.py): what TensorRT builds from the reference's
samples/centernet/onnx2trt_int8.sh (implicit quantisation: every layer it can, the deconvolutions included;
neck="int8") and from configs/centernet/centernet_resnet18_dcnv2_140e_coco_trt_q.py (`ResNetQ` / `Conv2dQ` backbone,
`CenterNetHeadQ`, the neck left in float: its quantised neck line is commented out; neck="fp16").  design/centernet_int8.md.

THE PLAN (`build_plan`) is a list of layers on NAMED tensors (int8_plan.py: Layer, Plan), so that one description serves
the layer and site counts (no tensor needed), the int8 run and the fp32 fake-quant statement of the tests:

  stem       7x7 / 2 + ReLU + 3x3 / 2 max-pool, fp16 arithmetic, int8 out        stem_conv_pool (csrc/stem.hip)
  BasicBlock conv1 3x3 / s + ReLU; downsample 1x1 / s (a stage's first block); conv2 3x3 + identity + ReLU with the
             identity IN FRONT of the ReLU                                        conv_slice_q_taps(res_first=True)
  neck int8  per level: offset convolution int8 -> 32 fp16 channels               conv_int8_chain_nhwc
             DCNv2 + ReLU on int8 channels-last tensors                           modulated_deformable_conv2d_int8_nhwc
             ConvTranspose2d(c, c, 4, 2, 1) + ReLU                                conv_transpose2d_q_nhwc (csrc/deconv_s8.hip)
  neck fp16  the last block leaves as fp16, CTResNetNeck.forward_nhwc unchanged, one quantize_rows pass
  head       64 -> 192 3x3 + ReLU int8 out, 192 -> 88 block-diagonal 1x1 fp16 out (merge_centernet_heads' operands)

ONE SCALE PER TENSOR.  Every int8 tensor has one calibration site ("centernet." + its name) and one scale; its producer
requantises with that scale and every consumer reads with it (there are no concatenations here).  The offsets and the
mask of a DCN pack are two more int8 tensors: the kernel quantises them from the fp16 output of the offset convolution
while it stages them."""
import torch
import torch.nn.functional as F

from . import bevformer as _B
from . import centernet as _cn
from . import functions as _hip_ops
from .functions import dispatch as _dispatch
from .functions import yolox_ops as _Y
from .functions.deconv import deconv_packed_weight, quantize_deconv_weight
from .int8_plan import (Int8Model, Layer, Plan, basic_block_conv, basic_block_layers, conv_call, conv_statement,   # noqa: F401
                        float_operands, load_calibration, save_calibration, scales_from, stored)

SITE_PREFIX = "centernet."
NECK_MODES = ("int8", "fp16")
DCN_INT8_CIN_MULTIPLE = 128     # bevops_mdconv_forward_int8_nhwc: 128-channel k-steps (csrc/mdconv_s8.hip, plan_s8)


# Layer ops: "stem", "conv", "offset", "dcn", "deconv", "neck_fp16", "quantize".  No layer writes `into` a buffer, so every
# tensor is its own scale group and plan.sites is one site per int8 tensor.
INT8_OPS = ("conv", "offset", "dcn", "deconv")


def dcn_int8_domain(model):
    """The packs of `model`'s neck outside the domain of the int8 DCN block (csrc/mdconv_s8.hip, plan_s8: input channels
    a multiple of 128, output channels of 4; a map of fewer pixels than one 64-pixel tile is inside it -- rows past the
    last pixel gather with zero area weights from pixel 0 and store nothing).  -> the list of their indices."""
    return [i for i, d in enumerate(model.neck.dcn)
            if d.weight.shape[1] % DCN_INT8_CIN_MULTIPLE or d.weight.shape[0] % 4]


def build_plan(model, neck="int8"):
    """The layers of `model` (a centernet.CenterNet) in the order of its fast path.  neck: "int8" | "fp16"."""
    if neck not in NECK_MODES:
        raise ValueError(f"neck in {NECK_MODES}")
    P = Plan(SITE_PREFIX, INT8_OPS)
    P.neck = neck
    x = P.add(Layer("stem", "stem", None, "stem"))
    stages = model.backbone.stages
    for i, stage in enumerate(stages):
        for j, blk in enumerate(stage):
            name = f"s{i}.b{j}"
            last = i == len(stages) - 1 and j == len(stage) - 1
            x = basic_block_layers(P, blk, name, x, "f16" if last and neck == "fp16" else "q")
    if neck == "int8":
        for l in range(len(model.neck.dcn)):
            name = f"neck{l}"
            om = P.add(Layer("offset", name + ".offset", x, name + ".om"), "f16")
            x = P.add(Layer("dcn", name + ".dcn", x, name + ".dcn", res=om, act="relu",
                            extra=(name + ".offset", name + ".mask")))
            x = P.add(Layer("deconv", name + ".up", x, name + ".up", act="relu"))
    else:
        f = P.add(Layer("neck_fp16", "neck", x, "neck.f16"), "f16")
        x = P.add(Layer("quantize", None, f, f"neck{len(model.neck.dcn) - 1}.up"))
    h = P.add(Layer("conv", "head.first", x, "head.hidden", act="relu"))
    P.add(Layer("conv", "head.final", h, "head.packed"), "f16")
    return P


def _conv_of(model, key):
    return basic_block_conv(model.backbone.stages[int(key[1])][int(key[4])], key[6:])


def _sources(model, plan):
    """{key: (weight [Cout, Cin, k, k], bias)} of every "conv" and "offset" layer of `plan`.  -> (table, head slices)."""
    w1, b1, w2, b2, slices = model.heads_merged()
    table = {}
    for l in plan.layers:
        if l.op == "offset":
            co = model.neck.dcn[int(l.key[4])].conv_offset
            table[l.key] = (co.weight, co.bias)
        elif l.op == "conv" and l.key.startswith("head."):
            table[l.key] = (w1, b1) if l.key == "head.first" else (w2, b2)
        elif l.op == "conv":
            c = _conv_of(model, l.key)
            table[l.key] = (c.weight, c.bias)
    return table, slices


def quantize_operands(model, plan):
    """{key: operands} for every layer of `plan` from the weights of `model`; "conv": (w_q_taps int8 [Cout, k, k, Cin],
    w_scales fp32, bias fp32) per output channel (functions.yolox_ops.quantize_weight_taps); "offset": the same with the
    27 filters padded to 32 (Int8ChainBackbone's recipe); "dcn": (weight_q int8 [Cout, Cin, 3, 3], ONE scale, bias fp32);
    "deconv": (weight_q int8 [Cin, Cout, 4, 4], w_scales fp32 [Cout], bias fp32); "slices": the head's channel slices."""
    src, slices = _sources(model, plan)
    table = {"slices": slices}
    for l in plan.layers:
        if l.op in ("conv", "offset"):
            if l.op == "offset" and src[l.key][0].shape[0] != 27:
                raise NotImplementedError("Int8CenterNet: DCNv2 packs other than 3x3 / deform_groups=1")
            # (the head's operands in the pack of merge_centernet_heads; the 27 offset filters padded to 32)
            kw = {"multiple": _cn.HEAD_PACK_MULTIPLE} if l.key.startswith("head.") else {"multiple": 32} if l.op == "offset" else {}
            table[l.key] = _Y.quantize_weight_taps(*src[l.key], **kw)
        elif l.op == "dcn":
            d = model.neck.dcn[int(l.key[4])]
            w = d.weight.detach().float()
            s = float(torch.tensor(max(float(w.abs().max()), 1e-12) / 127.0, dtype=torch.float32))
            q = torch.clamp(torch.round(w / s), -127, 127).to(torch.int8).contiguous()
            table[l.key] = (q, s, d.bias.detach().float().contiguous())
        elif l.op == "deconv":
            up = model.neck.deconv[int(l.key[4])]
            table[l.key] = quantize_deconv_weight(up.weight, up.bias)
    return table


def _float_operands(model, plan):
    """The un-quantised fp32 operands in the layouts of `quantize_operands` with unit scales (the statement with the
    quantisation disabled)."""
    src, slices = _sources(model, plan)
    table = dict(float_operands(src), slices=slices)
    for l in plan.layers:
        if l.op == "dcn":
            d = model.neck.dcn[int(l.key[4])]
            table[l.key] = (d.weight.detach().float(), 1.0, d.bias.detach().float())
        elif l.op == "deconv":
            up = model.neck.deconv[int(l.key[4])]
            table[l.key] = (up.weight.detach().float(), torch.ones(up.weight.shape[1], device=up.weight.device),
                            up.bias.detach().float())
    return table


def _neck_float(model, x, mdconv):
    """CTResNetNeck.forward in fp32 statements on the fp32 values of `model`'s weights."""
    for d, up in zip(model.neck.dcn, model.neck.deconv):
        co = d.conv_offset
        o1, o2, mask = torch.chunk(F.conv2d(x, co.weight.float(), co.bias.float(), 1, 1), 3, dim=1)
        x = F.relu(mdconv(x, torch.cat((o1, o2), dim=1), torch.sigmoid(mask), d.weight.float(), d.bias.float(), 1, 1, 1, 1, 1))
        x = F.relu(F.conv_transpose2d(x, up.weight.float(), up.bias.float(), 2, 1))
    return x


def emulate(model, plan, image, table, scales, mdconv=None, tensors=None):
    """The fp32 torch statement of the int8 run: NCHW fp32 tensors holding q * scale, fake quantisation
    (int8_plan.fake_quant: the kernels' clamp(rne(v * (1 / scale)), -127, 127) * scale) at every int8 tensor of the plan;
    the fp16 tensors (the offset convolution's output, the packed head output) are stated WITHOUT their rounding to
    binary16.  scales None: nothing is quantised (then `table` = the fp32 operands).  The DCN is the package's float
    `modulated_deformable_conv2d` on the fake-quantised input, offsets, mask and weight.  tensors: a dict that receives
    every tensor by name.  -> (heat map after the sigmoid, wh, offset), fp32."""
    mdconv = mdconv if mdconv is not None else _hip_ops.modulated_deformable_conv2d
    live = {} if tensors is None else tensors
    stem = model.backbone.stem
    fq = lambda v, name: stored(plan, name, v, scales, round_f16=False)
    for l in plan.layers:
        x = None if l.src is None else live[l.src]
        if l.op == "stem":
            v = F.max_pool2d(F.relu(F.conv2d(image.float(), stem.weight.float(), stem.bias.float(), 2, 3)), 3, 2, 1)
        elif l.op in ("conv", "offset"):
            v = conv_statement(l, x, table[l.key], None if l.res is None else live[l.res])
        elif l.op == "dcn":
            w, sw, b = table[l.key]
            om = live[l.res]
            off, mask = fq(om[:, :18], l.extra[0]), fq(torch.sigmoid(om[:, 18:27]), l.extra[1])
            live[l.extra[0]], live[l.extra[1]] = off, mask
            v = F.relu(mdconv(x, off.contiguous(), mask.contiguous(), w.float() * sw, b, 1, 1, 1, 1, 1))
        elif l.op == "deconv":
            w, ws, b = table[l.key]
            v = F.relu(F.conv_transpose2d(x, w.float() * ws[None, :, None, None], b, 2, 1))
        elif l.op == "neck_fp16":
            v = _neck_float(model, x, mdconv)
        else:
            v = x
        live[l.dst] = fq(v, l.dst)
    packed = live["head.packed"]
    heat, wh, off = (packed[:, a:b] for a, b in table["slices"])
    return torch.sigmoid(heat), wh, off


class Int8CenterNet(Int8Model):
    """`forward(image fp16 [B, 3, H, W])` -> CenterNet.forward's three outputs (fp16, the heat map after the sigmoid:
    three channel slices of the packed [B, H/4, W/4, 88] tensor) through the int8 plan.  fp: the fp16 centernet.CenterNet
    whose weights it quantises (kept: its parameters are this module's, and a weight reload rebuilds the int8
    operands); scales: {site: scale} for every site of the plan.  `forward`, `get_bboxes`, `prepare` and `cfg` as
    CenterNet: CenterNetRunner captures and replays it unchanged."""

    def __init__(self, fp, scales, ops=None, neck="int8"):
        super().__init__(fp)
        self.ops = ops if ops is not None else _hip_ops
        self.neck_note = neck
        outside = dcn_int8_domain(fp) if neck == "int8" else []
        if outside:       # the int8 DCN block does not take these packs: the float neck of the explicit config
            neck = "fp16"
            self.neck_note = f"fp16 (DCN packs {outside} are outside the int8 block's domain: input channels % 128)"
        self.neck = neck
        self.plan = build_plan(fp, neck)
        self._set_scales(scales, self.plan.sites)

    # ---- the cached operands (Int8Model.operands: stamped with every parameter of fp)
    OPERAND = "quantised or packed"

    def _quantize(self):
        return quantize_operands(self.fp, self.plan)

    def _packs(self, table, build):
        """The parity-major packed int8 deconvolution weights and the int8 DCN weight images of `table` (and, for the
        fp16 neck, the fp16 model's own packed operands); build=False: whether all of them are cached."""
        from .functions import int8_chain as C
        from .functions.modulated_deformable_conv2d import _packed_weight
        from .utils import lib as _lib
        ok = True
        for l in self.plan.layers:
            if l.op == "deconv":
                ok &= deconv_packed_weight(table[l.key][0], build=build) is not None
            elif l.op == "dcn":
                if build and table[l.key][0].is_cuda:
                    _packed_weight(_lib.load_library(), table[l.key][0], _lib.I8, cache=C._PACKED_S8, empty=torch.empty)
                ok &= (not table[l.key][0].is_cuda) or C._PACKED_S8.get(table[l.key][0]) is not None
            elif l.op == "neck_fp16":
                if build:
                    self.fp.prepare()
                ok &= self.fp._operands_ready()
        return ok

    def prepare(self):
        """Build (or refresh) the int8 operands and their packed images; allocates, so it must run OUTSIDE stream capture."""
        self._outside_capture()
        self.operands()
        return self

    # ---- the int8 run
    def run(self, image, table, ops, tensors=None):
        """The layers of the plan on `ops`.  -> the packed head output [B, 88, H/4, W/4] fp16 channels-last."""
        live = {} if tensors is None else tensors
        i8, f16 = torch.int8, torch.float16
        stem = self.fp.backbone.stem
        scale_of = lambda name: None if name is None else self.scale(name)
        for l in self.plan.layers:
            x = None if l.src is None else live[l.src]
            q_out = self.plan.tensors[l.dst] == "q"
            s_out = self.scale(l.dst) if q_out else None
            if l.op == "stem":
                y = ops.stem_conv_pool(image, stem.weight, stem.bias, s_out)
            elif l.op == "conv":
                y = conv_call(ops, l, x, self.scale(l.src), table[l.key], live.get(l.res), scale_of(l.res), None, s_out)
            elif l.op == "offset":
                w, ws, b = table[l.key]
                y = ops.conv_int8_chain_nhwc(x, self.scale(l.src), w, ws, b, False, 1, f16)
            elif l.op == "dcn":
                w, sw, b = table[l.key]
                y = ops.modulated_deformable_conv2d_int8_nhwc(x, self.scale(l.src), live[l.res], self.scale(l.extra[0]),
                                                              self.scale(l.extra[1]), w, sw, b, s_out, True, 1, 1, 1, 1, 1)
            elif l.op == "deconv":
                w, ws, b = table[l.key]
                y = ops.conv_transpose2d_q_nhwc(x, self.scale(l.src), w, ws, b, True, s_out, i8)
            elif l.op == "neck_fp16":
                y = self.fp.neck.forward_nhwc(x, ops)
            else:   # "quantize": one pass over the neck's fp16 output (rows of a channels-last tensor)
                y = ops.quantize_rows(x.permute(0, 2, 3, 1), s_out).permute(0, 3, 1, 2)
            live[l.dst] = y
        return live["head.packed"]

    @torch.no_grad()
    def forward(self, image):
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] % 32 or image.shape[3] % 32:
            raise ValueError(f"CenterNet: image [B, 3, H, W] with H and W multiples of 32, got {tuple(image.shape)}")
        table = self._ready(image, "an fp16 CUDA image")
        with _dispatch.using(rule=True):
            packed = self.run(image.contiguous(), table, self.ops)
        heat, wh, off = (packed[:, a:b] for a, b in table["slices"])
        heat.sigmoid_()
        return heat, wh, off

    @torch.no_grad()
    def fake_quant_reference(self, image, quantize=True, tensors=None):
        """The fp32 torch statement of `forward` (quantise and dequantise at every int8 tensor with the same scales, the
        same weight quantisation): independent of the kernels.  quantize=False: the same statements on the
        un-quantised weights with no fake quantisation -- the fp32 plain path.  -> three fp32 outputs."""
        if quantize:
            return emulate(self.fp, self.plan, image, self.operands(), self.scales, tensors=tensors)
        return emulate(self.fp, self.plan, image, _float_operands(self.fp, self.plan), None, tensors=tensors)

    def get_bboxes(self, outputs, img_metas, rescale=True):
        return _cn.CenterNet.get_bboxes(self, outputs, img_metas, rescale)


# ---- calibration

def all_sites(fp):
    """Every site a calibration run visits: the union of both neck modes' sites (the last block's output is a site of
    the int8 neck only; everything else the fp16 neck reads is a site of the int8 neck too)."""
    return build_plan(fp, "int8").sites


def calibrate(fp, images, cal, ops=None):
    """Run the fp16 fast path of `fp` on `images` (an iterable of fp16 CUDA images) layer by layer, collecting every
    tensor the plans quantise under its site -- one site per tensor, both neck modes served by one run.  -> the number
    of frames."""
    ops = ops if ops is not None else fp.ops
    fp.prepare()
    w1, b1, _, _, _ = fp.heads_merged()
    stem = fp.backbone.stem
    site = lambda name, t: cal.collect(SITE_PREFIX + name, t)
    n = 0
    with torch.no_grad(), _dispatch.using(rule=True):
        for image in images:
            x = ops.stem_conv_pool(image.contiguous(), stem.weight, stem.bias)
            site("stem", x)
            for i, stage in enumerate(fp.backbone.stages):
                for j, blk in enumerate(stage):
                    name = f"s{i}.b{j}"
                    idt = x
                    if blk.downsample is not None:
                        idt = _B._conv1x1_nhwc(ops, x, blk.downsample, False)
                        site(name + ".idt", idt)
                    t = _B._conv_nhwc(ops, x, blk.conv1, True)
                    site(name + ".t1", t)
                    x = _B._conv_nhwc(ops, t, blk.conv2, True, idt)
                    site(name + ".out", x)
            for l, (dcn, up) in enumerate(zip(fp.neck.dcn, fp.neck.deconv)):
                dcn.chain_cal, dcn.chain_site = cal, f"{SITE_PREFIX}neck{l}"      # (DCNv2Pack._chain_collect: .offset, .mask)
                try:
                    x = dcn.forward_nhwc(x, True)
                finally:
                    del dcn.chain_cal, dcn.chain_site
                site(f"neck{l}.dcn", x)
                x = ops.conv_transpose2d_nhwc(x, up.weight, up.bias, relu=True)
                site(f"neck{l}.up", x)
            site("head.hidden", ops.conv_nhwc(x, w1, b1, True))
            n += 1
    return n
