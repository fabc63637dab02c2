"""The INT8 build of YOLOX (yolox.py): every convolution of the backbone, the PAFPN and the head on
bevops_conv_slice_s8, every tensor between two layers int8 -- what TensorRT builds from the reference's
configs/yolox/yolox_x_8x8_300e_coco_trt_q.py (`Conv2dQ` in the backbone, the neck and the head).  design/yolox_int8.md.

THE PLAN (`build_plan`) restates the fast path of yolox.py (YOLOX._forward_fast and the forward_fast methods) as a list
of steps on symbolic buffers, so that one description serves the scale groups (no tensor needed), the calibration run
(fp16 operators), the int8 run and the fp32 fake-quant statement of the tests.  `run_plan(..., mode="fp16")` issues the
calls of the fp16 fast path, in its order, on buffers of its shapes: its nine outputs equal YOLOX.forward's bit for bit
(tests/test_yolox_int8_gpu.py).

ONE SCALE PER BUFFER.  Every buffer of the plan (every `nhwc_empty` of the fast path) is one scale group: all channel
slices of a concatenation buffer are read by ONE convolution with ONE scale_a, so their producers requantise with one
scale.  The two data movers that keep their input's scale merge groups: nearest up-sampling copies bytes, so the group
of its source joins the group of its destination (-> [up(high5) | c4] and [down1 | high5] share one scale, and so do
[up(high4) | c3] and [down0 | high4]); the SPP pools write three quarters of the buffer their source is the first
quarter of.  A group's calibration statistic is collected under ONE site name from every slice written into it, so it
is the joint statistic of the union.  The three packed predictor outputs are fp16 and belong to no group."""
import torch
import torch.nn.functional as F

from . import functions as _hip_ops
from . import yolox as _yx
from .functions import yolox_ops as _Y
from .int8_plan import Int8Model, fake_quant, load_calibration, save_calibration, scales_from   # noqa: F401


class Ref:
    """Channels [c0, c0 + C) of buffer `buf`; div: the image's size over the map's."""

    def __init__(self, buf, c0, C, div):
        self.buf, self.c0, self.C, self.div = buf, c0, C, div

    def part(self, c0, C=None):
        C = self.C - c0 if C is None else C
        assert 0 <= c0 and c0 + C <= self.C
        return Ref(self.buf, self.c0 + c0, C, self.div)


class Step:
    """op in "focus", "conv", "pool", "up"; key: the operand-table key of a convolution."""

    def __init__(self, op, src, dst, key=None, res=None, act=None, stride=1, ks=None):
        self.op, self.src, self.dst, self.key, self.res, self.act, self.stride, self.ks = op, src, dst, key, res, act, stride, ks


class Plan:
    def __init__(self):
        self.bufs, self.steps, self.outputs = [], [], []    # bufs: (channels, div, "q" | "f16")

    def new(self, C, div, kind="q"):
        self.bufs.append((C, div, kind))
        return Ref(len(self.bufs) - 1, 0, C, div)

    # ---- scale groups: union-find over the int8 buffers
    def groups(self):
        """-> (group id of every buffer, None for the fp16 ones; number of groups).  Ids count in the order of the groups'
        first buffers."""
        parent = list(range(len(self.bufs)))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i

        for s in self.steps:
            if s.op in ("up", "pool") and s.src.buf != s.dst.buf:
                a, b = find(s.src.buf), find(s.dst.buf)
                parent[max(a, b)] = min(a, b)
        ids, out = {}, []
        for i, (_, _, kind) in enumerate(self.bufs):
            if kind != "q":
                out.append(None)
                continue
            out.append(ids.setdefault(find(i), len(ids)))
        return out, len(ids)


def build_plan(model):
    """The steps of YOLOX._forward_fast for `model` (a yolox.YOLOX), in its order."""
    P, pw = Plan(), _Y.padded_width

    def run(conv, x, residual=None, out=None, key=None, cout=None, act=None, kind="q"):
        cout = pw(conv.out_channels) if cout is None else cout
        stride = conv.stride[0]
        if out is None:
            out = P.new(cout, x.div * stride, kind)
        assert out.C == cout and out.div == x.div * stride and (residual is None or residual.C == cout)
        P.steps.append(Step("conv", x, out, conv if key is None else key, residual, conv.act if act is None else act, stride))
        return out

    def csp(layer, x, out=None):
        pm = pw(layer.mid)
        cat = P.new(2 * pm, x.div)
        run(layer.short_conv, x, out=cat.part(pm))
        main = run(layer.main_conv, x)
        for j, blk in enumerate(layer.blocks):
            hidden = run(blk.conv1, main)
            main = run(blk.conv2, hidden, residual=main if blk.add_identity else None,
                       out=cat.part(0, pm) if j == len(layer.blocks) - 1 else None)
        return run(layer.final_conv, cat, out=out)

    neck, head = model.neck, model.bbox_head
    c = neck.in_channels
    # YOLOXPAFPN.buffers: td0 [up(reduce 0) | c4], td1 [up(reduce 1) | c3], bu0 [down 0 | reduce 1], bu1 [down 1 | reduce 0]
    td0, td1, bu0, bu1 = P.new(2 * c[1], 16), P.new(2 * c[0], 8), P.new(2 * c[0], 16), P.new(2 * c[1], 32)
    dests = (td1.part(c[0]), td0.part(c[1]), None)
    x = P.new(_Y.FOCUS_CHANNELS, 2)
    P.steps.append(Step("focus", None, x))
    x = run(model.backbone.stem.conv, x)
    outs = []
    for i, stage in enumerate(model.backbone.stages):
        x = run(stage[0], x)
        if len(stage) == 3:
            spp = stage[1]
            pm = pw(spp.mid)
            cat = P.new(4 * pm, x.div)
            run(spp.conv1, x, out=cat.part(0, pm))
            P.steps.append(Step("pool", cat.part(0, pm), cat.part(pm), ks=spp.kernel_sizes))
            x = run(spp.conv2, cat)
        x = csp(stage[-1], x, out=dests[i - 1] if i >= 1 else None)
        outs.append(x)
    c5 = outs[3]
    high5 = run(neck.reduce_layers[0], c5, out=bu1.part(c[1]))
    P.steps.append(Step("up", high5, td0.part(0, c[1])))
    inner4 = csp(neck.top_down_blocks[0], td0)
    high4 = run(neck.reduce_layers[1], inner4, out=bu0.part(c[0]))
    P.steps.append(Step("up", high4, td1.part(0, c[0])))
    out0 = csp(neck.top_down_blocks[1], td1)
    run(neck.downsamples[0], out0, out=bu0.part(0, c[0]))
    out1 = csp(neck.bottom_up_blocks[0], bu0)
    run(neck.downsamples[1], out1, out=bu1.part(0, c[1]))
    out2 = csp(neck.bottom_up_blocks[1], bu1)
    feats = tuple(run(conv, o) for conv, o in zip(neck.out_convs, (out0, out1, out2)))
    feat = head.feat
    n_pred = (head.num_classes + 5 + _yx.HEAD_PACK_MULTIPLE - 1) // _yx.HEAD_PACK_MULTIPLE * _yx.HEAD_PACK_MULTIPLE
    for l, x in enumerate(feats):
        first = run(head.cls_convs[l][0], x, key=("first", l), cout=2 * feat)
        second = P.new(2 * feat, x.div)
        run(head.cls_convs[l][1], first.part(0, feat), out=second.part(0, feat))
        run(head.reg_convs[l][1], first.part(feat), out=second.part(feat))
        P.outputs.append(run(head.cls_convs[l][1], second, key=("pred", l), cout=n_pred, act="none", kind="f16"))
    return P


def group_site(g):
    return f"yolox.group{g}"


def quantize_operands(model):
    """{key: (w_q_taps int8, w_scales fp32, bias fp32)} for every convolution of the plan, from the fp weights of
    `model`: per output channel min-max after the padding and merging of YOLOX._build_operands
    (functions.yolox_ops.quantize_weight_taps)."""
    table, head = {}, model.bbox_head
    for m in model.modules():
        if isinstance(m, _yx.ConvAct):
            table[m] = _Y.quantize_weight_taps(m.weight, m.bias, groups_in=m.groups_in)
    for l in range(len(head.cls_convs)):
        a, r = head.cls_convs[l][0], head.reg_convs[l][0]
        table[("first", l)] = _Y.quantize_weight_taps(torch.cat([a.weight.detach(), r.weight.detach()], 0),
                                                      torch.cat([a.bias.detach(), r.bias.detach()], 0))
        w, b, slices = _yx.merge_yolox_predictors(*((c[l].weight, c[l].bias) for c in (head.conv_cls, head.conv_reg,
                                                                                      head.conv_obj)))
        table[("pred", l)] = _Y.quantize_weight_taps(w, b, multiple=_yx.HEAD_PACK_MULTIPLE)
        table["slices"] = slices
    return table


def run_plan(plan, image, mode, ops, table, scales=None, collect=None):
    """One forward of `plan`.  mode "fp16": the fp16 fast path's calls (`table` = YOLOX.operands()); "int8": the int8
    operators (`table` = quantize_operands(), scales[g] per group); "emulate": the fp32 fake-quant statement of the int8
    run in torch ops alone (NCHW fp32 tensors holding q * scale; scales None: no activation is quantised).
    collect(group, written slice): called in "fp16" and "emulate" mode behind every write of a convolution or of Focus
    into an int8 group's buffer.  -> the three packed predictor outputs [B, P, H, W]."""
    B, _, H, W = image.shape
    gid, _ = plan.groups()
    last = {}
    for i, s in enumerate(plan.steps):
        for r in (s.src, s.dst, s.res):
            if r is not None:
                last[r.buf] = i
    keep = {r.buf for r in plan.outputs}
    live = {}

    def view(r):
        if r.buf not in live:
            C, div, kind = plan.bufs[r.buf]
            if mode == "emulate":
                live[r.buf] = torch.zeros((B, C, H // div, W // div), device=image.device, dtype=torch.float32)
            else:
                dtype = torch.int8 if (mode == "int8" and kind == "q") else torch.float16
                live[r.buf] = _Y.nhwc_empty(B, C, H // div, W // div, image.device, dtype)
        return live[r.buf][:, r.c0:r.c0 + r.C]

    def scale_of(r):
        g = gid[r.buf]
        return None if g is None else scales[g]

    def fq(v, r):                              # "emulate" without scales: the plan in fp32, nothing quantised
        return v if scales is None else fake_quant(v, scale_of(r))

    for i, s in enumerate(plan.steps):
        dst = view(s.dst)
        if mode == "fp16":
            if s.op == "focus":
                ops.focus_nhwc(image, out=dst)
            elif s.op == "conv":
                w, b = table[s.key]
                ops.conv_slice_taps(view(s.src), w, b, s.act, None if s.res is None else view(s.res), s.stride, dst)
            elif s.op == "pool":
                ops.spp_maxpool_nhwc(view(s.src), out=dst, kernel_sizes=s.ks)
            else:
                ops.upsample_nearest2x_nhwc(view(s.src), out=dst)
            if collect is not None and s.op in ("focus", "conv") and gid[s.dst.buf] is not None:
                collect(gid[s.dst.buf], dst)
        elif mode == "int8":
            if s.op == "focus":
                ops.focus_nhwc_q(image, scale_of(s.dst), out=dst)
            elif s.op == "conv":
                w, ws, b = table[s.key]
                f16 = gid[s.dst.buf] is None
                ops.conv_slice_q_taps(view(s.src), scale_of(s.src), w, ws, b, s.act,
                                      None if s.res is None else view(s.res), 1.0 if s.res is None else scale_of(s.res),
                                      s.stride, dst, None if f16 else scale_of(s.dst),
                                      torch.float16 if f16 else torch.int8)
            elif s.op == "pool":
                ops.spp_maxpool_nhwc(view(s.src), out=dst, kernel_sizes=s.ks)
            else:
                ops.upsample_nearest2x_nhwc(view(s.src), out=dst)
        else:
            if s.op == "focus":
                x = image.float()
                tl, tr, bl, br = x[..., ::2, ::2], x[..., ::2, 1::2], x[..., 1::2, ::2], x[..., 1::2, 1::2]
                dst.zero_()
                dst[:, :12] = fq(torch.cat((tl, bl, tr, br), dim=1), s.dst)
            elif s.op == "conv":
                w, ws, b = table[s.key]
                wf = (w.float() * ws[:, None, None, None]).permute(0, 3, 1, 2)
                v = F.conv2d(view(s.src), wf, b, s.stride, w.shape[1] // 2)
                v = _yx.silu(v) if s.act == "silu" else (F.relu(v) if s.act == "relu" else v)
                if s.res is not None:
                    v = v + view(s.res)
                dst.copy_(v if gid[s.dst.buf] is None else fq(v, s.dst))
            elif s.op == "pool":
                dst.copy_(torch.cat([F.max_pool2d(view(s.src), k, 1, k // 2) for k in s.ks], dim=1))
            else:
                dst.copy_(F.interpolate(view(s.src), scale_factor=2, mode="nearest"))
            if collect is not None and s.op in ("focus", "conv") and gid[s.dst.buf] is not None:
                collect(gid[s.dst.buf], dst)
        for r in (s.src, s.dst, s.res):
            if r is not None and last[r.buf] == i and r.buf not in keep:
                live.pop(r.buf, None)
    return [live[r.buf] for r in plan.outputs]


def split_outputs(packed, slices):
    """The nine head outputs (cls 1..3, bbox 1..3, objectness 1..3) as channel slices of the three packed tensors."""
    cls, reg, obj = [], [], []
    for p in packed:
        for lst, (a, b) in zip((cls, reg, obj), slices):
            lst.append(p[:, a:b])
    return tuple(cls + reg + obj)


class Int8YOLOX(Int8Model):
    """`forward(image fp16 [B, 3, H, W])` -> YOLOX.forward's nine outputs (fp16 logits) through the int8 plan.
    fp: the fp16 yolox.YOLOX whose weights it quantises (kept: its parameters are this module's, and a weight reload
    rebuilds the int8 operands); group_scales: one scale per scale group.  `forward`, `get_bboxes` and `prepare` as
    YOLOX: YOLOXRunner captures and replays it unchanged."""

    def __init__(self, fp, group_scales, ops=None):
        super().__init__(fp)
        self.ops = ops if ops is not None else _hip_ops
        self.plan = build_plan(fp)
        self.group_of, self.num_groups = self.plan.groups()
        if len(group_scales) != self.num_groups:
            raise ValueError(f"Int8YOLOX: {self.num_groups} scale groups, {len(group_scales)} scales")
        sites = [group_site(g) for g in range(self.num_groups)]
        self._set_scales(dict(zip(sites, group_scales)), sites, what="group scale")
        self.group_scales = [self.scales[s] for s in sites]

    @property
    def num_int8_layers(self):
        return sum(1 for s in self.plan.steps if s.op == "conv")

    def _quantize(self):
        return quantize_operands(self.fp)

    def prepare(self):
        """Build (or refresh) the int8 operands; allocates, so it must run OUTSIDE stream capture."""
        self._outside_capture()
        self.operands()
        return self

    @torch.no_grad()
    def forward(self, image):
        if image.dim() != 4 or image.shape[1] != 3 or image.shape[2] % 32 or image.shape[3] % 32:
            raise ValueError(f"YOLOX: image [B, 3, H, W] with H and W multiples of 32, got {tuple(image.shape)}")
        table = self._ready(image, "an fp16 CUDA image")
        packed = run_plan(self.plan, image.contiguous(), "int8", self.ops, table, self.group_scales)
        return split_outputs(packed, table["slices"])

    @torch.no_grad()
    def fake_quant_reference(self, image):
        """The fp32 torch statement of `forward` (quantise and dequantise at every group with the same scales, the same
        per-channel weight quantisation): independent of the kernels.  -> nine fp32 outputs."""
        table = self.operands()
        packed = run_plan(self.plan, image, "emulate", None, table, self.group_scales)
        return split_outputs(packed, table["slices"])

    def get_bboxes(self, outputs, img_metas, rescale=True):
        return _yx.YOLOX.get_bboxes(self, outputs, img_metas, rescale)


# ---- calibration

def calibrate(fp, images, cal, ops=None):
    """Run the fp16 fast path of `fp` on `images` (an iterable of fp16 CUDA images), collecting every write into an
    int8 group's buffer under the group's site.  -> the number of frames."""
    ops = ops if ops is not None else _hip_ops
    plan = build_plan(fp)
    fp.prepare()
    n = 0
    with torch.no_grad():
        for image in images:
            run_plan(plan, image.contiguous(), "fp16", ops, fp.operands(),
                     collect=lambda g, t: cal.collect(group_site(g), t))
            n += 1
    return n


def group_scales_from(cal, num_groups):
    """One scale per scale group, in the order of the groups."""
    sites = [group_site(g) for g in range(num_groups)]
    return list(scales_from(cal, sites, "build_int8_yolox").values())
