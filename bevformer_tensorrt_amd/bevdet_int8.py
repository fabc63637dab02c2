"""The INT8 BEV half of BEVDet-R50 (bevdet.py): everything behind the image neck on the int8 matrix cores, every tensor
between two layers one byte per element -- what "INT8" means for YOLOX and CenterNet here (yolox_int8.py,
centernet_int8.py) and for the reference's TensorRT build.  quantization.build_int8_bevdet(bev_half="int8") puts it behind
the int8 image chain.  design/bevdet_int8.md.

THE PLAN (`build_plan`) is a list of layers on NAMED tensors; one description serves the layer and site counts (no
tensor needed), the int8 run and the fp32 fake-quant statement of the tests:

  quantize    the fp16 image-neck output, one pass                                     quantize_rows
  depth_net   256 -> 128 merged columns [features | depth logits | zeros], fp16 out    conv_slice_q_taps (1 x 1)
  split       softmax over the depth bins + split -> int8 depth planes, int8 features  lss_depth_split_q
  pool        int8 in, int32 sums, int8 BEV [1, 128, 128, 64]                           bev_pool_v2_int8 / _indirect
  BasicBlock  3x3 / 2 downsample, conv1 3x3 + ReLU, conv2 3x3 + identity + ReLU with the
              identity IN FRONT of the ReLU                                            conv_slice_q_taps(res_first=True)
  upsample    align_corners bilinear x 4 into channels 128 .. 640 of the 640-channel
              buffer whose first 128 channels stage 1's last block wrote; x 2          upsample_bilinear_nhwc_q
  neck_conv, up2_conv, shared_conv, the heads as 64 -> 384 (int8 out) and the
              block-diagonal 384 -> 32 (fp16 out: the packed tensor the decode reads)   conv_slice_q_taps

ONE SCALE PER TENSOR, one calibration site ("bevdet." + name) each.  The concatenation buffer is ONE group ("cat") with
two writers, stage 1's last block and the x 4 up-sampler: both requantise with the group's scale (YOLOX's rule).  What
stays fp16: depth_net's logits (the softmax input; 59 bins of exponentials do not survive 8 bits) and the packed head
output (what centerpoint_decode / get_candidates / get_bboxes read; post-processing is untouched)."""
import torch
import torch.nn.functional as F

from . import bevdet as _bd
from . import functions as _hip_ops
from .functions import dispatch as _dispatch
from .functions import yolox_ops as _Y
from .int8_plan import (Int8Model, Layer, Plan, basic_block_conv, basic_block_layers, conv_call, conv_statement,   # noqa: F401
                        float_operands, load_calibration, out_slice, place, save_calibration, scales_from, stored)

SITE_PREFIX = "bevdet."
CAT = "cat"


# Layer ops: "quantize", "conv", "split", "pool", "upsample" (bevdepth_int8.py adds "gate" and "avgpool").
INT8_OPS = ("conv", "pool")


def build_plan(model):
    """The layers of `model`'s (a bevdet.BEVDet) BEV half in the order of its fast path."""
    P = Plan(SITE_PREFIX, INT8_OPS)
    x = P.add(Layer("quantize", None, "x.f16", "x"))
    dn = P.add(Layer("conv", "depth_net", x, "depth_net"), "f16")
    P.add(Layer("split", None, dn, "feat", extra=("depth",)))
    x = P.add(Layer("pool", None, "depth", "bev", res="feat"))
    widths = [stage[0].conv1.out_channels for stage in model.bev_stages]
    c_cat = widths[0] + widths[-1]
    P.buffers[CAT] = c_cat
    feats = []
    for i, stage in enumerate(model.bev_stages):
        for j, blk in enumerate(stage):
            x = basic_block_layers(P, blk, f"s{i}.b{j}", x, into=(CAT, 0) if i == 0 and j == len(stage) - 1 else None)
        feats.append(x)
    P.add(Layer("upsample", None, feats[-1], "up4", into=(CAT, widths[0]), factor=4))
    x = P.add(Layer("conv", "neck_conv.0", CAT, "neck0", act="relu"))
    x = P.add(Layer("conv", "neck_conv.1", x, "neck1", act="relu"))
    x = P.add(Layer("upsample", None, x, "up2", factor=2))
    x = P.add(Layer("conv", "up2_conv.0", x, "u0", act="relu"))
    x = P.add(Layer("conv", "up2_conv.1", x, "u1"))
    x = P.add(Layer("conv", "shared_conv", x, "shared", act="relu"))
    h = P.add(Layer("conv", "head.first", x, "head.hidden", act="relu"))
    P.add(Layer("conv", "head.final", h, "head.packed"), "f16")
    P.readable(CAT)
    return P


def _conv_of(model, key):
    if key[0] == "s" and key[1].isdigit():
        return basic_block_conv(model.bev_stages[int(key[1])][int(key[4])], key[6:])
    if key == "shared_conv":
        return model.shared_conv
    name, i = key.split(".")
    return getattr(model, name)[int(i)]


def _sources(model, plan):
    """{key: (weight [Cout, Cin, k, k], bias)} of every convolution of `plan`; the merged operands of depth_net and the
    heads come from bevdet.merge_depth_net / merge_heads.  -> (table, depth_net layout, head slices)."""
    w, b, lay = model.view.depth_net_merged()
    w1, b1, w2, b2, slices = model.heads_merged()
    table = {}
    for l in plan.layers:
        if l.op != "conv":
            continue
        if l.key == "depth_net":
            table[l.key] = (w.reshape(w.shape[0], w.shape[1], 1, 1), b)
        elif l.key.startswith("head."):
            table[l.key] = (w1, b1) if l.key == "head.first" else (w2, b2)
        else:
            c = _conv_of(model, l.key)
            table[l.key] = (c.weight, c.bias)
    return table, lay, slices


def quantize_operands(model, plan):
    """{key: (w_q_taps int8 [Cout, k, k, Cin], w_scales fp32 [Cout], bias fp32 [Cout])} per output channel
    (functions.yolox_ops.quantize_weight_taps); "layout": merge_depth_net's column layout; "slices": the heads'."""
    src, lay, slices = _sources(model, plan)
    table = {k: _Y.quantize_weight_taps(w, b) for k, (w, b) in src.items()}
    table["layout"], table["slices"] = lay, slices
    return table


def _float_operands(model, plan):
    """The un-quantised fp32 operands in the layouts of `quantize_operands` with unit scales."""
    src, lay, slices = _sources(model, plan)
    return dict(float_operands(src), layout=lay, slices=slices)


def pool_statement(depth_q, feat_q, ranks, sio, cells):
    """bev_pool_v2 in BEVOPS_I8 as a torch statement: exact integer sums of depth_q[ranks_depth] feat_q[ranks_feat] per
    cell (float64 holds them exactly), then the plugin's requantisation q = t2int8((float)sum * sio): clamp to
    [-128, 127], round half away from zero; sio = scale_depth * scale_feat / scale_out in fp32.  depth_q / feat_q integer
    valued tensors [N, D, H, W] / [N, H, W, C]; ranks = (ranks_bev, ranks_depth, ranks_feat) trimmed.  -> [cells, C]."""
    rb, rd, rf = (r.long() for r in ranks)
    C = feat_q.shape[-1]
    acc = torch.zeros((cells, C), dtype=torch.float64, device=feat_q.device)
    step = 1 << 16
    d, f = depth_q.reshape(-1).double(), feat_q.reshape(-1, C).double()
    for i in range(0, rb.numel(), step):
        acc.index_add_(0, rb[i:i + step], d[rd[i:i + step], None] * f[rf[i:i + step]])
    a = torch.clamp(acc.float() * sio, -128.0, 127.0)
    return torch.trunc(a + torch.where(a > 0, 0.5, -0.5))


def emulate(model, plan, x, ranks, table, scales, tensors=None, layers=None, other=None):
    """The fp32 torch statement of the int8 BEV half from the fp16 image features x [cams, Cin, H, W]: NCHW fp32 tensors
    holding q * scale, fake quantisation (`fake_quant`: the kernels' clamp(rne(v * (1 / scale)), -127, 127) * scale) at
    every int8 tensor of the plan, depth_net's logits rounded to binary16, the pooling's integer sums and its own rounding.
    scales None: nothing is quantised or rounded (then `table` = the fp32 operands) -- the fp32 plain path.
    ranks = (ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths) trimmed.  -> the packed [1, 32, h, w].
    layers: the part of plan.layers to run on the tensors already in `tensors` (bevdepth_int8.py: everything from the split
    on, behind its own DepthNet statement); None: all of them.  other(layer, src, live) -> the value of a layer whose op this
    plan does not have (bevdepth_int8.py: "gate", "avgpool")."""
    live = {} if tensors is None else tensors
    view = model.view
    D, C = view.D, view.out_channels
    bev_h, bev_w = int(view.grid_size[1]), int(view.grid_size[0])
    lay = table["layout"]
    sc = (lambda name: scales[plan.site(name)]) if scales is not None else None
    fq = lambda v, name: stored(plan, name, v, scales, round_f16=True)
    live["x.f16"] = x.float()
    for l in (plan.layers if layers is None else layers):
        src = live[l.src]
        if l.op == "quantize":
            v = fq(src, l.dst)
        elif l.op == "conv":
            v = fq(conv_statement(l, src, table[l.key], live.get(l.res), live.get(l.image_bias)), l.dst)
        elif l.op == "split":
            do, fo = lay["depth_offset"], lay["feat_offset"]
            live["depth"] = fq(src[:, do:do + D].softmax(dim=1), "depth")
            v = fq(src[:, fo:fo + C].permute(0, 2, 3, 1), "feat")
        elif l.op == "pool":
            depth, feat = src, live[l.res]
            if scales is None:
                acc = torch.zeros((bev_h * bev_w, C), dtype=torch.float64, device=feat.device)
                rb, rd, rf = (r.long() for r in ranks[:3])
                acc.index_add_(0, rb, depth.reshape(-1).double()[rd, None] * feat.reshape(-1, C).double()[rf])
                v = acc.float()
            else:
                sd, sf, so = sc("depth"), sc("feat"), sc(l.dst)
                f32 = lambda s: torch.tensor(s, dtype=torch.float32)
                sio = float(f32(sd) * f32(sf) / f32(so))
                q = pool_statement(torch.round(depth / sd), torch.round(feat / sf), ranks[:3], sio, bev_h * bev_w)
                v = q * so
            v = v.view(1, bev_h, bev_w, C).permute(0, 3, 1, 2)
        elif l.op == "upsample":
            v = fq(F.interpolate(src, scale_factor=l.factor, mode="bilinear", align_corners=True), l.dst)
        else:
            v = other(l, src, live)
        live[l.dst] = place(plan, l, live, v)
    return live.get("head.packed")                  # (None when `layers` ends in front of the heads)


class Int8BEVDet(Int8Model):
    """The INT8 BEVDet: the image half is `fp`'s int8 activation chain (quantization.Int8ChainBackbone, frozen), the BEV
    half the int8 plan above.  fp: the bevdet.BEVDet whose weights it quantises (kept: its parameters are this module's,
    and a weight reload rebuilds the int8 operands); scales: {site: scale} for every site of the plan.  `forward`,
    `forward_calibrated`, `bev_half_calibrated`, `get_candidates`, `get_bboxes`, `prepare_bev_half` as BEVDet:
    BEVDetRunner captures and replays it unchanged."""

    def __init__(self, fp, scales, ops=None):
        super().__init__(fp)
        self.bev_ops = ops if ops is not None else _hip_ops
        self.plan = self._plan_of(fp)
        self._set_scales(scales, self.plan.sites)

    # ---- the plan and its statements (bevdepth_int8.Int8BEVDepth puts its own in their place)
    _plan_of = staticmethod(build_plan)
    _quantize_of = staticmethod(quantize_operands)
    _floats = staticmethod(_float_operands)

    # ---- what BEVDetRunner and the post-processing read
    @property
    def view(self):
        return self.fp.view

    @property
    def ops(self):
        return self.fp.ops

    @property
    def bbox_coder(self):
        return self.fp.bbox_coder

    test_cfg = _bd.BEVDet.test_cfg

    def get_candidates(self, outputs, padded=False):
        return _bd.BEVDet.get_candidates(self, outputs, padded)

    def get_bboxes(self, outputs, padded=False):
        return _bd.BEVDet.get_bboxes(self, outputs, padded)

    # ---- the cached operands (Int8Model.operands: stamped with every BEV-half parameter)
    PREPARE, OPERAND = "prepare_bev_half", "merged or quantised"

    def _stamped(self):
        fp = self.fp
        mods = [fp.view.depth_net, fp.bev_stages, fp.neck_conv, fp.up2_conv, fp.shared_conv, fp.heads]
        return [p for m in mods for p in m.parameters()]

    def _quantize(self):
        return self._quantize_of(self.fp, self.plan)

    def prepare_bev_half(self):
        """Build (or refresh) the merged int8 operands; allocates, so it must run OUTSIDE stream capture."""
        p = self._outside_capture()
        if p.is_cuda and p.dtype == torch.float16:
            self.fp._nhwc_weights()   # (what the first fp16 frame does to the filters; the operands' stamps follow them)
        self.operands()
        return self

    # ---- the int8 run
    def run(self, x, pool, table, ops, tensors=None, layers=None, other=None):
        """The layers of the plan on `ops` from the fp16 image features x [cams, Cin, H, W] (channels-last); pool(depth_q,
        feat_q, scales) runs the pooling.  -> the packed head output [1, 32, h, w] fp16 channels-last.  layers: the part
        of the plan to run on the tensors already in `tensors` (None: all of it); other(layer, src, live, scale_out) runs a
        layer whose op this plan does not have (bevdepth_int8.py: "gate", "avgpool")."""
        live = {} if tensors is None else tensors
        view = self.fp.view
        lay = table["layout"]
        scale_of = lambda name: None if name is None else self.scale(name)
        live["x.f16"] = x
        for l in (self.plan.layers if layers is None else layers):
            src = live[l.src]
            q_out = self.plan.tensors[l.dst] == "q"
            s_out = self.scale(l.dst) if q_out else None
            out = out_slice(self.plan, l, live, src, table[l.key][0].shape[0] if l.op == "conv" else src.shape[1],
                            torch.int8 if q_out else torch.float16)
            if l.op == "quantize":
                y = ops.quantize_rows(src.permute(0, 2, 3, 1), s_out).permute(0, 3, 1, 2)
            elif l.op == "conv":
                y = conv_call(ops, l, src, self.scale(l.src), table[l.key], live.get(l.res), scale_of(l.res), out, s_out,
                              live.get(l.image_bias))
            elif l.op == "split":
                n, c, h, w = src.shape
                rows = src.permute(0, 2, 3, 1).reshape(n * h * w, c)          # (a view: channels-last)
                live["depth"], y = ops.lss_depth_split_q(rows, n, view.D, view.out_channels, lay["depth_offset"],
                                                         lay["feat_offset"], self.scale("depth"), s_out, spatial=(h, w))
            elif l.op == "pool":
                y = pool(src, live[l.res], (self.scale(l.src), self.scale(l.res), s_out)).permute(0, 3, 1, 2)
            elif l.op == "upsample":
                y = ops.upsample_bilinear_nhwc_q(src, self.scale(l.src), s_out, scale_factor=l.factor, out=out)
            else:
                y = other(l, src, live, s_out)
            live[l.dst] = y
        return live.get("head.packed")              # (None when `layers` ends in front of the heads)

    def _heads(self, packed, table):
        return tuple(packed[:, a:b] for a, b in table["slices"])

    def _features(self, image):
        x = self.fp.image_features(image.flatten(0, 1))
        return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)

    @torch.no_grad()
    def forward(self, image, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths):
        table = self._ready(image)
        ops = self.bev_ops
        h, w = int(self.view.grid_size[1]), int(self.view.grid_size[0])
        pool = lambda d, f, s: ops.bev_pool_v2_int8(d, f, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                                    interval_lengths, *s, h, w)
        with _dispatch.using(rule=True):
            return self._heads(self.run(self._features(image), pool, table, ops), table)

    @torch.no_grad()
    def forward_calibrated(self, image, calib):
        self._ready(image)
        with _dispatch.using(rule=True):
            x = self._features(image)
        return self.bev_half_calibrated(x, calib)

    @torch.no_grad()
    def bev_half_calibrated(self, x, calib):
        """Everything behind `image_features`: x = its fp16 [cams, 256, H / 16, W / 16] channels-last result; the index
        build and the pooling run on the device from the packed calibration buffer.  calib [B, cams * 24 + 9] with x
        [B * cams, ...]: the plan runs for B samples -- the pooled view [B, h, w, C], every later tensor with B items (the
        concatenation buffer [B, 64, 64, 640]); same operands, same scales."""
        table = self._ready(x)
        ops = self.bev_ops
        rb, rd, rf, ist, il, counts = self.view.prepare_calibrated(calib)
        h, w = int(self.view.grid_size[1]), int(self.view.grid_size[0])
        kw = {}
        if calib.dim() == 2:
            if x.shape[0] * 24 != calib.shape[0] * (calib.shape[1] - 9):
                raise ValueError(f"calib {tuple(calib.shape)} does not describe the {x.shape[0]} camera images of x")
            kw["batch"] = calib.shape[0]
        pool = lambda d, f, s: ops.bev_pool_v2_indirect(d, f, rd, rf, rb, ist, il, counts, h, w, scales=s, **kw)
        with _dispatch.using(rule=True):
            return self._heads(self.run(x, pool, table, ops), table)

    @torch.no_grad()
    def fake_quant_reference(self, x, ranks, quantize=True, tensors=None):
        """The fp32 torch statement of the BEV half from the image features x (quantise and dequantise at every int8
        tensor with the same scales, the same weight quantisation): independent of the kernels.  quantize=False: the same
        statements on the un-quantised weights with no fake quantisation -- the fp32 plain path.  ranks: the five trimmed
        index arrays.  -> the six head outputs, fp32."""
        if quantize:
            table, scales = self.operands(), self.scales
        else:
            table, scales = self._floats(self.fp, self.plan), None
        return self._heads(emulate(self.fp, self.plan, x, ranks, table, scales, tensors), table)


# ---- calibration

def calibrate_frame(fp, x, ranks, cal, ops=None):
    """The BEV half of `fp` on the fp16 "hip" path's kernels from one frame's fp16 image features x, layer by layer,
    collecting every tensor the plan quantises under its site (the concatenation buffer as one tensor)."""
    ops = ops if ops is not None else _hip_ops
    view = fp.view
    site = lambda name, t: cal.collect(SITE_PREFIX + name, t)
    rb, rd, rf, ist, il = ranks
    conv = lambda t, c, relu=False, res=None: _bd._conv(ops, t, c, relu, res)
    with torch.no_grad(), _dispatch.using(rule=True):
        x = x.contiguous(memory_format=torch.channels_last)
        site("x", x)
        w, b, lay = view.depth_net_merged()
        n, cin, h, wd = x.shape
        y = ops.dense_auto(x.permute(0, 2, 3, 1).reshape(n * h * wd, cin), w, b, None, False)
        depth, feat = ops.lss_depth_split(y, n, view.D, view.out_channels, lay["depth_offset"], lay["feat_offset"],
                                          spatial=(h, wd))
    calibrate_behind_split(fp, depth, feat, ranks, cal, ops)


def calibrate_behind_split(fp, depth, feat, ranks, cal, ops):
    """`calibrate_frame` from the softmax + split on: depth [n, D, h, w] and feat [n, h, w, C] fp16 as lss_depth_split
    leaves them (bevdepth_int8.calibrate_frame arrives here from its own DepthNet)."""
    view = fp.view
    site = lambda name, t: cal.collect(SITE_PREFIX + name, t)
    rb, rd, rf, ist, il = ranks
    conv = lambda t, c, relu=False, res=None: _bd._conv(ops, t, c, relu, res)
    with torch.no_grad(), _dispatch.using(rule=True):
        site("depth", depth)
        site("feat", feat)
        x = ops.bev_pool_v2_2(depth, feat, rd, rf, rb, ist, il, int(view.grid_size[1]), int(view.grid_size[0]))
        x = x.permute(0, 3, 1, 2)
        site("bev", x)
        feats = []
        for i, stage in enumerate(fp.bev_stages):
            for j, blk in enumerate(stage):
                name = f"s{i}.b{j}"
                idt = x
                if blk.downsample is not None:
                    idt = conv(x, blk.downsample)
                    site(name + ".idt", idt)
                t = conv(x, blk.conv1, True)
                site(name + ".t1", t)
                x = conv(t, blk.conv2, True, idt)
                if not (i == 0 and j == len(stage) - 1):
                    site(name + ".out", x)
            feats.append(x)
        x = ops.upsample_bilinear_concat_nhwc(feats[0], feats[-1])
        site(CAT, x)
        x = conv(x, fp.neck_conv[0], True)
        site("neck0", x)
        x = conv(x, fp.neck_conv[1], True)
        site("neck1", x)
        x = ops.upsample_bilinear_concat_nhwc(None, x, scale_factor=2)
        site("up2", x)
        x = conv(x, fp.up2_conv[0], True)
        site("u0", x)
        x = conv(x, fp.up2_conv[1])
        site("u1", x)
        x = conv(x, fp.shared_conv, True)
        site("shared", x)
        w1, b1, _, _, _ = fp.heads_merged()
        site("head.hidden", ops.conv_nhwc(x, w1, b1, True))
