"""The INT8 BEVDepth: the camera-aware DepthNet with ASPP (bevdepth.py) on the int8 matrix cores, in front of the int8
BEV half of bevdet_int8.py.  quantization.build_int8_bevdet(<BEVDepth model>, bev_half="int8") builds it.
design/bevdepth_int8.md.

THE PLAN (`build_plan`) is bevdet_int8's with the single fp16-out `depth_net` layer replaced by the DepthNet's layers, in
the order of DepthNet.forward_hip; everything from the softmax + split on is bevdet_int8's, unchanged:

  quantize      the fp16 image-neck output                                              quantize_rows
  reduce_conv   3 x 3 + ReLU                                        -> dn.r             conv_slice_q_taps
  gates         fp32 from the 27 calibration values (unchanged), both gated copies,
                each requantised with its own scale                 -> dn.depth0, dn.context   lss_camera_gate, se_gate2_nhwc_q
  context_conv  1 x 1, FP16 out into the feature columns of the row buffer              conv_slice_q_taps
  BasicBlock x 3  conv1 + ReLU; conv2 + identity in front of the ReLU -> dn.b{i}.t1, dn.b{i}.out   conv_slice_q_taps(res_first=True)
  aspp1 .. 4    dilation 1 / 6 / 12 / 18 + ReLU into the four slices of ONE int8 buffer -> dn.aspp.cat   conv_slice_q_taps(dilation=)
  pooled branch global average of dn.b2.out (exact integer sums) -> fp16; the two few-row
                GEMMs stay fp16 -> image_bias [n, mid] fp16                             global_avgpool_nhwc_q, dense_auto
  conv1         1 x 1 over 4 mid + the per-image bias + ReLU         -> dn.aspp.out      conv_slice_q_taps(image_bias=)
  DCN layer     (use_dcn=True, depthnet_dcn="int8") the pack's conv_offset as an int8 3 x 3 with
                FP16 out (18 rows padded to 24; the offsets are never quantised) -> dn.dcn.om;
                the grouped deformable convolution, int8 out                 -> dn.dcn    conv_slice_q_taps, deform_conv2d_q_nhwc
  last          1 x 1 mid -> D (padded to 8), FP16 out into the logit columns           conv_slice_q_taps

ONE SCALE PER TENSOR; `dn.aspp.cat` is one group with four writers (the rule of `cat`).  The logits and the feature
columns stay fp16: they are what lss_depth_split_q reads."""
import torch
import torch.nn.functional as F

from . import bevdet_int8 as _bi
from . import functions as _hip_ops
from .bevdepth import ASPP_DILATIONS, MLP_INPUTS
from .bevdet_int8 import CAT, SITE_PREFIX   # noqa: F401
from .functions import dispatch as _dispatch
from .functions import yolox_ops as _Y
from .int8_plan import (Layer, Plan, basic_block_layers, fake_quant, float_operands, load_calibration,   # noqa: F401
                        save_calibration, scales_from, stored)

ASPP_CAT = "dn.aspp.cat"
ROWS = "dn.rows"


# Layer ops beside bevdet_int8's: "gate" (dst and extra[0]: the depth and the context copy), "avgpool" (the pool + the
# two fp16 GEMMs of the pooled branch) and "dcn" (the DCN layer's deformable convolution; res: its fp16 offset rows --
# an int8 layer of a plan with the layer).
DCN, DCN_OFFSET = "dn.dcn", "dn.dcn.offset"


def depthnet_layers(P, dn, x):
    """The DepthNet's layers on the plan P from the int8 tensor `x`; the last one writes "depth_net", the fp16 row buffer."""
    lay = dn.row_layout()
    P.buffers[ROWS] = lay["row_stride"]
    r = P.add(Layer("conv", "dn.reduce_conv", x, "dn.r", act="relu"))
    P.add(Layer("gate", None, r, "dn.depth0", extra=("dn.context",)))
    P.add(Layer("conv", "dn.context_conv", "dn.context", "dn.feat_cols", into=(ROWS, lay["feat_offset"])), "f16")
    d = "dn.depth0"
    for i, blk in enumerate(dn.depth_conv[:3]):
        d = basic_block_layers(P, blk, f"dn.b{i}", d)
    if dn.use_aspp:
        amid = dn.aspp.aspp1.out_channels
        if amid % 16:
            raise NotImplementedError("INT8 DepthNet: aspp_mid_channels must be a multiple of 16 (int8 channel slices)")
        P.buffers[ASPP_CAT] = 4 * amid
        for i, dil in enumerate(ASPP_DILATIONS):
            P.add(Layer("conv", f"dn.aspp{i + 1}", d, f"dn.aspp.b{i}", act="relu", dilation=dil, into=(ASPP_CAT, i * amid)))
        P.readable(ASPP_CAT)
        P.add(Layer("avgpool", None, d, "dn.image_bias"), "f16")
        d = P.add(Layer("conv", "dn.aspp.conv1", ASPP_CAT, "dn.aspp.out", act="relu", image_bias="dn.image_bias"))
    if dn.use_dcn:
        om = P.add(Layer("conv", DCN_OFFSET, d, "dn.dcn.om"), "f16")        # no site: the offsets stay fp16
        d = P.add(Layer("dcn", DCN, d, DCN, res=om))
    return P.add(Layer("conv", "dn.last", d, "depth_net", into=(ROWS, lay["depth_offset"])), "f16")


def build_plan(model):
    """bevdet_int8.build_plan(model) with the DepthNet's layers in place of the `depth_net` layer.  plan.tail: the index
    of the softmax + split, where bevdet_int8's own layers begin."""
    base = _bi.build_plan(model)
    dcn = model.view.depth_net.use_dcn
    P = Plan(base.prefix, base.int8_ops + (("dcn",) if dcn else ()))
    P.buffers.update(base.buffers)
    x = P.add(base.layers[0])
    assert base.layers[0].op == "quantize" and base.layers[1].key == "depth_net" and base.layers[2].op == "split"
    depthnet_layers(P, model.view.depth_net, x)
    P.tail = len(P.layers)
    for l in base.layers[2:]:
        P.add(l, base.tensors[l.dst])
    P.readable(CAT)
    return P


# ---- operands

def _dn_sources(dn):
    """{key: (weight [Cout, Cin, k, k], bias or None)} of the DepthNet's convolutions: conv1 without the pooled branch's
    columns and without its bias (both are in the per-image bias), the last convolution and context_conv zero-padded to the
    widths of the row buffer."""
    lay = dn.row_layout()
    fast = dn.fast_operands()

    def padded(conv, rows):
        w = conv.weight.new_zeros((rows,) + tuple(conv.weight.shape[1:]))
        b = conv.weight.new_zeros((rows,))
        w[:conv.weight.shape[0]] = conv.weight.detach()
        b[:conv.weight.shape[0]] = conv.bias.detach()
        return w, b

    table = {"dn.reduce_conv": (dn.reduce_conv.weight, dn.reduce_conv.bias),
             "dn.context_conv": padded(dn.context_conv, lay["depth_offset"] - lay["feat_offset"]),
             "dn.last": (fast["wd"], fast["bd"])}
    for i, blk in enumerate(dn.depth_conv[:3]):
        table[f"dn.b{i}.conv1"] = (blk.conv1.weight, blk.conv1.bias)
        table[f"dn.b{i}.conv2"] = (blk.conv2.weight, blk.conv2.bias)
    if dn.use_aspp:
        for i, m in enumerate(dn.aspp.branches()):
            table[f"dn.aspp{i + 1}"] = (m.weight, m.bias)
        table["dn.aspp.conv1"] = (fast["conv1_main"], None)
    if dn.use_dcn:
        table[DCN_OFFSET] = (dn.dcn.conv_offset.weight, dn.dcn.conv_offset.bias)
    return table


def _dcn_source(model):
    """{"dn.dcn": (weight [Cout, Cin / groups, 3, 3], None)} of a DepthNet with the DCN layer, else {}.  Per-output-channel
    scales are legal with groups: the epilogue is per output channel."""
    dn = model.view.depth_net
    return {DCN: (dn.dcn.weight, None)} if dn.use_dcn else {}


def _sources(model, plan):
    w1, b1, w2, b2, slices = model.heads_merged()
    dn = _dn_sources(model.view.depth_net)
    table = {}
    for l in plan.layers:
        if l.op != "conv":
            continue
        if l.key in dn:
            table[l.key] = dn[l.key]
        elif l.key.startswith("head."):
            table[l.key] = (w1, b1) if l.key == "head.first" else (w2, b2)
        else:
            c = _bi._conv_of(model, l.key)
            table[l.key] = (c.weight, c.bias)
    return table, model.view.depth_net.row_layout(), slices


def quantize_operands(model, plan):
    """bevdet_int8.quantize_operands for the plan with the DepthNet: per-output-channel int8 taps-major weights, scales and
    fp32 biases (the zero pad rows of the last convolution, of context_conv and of the DCN layer's offset convolution --
    18 rows padded to 24 -- get scale 1 and stay exact zeros); "dn.dcn": the deformable convolution's
    [Cout, 3, 3, Cin / groups]; "fast":
    the DepthNet's fp16 operands -- the packed gate block and the pooled branch's two GEMM weights."""
    src, lay, slices = _sources(model, plan)
    table = {k: _Y.quantize_weight_taps(w, b, multiple=8) for k, (w, b) in src.items()}
    table.update({k: _Y.quantize_weight_taps(w, None) for k, (w, _) in _dcn_source(model).items()})
    table["layout"], table["slices"], table["fast"] = lay, slices, model.view.depth_net.fast_operands()
    return table


def _float_operands(model, plan):
    src, lay, slices = _sources(model, plan)
    src.update(_dcn_source(model))
    return dict(float_operands(src), layout=lay, slices=slices, fast=model.view.depth_net.fast_operands())


# ---- the fp32 statement

def gates_statement(dn, mlp_input):
    """The camera gates [2, n, mid] from the module's weights in float64 (BatchNorm1d, fc1, ReLU, fc2, conv_reduce, ReLU,
    conv_expand, sigmoid), rounded once to fp32: independent of the packed block and of lss_camera_gate."""
    v = mlp_input.reshape(-1, MLP_INPUTS).double()
    bn = dn.bn
    dd = lambda t: t.detach().double()
    v = (v - dd(bn.running_mean)) / torch.sqrt(dd(bn.running_var) + bn.eps) * dd(bn.weight) + dd(bn.bias)
    out = []
    for mlp, se in ((dn.depth_mlp, dn.depth_se), (dn.context_mlp, dn.context_se)):
        h = F.linear(F.relu(F.linear(v, dd(mlp.fc1.weight), dd(mlp.fc1.bias))), dd(mlp.fc2.weight), dd(mlp.fc2.bias))
        h = F.relu(F.linear(h, dd(se.conv_reduce.weight).flatten(1), dd(se.conv_reduce.bias)))
        out.append(torch.sigmoid(F.linear(h, dd(se.conv_expand.weight).flatten(1), dd(se.conv_expand.bias))))
    return torch.stack(out).float()


def emulate(model, plan, x, ranks, table, scales, tensors=None, mlp_input=None):
    """bevdet_int8.emulate with the DepthNet in front: fake quantisation at every int8 tensor (both gate products
    included), the dilated convolutions, the average pool of the dequantised tensor, the pooled branch's two GEMMs and
    the resulting per-image bias each rounded to binary16 where the kernels round, the feature and logit columns rounded
    to binary16.  The DCN layer: the offsets rounded to binary16 (its convolution's fp16 out), the sampled column built
    with deform_conv2d's rules in fp32 and fake-quantised with the SOURCE tensor's scale -- the kernel rounds the column
    to int8 there -- then the grouped product with the dequantised weights.  scales None: nothing is quantised or
    rounded -- the fp32 plain path."""
    live = {} if tensors is None else tensors
    if mlp_input is None:
        raise ValueError("the BEVDepth statement needs mlp_input")
    dn, fast = model.view.depth_net, table["fast"]
    h16 = (lambda v: v.half().float()) if scales is not None else (lambda v: v)
    fq = lambda v, name: stored(plan, name, v, scales, round_f16=True)
    gates = gates_statement(dn, mlp_input.to(x.device))

    def other(l, src, live):
        if l.op == "gate":
            live[l.extra[0]] = fq(src * gates[1][:, :, None, None], l.extra[0])
            return fq(src * gates[0][:, :, None, None], l.dst)
        if l.op == "dcn":
            from .functions.deform_conv import _deform_conv2d_cpu
            w, ws, _ = table[l.key]
            wf = (w.float() * ws[:, None, None, None]).permute(0, 3, 1, 2).contiguous()
            column = None if scales is None else (lambda c: fake_quant(c, scales[plan.site(l.src)]))
            return fq(_deform_conv2d_cpu(src, live[l.res][:, :18], wf, 1, 1, 1, dn.dcn.groups, 1, column=column), l.dst)
        assert l.op == "avgpool"
        pooled = h16(src.mean(dim=(2, 3)))
        a = dn.aspp
        g = h16(F.relu(F.linear(pooled, fast["pool_w"].float(), a.global_avg_pool.bias.detach().float())))
        return h16(F.linear(g, fast["conv1_pool"].float(), a.conv1.bias.detach().float()))

    _bi.emulate(model, plan, x, ranks, table, scales, live, layers=plan.layers[:plan.tail], other=other)
    live["depth_net"] = live[ROWS]
    return _bi.emulate(model, plan, x, ranks, table, scales, live, layers=plan.layers[plan.tail:])


# ---- the model

class Int8BEVDepth(_bi.Int8BEVDet):
    """bevdet_int8.Int8BEVDet for a BEVDepth model: `forward` takes mlp_input behind the ranks, `forward_calibrated` /
    `bev_half_calibrated` split the [N * 51 + 9] calibration row(s) with view.split_calibration.  BEVDetRunner captures
    and replays it unchanged."""

    _plan_of = staticmethod(build_plan)
    _quantize_of = staticmethod(quantize_operands)
    _floats = staticmethod(_float_operands)

    def _stamped(self):
        return super()._stamped() + list(self.fp.view.depth_net.buffers())

    def run(self, x, pool, table, ops, tensors=None, layers=None, mlp_input=None):
        live = {} if tensors is None else tensors
        if mlp_input is None:
            raise ValueError("Int8BEVDepth: the DepthNet needs mlp_input")
        plan, dn, fast = self.plan, self.fp.view.depth_net, table["fast"]
        gates = ops.lss_camera_gate(mlp_input.to(x.device, torch.float32), fast["gate"], dn.mid_channels)

        def other(l, src, live, s_out):
            if l.op == "gate":
                y, live[l.extra[0]] = ops.se_gate2_nhwc_q(src, self.scale(l.src), gates, s_out, self.scale(l.extra[0]))
                return y
            if l.op == "dcn":
                w, ws, _ = table[l.key]
                return ops.deform_conv2d_q_nhwc(src, self.scale(l.src), live[l.res], w, ws, None, dn.dcn.groups, None, s_out)
            assert l.op == "avgpool"
            a = dn.aspp
            pooled = ops.global_avgpool_nhwc_q(src, self.scale(l.src))
            g = ops.dense_auto(pooled, fast["pool_w"], a.global_avg_pool.bias, None, True)
            return ops.dense_auto(g, fast["conv1_pool"], a.conv1.bias, None, False)

        super().run(x, pool, table, ops, live, layers=plan.layers[:plan.tail], other=other)
        live["depth_net"] = live[ROWS]
        return super().run(x, pool, table, ops, live, layers=plan.layers[plan.tail:] if layers is None else layers)

    def depth_and_features(self, x, mlp_input, table, ops):
        """The plan up to and including the softmax + split: -> (depth int8 [n, D, H, W], features int8 [n, H, W, C])."""
        live = {}
        self.run(x, None, table, ops, live, layers=self.plan.layers[self.plan.tail:self.plan.tail + 1], mlp_input=mlp_input)
        return live["depth"], live["feat"]

    @torch.no_grad()
    def forward(self, image, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, mlp_input=None):
        table = self._ready(image)
        ops = self.bev_ops
        h, w = int(self.view.grid_size[1]), int(self.view.grid_size[0])
        pool = lambda d, f, s: ops.bev_pool_v2_int8(d, f, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                                    interval_lengths, *s, h, w)
        if mlp_input is None:
            raise ValueError("Int8BEVDepth.forward needs mlp_input (view.get_mlp_input of the frame)")
        with _dispatch.using(rule=True):
            return self._heads(self.run(self._features(image), pool, table, ops,
                                        mlp_input=mlp_input.reshape(-1, MLP_INPUTS)), table)

    @torch.no_grad()
    def bev_half_calibrated(self, x, calib):
        """bevdet_int8's, on the [N * 51 + 9] row(s) of LSSViewTransformerBEVDepth.calibration_matrices: the first part
        feeds the index build, the [B N, 27] rest the camera gates."""
        table = self._ready(x)
        ops = self.bev_ops
        geo, mlp = self.view.split_calibration(calib)
        if mlp.shape[0] != x.shape[0]:
            raise ValueError(f"calib {tuple(calib.shape)} does not describe the {x.shape[0]} camera images of x")
        rb, rd, rf, ist, il, counts = self.view.prepare_calibrated(calib)
        h, w = int(self.view.grid_size[1]), int(self.view.grid_size[0])
        kw = dict(batch=calib.shape[0]) if calib.dim() == 2 else {}
        pool = lambda d, f, s: ops.bev_pool_v2_indirect(d, f, rd, rf, rb, ist, il, counts, h, w, scales=s, **kw)
        with _dispatch.using(rule=True):
            return self._heads(self.run(x, pool, table, ops, mlp_input=mlp), table)

    @torch.no_grad()
    def fake_quant_reference(self, x, ranks, mlp_input=None, quantize=True, tensors=None):
        """bevdet_int8's statement with the DepthNet in front (mlp_input [n, 27] fp32).  -> the six head outputs, fp32."""
        if quantize:
            table, scales = self.operands(), self.scales
        else:
            table, scales = self._floats(self.fp, self.plan), None
        return self._heads(emulate(self.fp, self.plan, x, ranks, table, scales, tensors, mlp_input), table)


# ---- calibration

def calibrate_frame(fp, x, rest, cal, ops=None):
    """One calibration frame of a BEVDepth model from its fp16 image features x: rest = (ranks_bev, ranks_depth,
    ranks_feat, interval_starts, interval_lengths, mlp_input).  The DepthNet runs layer by layer on the fp16 fast path's
    kernels (DepthNet.forward_hip's calls) and every tensor the plan quantises is collected under its site, the ASPP
    buffer as ONE tensor, the DCN layer's output behind its two fp16 launches; from the split on, bevdet_int8.calibrate_behind_split."""
    ops = ops if ops is not None else _hip_ops
    ranks, mlp_input = tuple(rest[:5]), rest[5]
    view = fp.view
    dn = view.depth_net
    site = lambda name, t: cal.collect(SITE_PREFIX + name, t)
    with torch.no_grad(), _dispatch.using(rule=True):
        x = x.contiguous(memory_format=torch.channels_last)
        site("x", x)
        P = dn.fast_operands()
        lay, mid = P["layout"], dn.mid_channels
        n, _, H, W = x.shape
        gates = ops.lss_camera_gate(mlp_input.reshape(-1, MLP_INPUTS).to(x.device, torch.float32), P["gate"], mid)
        r = ops.conv_nhwc(x, dn.reduce_conv.weight, dn.reduce_conv.bias, True)
        site("dn.r", r)
        depth, context = ops.se_gate2_nhwc(r, gates)
        site("dn.depth0", depth)
        site("dn.context", context)
        rows = _Y.nhwc_empty(n, lay["row_stride"], H, W, x.device)
        o = lay["depth_offset"]
        ops.conv_slice_nhwc(context, dn.context_conv.weight, dn.context_conv.bias, "none", out=rows[:, :o])
        for i, m in enumerate(dn.depth_conv[:3]):
            t = ops.conv_nhwc(depth, m.conv1.weight, m.conv1.bias, True)
            site(f"dn.b{i}.t1", t)
            depth = ops.conv_nhwc(t, m.conv2.weight, m.conv2.bias, True, depth)
            site(f"dn.b{i}.out", depth)
        if dn.use_aspp:
            a = dn.aspp
            amid = a.aspp1.out_channels
            cat = _Y.nhwc_empty(n, 4 * amid, H, W, x.device)
            for i, (m, d) in enumerate(zip(a.branches(), ASPP_DILATIONS)):
                ops.conv_slice_nhwc(depth, m.weight, m.bias, "relu", out=cat[:, i * amid:(i + 1) * amid], dilation=d)
            site(ASPP_CAT, cat)
            pooled = ops.global_avgpool_nhwc(depth)
            g = ops.dense_auto(pooled, P["pool_w"], a.global_avg_pool.bias, None, True)
            image_bias = ops.dense_auto(g, P["conv1_pool"], a.conv1.bias, None, False)
            depth = ops.conv_slice_nhwc(cat, P["conv1_main"], None, "relu", image_bias=image_bias)
            site("dn.aspp.out", depth)
        if dn.use_dcn:
            depth = dn.dcn.forward_hip(depth, ops)                  # the two fp16 launches
            site(DCN, depth)
        ops.conv_slice_nhwc(depth, P["wd"], P["bd"], "none", out=rows[:, o:o + lay["depth_padded"]])
        d, f = ops.lss_depth_split(rows.permute(0, 2, 3, 1).reshape(n * H * W, lay["row_stride"]), n, view.D,
                                   view.out_channels, lay["depth_offset"], lay["feat_offset"], spatial=(H, W))
    _bi.calibrate_behind_split(fp, d, f, ranks, cal, ops)
