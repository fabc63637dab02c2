"""BEVDepth's view transformer: the camera-aware DepthNet with ASPP in front of the LSS pooling
(third_party/bev_mmdet3d/models/necks/view_transformer.py: DepthNet :534-712, ASPP :417-481, Mlp :492, SELayer :519,
LSSViewTransformerBEVDepth :781-895), re-hosted without mmcv / mmdet with the reference's attribute names.  Frozen
BatchNorm2d is folded into the convolution in front of it, as everywhere in bevdet.py (checkpoint.py folds while
loading); Dropout is the identity.  design/bevdepth.md has the operation orders and what was left out.

Two data paths through the same weights:
  * plain (`DepthNet.forward`): the reference's op sequence in torch -- F.conv2d(dilation=), adaptive_avg_pool2d,
    interpolate, cat, x * gate -- on any device and dtype;
  * fast (`DepthNet.forward_hip`): channels-last fp16 CUDA tensors with bev_half="hip".  The camera gates in one
    launch from the fp32 calibration values (functions.lss_camera_gate), reduce_conv and the three BasicBlocks on the
    tiled convolution, both gated copies in one launch (se_gate2_nhwc), the four ASPP branches into four slices of ONE
    buffer (conv_slice_nhwc, three of them dilated), ASPP's pooled branch as a per-image bias of conv1
    (global_avgpool_nhwc + two few-row GEMMs: a bilinear up-sampling of a 1 x 1 map is a constant), context_conv and
    the last 1 x 1 into the feature / depth-logit columns of the row buffer lss_depth_split reads.  No library
    convolution, pooling, interpolation, torch.cat or layout copy.

DepthNet(use_dcn=True) puts the reference's DCN layer (mmcv's DCNv1 pack, groups = 4; `DeformConv2dPack`) between the
ASPP and the last convolution: functions.deform_conv2d on the plain path, conv_offset_nhwc + deform_conv2d_nhwc (two
launches) on the fast one.  design/bevdepth_dcn.md.

DepthNet(stereo=True, bias=...) is BEVStereo's depth net: the temporal-stereo cost volume of the previous frame's
stride-4 features (functions.stereo: one launch on the fast path), `cost_volumn_net` (two stride-2 convolutions, no
ReLU) and a first BasicBlock that reads the gated depth copy and the reduced cost volume side by side -- two channel
slices of ONE buffer on the fast path, no torch.cat.  LSSViewTransformerBEVStereo carries `cv_frustum`.
design/bevstereo.md."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .bevdet import BasicBlock, LSSViewTransformer, _rule_dispatch
from .functions.multi_scale_deformable_attn import _TensorCache
from .functions.stereo import CV_DOWNSAMPLE

MLP_INPUTS = 27
ASPP_DILATIONS = (1, 6, 12, 18)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, out_features):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(in_features, hidden_features), nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(F.relu(self.fc1(x)))


class SELayer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv_reduce, self.conv_expand = nn.Conv2d(channels, channels, 1), nn.Conv2d(channels, channels, 1)

    def gate(self, x_se):
        return torch.sigmoid(self.conv_expand(F.relu(self.conv_reduce(x_se))))

    def forward(self, x, x_se):
        return x * self.gate(x_se)


class ASPP(nn.Module):
    """aspp1 .. aspp4, global_avg_pool and conv1 each stand for the reference's convolution WITH its BatchNorm (and
    ReLU): _ASPPModule.atrous_conv + bn, global_avg_pool[1] + [2], conv1 + bn1."""

    def __init__(self, inplanes, mid_channels):
        super().__init__()
        d = ASPP_DILATIONS
        self.aspp1 = nn.Conv2d(inplanes, mid_channels, 1)
        self.aspp2 = nn.Conv2d(inplanes, mid_channels, 3, 1, d[1], d[1])
        self.aspp3 = nn.Conv2d(inplanes, mid_channels, 3, 1, d[2], d[2])
        self.aspp4 = nn.Conv2d(inplanes, mid_channels, 3, 1, d[3], d[3])
        self.global_avg_pool = nn.Conv2d(inplanes, mid_channels, 1)
        self.conv1 = nn.Conv2d(5 * mid_channels, inplanes, 1)

    def branches(self):
        return (self.aspp1, self.aspp2, self.aspp3, self.aspp4)

    def forward(self, x):
        xs = [F.relu(F.conv2d(x, m.weight, m.bias, 1, m.padding, m.dilation)) for m in self.branches()]
        x5 = F.relu(self.global_avg_pool(F.adaptive_avg_pool2d(x, (1, 1))))
        xs.append(F.interpolate(x5, size=x.shape[2:], mode="bilinear", align_corners=True))
        return F.relu(self.conv1(torch.cat(xs, dim=1)))


def fold_pooled_branch(aspp, pooled):
    """ASPP's fifth branch as a per-image bias of conv1: pooled [n, inplanes] (the global average) ->
    conv1.weight[:, 4 mid:] @ relu(global_avg_pool(pooled)) + conv1.bias, [n, inplanes].  In the tensors' dtype; the
    statement the fast path's two few-row GEMMs evaluate."""
    mid = aspp.aspp1.out_channels
    g = F.relu(F.linear(pooled, aspp.global_avg_pool.weight.flatten(1), aspp.global_avg_pool.bias))
    return F.linear(g, aspp.conv1.weight.flatten(1)[:, 4 * mid:], aspp.conv1.bias)


STEREO_WIDTH_MULTIPLE = 32               # csrc/conv_slice.hip: Cin % 32 == 0 for the layers that read mid + Dpad columns
DCN_GROUPS = 4
DCN_WIDTH_MULTIPLE = 32 * DCN_GROUPS     # csrc/deform_conv.hip: (channels / groups) % 32 == 0


class DeformConv2dPack(nn.Module):
    """mmcv's `DCN` (DeformConv2dPack, DCNv1) as DepthNet builds it: `conv_offset` (3 x 3, 18 channels, zero-initialised:
    an untrained pack is a plain grouped convolution) and an UNMODULATED deformable 3 x 3 convolution with groups = 4,
    deform_groups = 1, no bias; no BatchNorm or ReLU behind it.  mmcv's attribute names."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, dilation=1, groups=DCN_GROUPS,
                 deform_groups=1):
        super().__init__()
        if (kernel_size, stride, padding, dilation, deform_groups) != (3, 1, 1, 1, 1):
            raise NotImplementedError("DeformConv2dPack: 3 x 3 / stride 1 / padding 1 / dilation 1 / one deform group only")
        if in_channels % groups or out_channels % groups:
            raise ValueError("DeformConv2dPack: channels must divide into the groups")
        self.in_channels, self.out_channels, self.groups, self.deform_groups = in_channels, out_channels, groups, deform_groups
        self.kernel_size, self.stride, self.padding, self.dilation = (3, 3), (1, 1), (1, 1), (1, 1)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, 3, 3))
        stdv = 1.0 / (in_channels * 9) ** 0.5                       # (mmcv DeformConv2d.reset_parameters)
        nn.init.uniform_(self.weight, -stdv, stdv)
        self.conv_offset = nn.Conv2d(in_channels, deform_groups * 18, 3, 1, 1)
        nn.init.zeros_(self.conv_offset.weight)
        nn.init.zeros_(self.conv_offset.bias)

    def forward(self, x):
        from .functions.deform_conv import deform_conv2d
        offset = self.conv_offset(x)
        return deform_conv2d(x, offset, self.weight, 1, 1, 1, self.groups, self.deform_groups)

    def prepack(self):
        """Both packed operands of `forward_hip` (never under capture)."""
        from .functions.deform_conv import deform_conv_packed_weight
        from .functions.modulated_deformable_conv2d import conv_offset_nhwc
        w = self.conv_offset.weight
        deform_conv_packed_weight(self.weight)
        # an empty batch: the wrapper packs the offset weight and pads the bias, and launches nothing
        conv_offset_nhwc(w.new_empty((0, self.in_channels, 1, 1)).contiguous(memory_format=torch.channels_last), w,
                         self.conv_offset.bias)

    def forward_hip(self, x, ops):
        """Two launches: the offset convolution ([n, 32, H, W] channels-last, offsets in channels 0 .. 18) and the
        deformable convolution that reads its rows in place."""
        om = ops.conv_offset_nhwc(x, self.conv_offset.weight, self.conv_offset.bias)
        return ops.deform_conv2d_nhwc(x, om, self.weight, None, self.groups)


class DepthNet(nn.Module):
    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, use_aspp=True, aspp_mid_channels=-1,
                 use_dcn=False, stereo=False, bias=0.0):
        super().__init__()
        if use_dcn and mid_channels % DCN_WIDTH_MULTIPLE:
            raise NotImplementedError(f"DepthNet(use_dcn=True): the DCN layer (mmcv DCN: DCNv1, groups={DCN_GROUPS}) is built "
                                      f"for mid_channels % {DCN_WIDTH_MULTIPLE} == 0 only (mid_channels / {DCN_GROUPS} a multiple "
                                      f"of 32, on both data paths); got {mid_channels} (design/bevdepth_dcn.md)")
        if stereo and mid_channels % STEREO_WIDTH_MULTIPLE:
            raise NotImplementedError(f"DepthNet(stereo=True): the BEVStereo cost volume is built for mid_channels % "
                                      f"{STEREO_WIDTH_MULTIPLE} == 0 only (the first block reads mid + Dpad columns of one "
                                      f"buffer, on both data paths); got {mid_channels} (design/bevstereo.md)")
        self.mid_channels, self.context_channels, self.depth_channels = mid_channels, context_channels, depth_channels
        self.stereo, self.bias = bool(stereo), float(bias)
        self.reduce_conv = nn.Conv2d(in_channels, mid_channels, 3, 1, 1)
        self.context_conv = nn.Conv2d(mid_channels, context_channels, 1)
        self.bn = nn.BatchNorm1d(MLP_INPUTS)
        self.depth_mlp, self.depth_se = Mlp(MLP_INPUTS, mid_channels, mid_channels), SELayer(mid_channels)
        self.context_mlp, self.context_se = Mlp(MLP_INPUTS, mid_channels, mid_channels), SELayer(mid_channels)
        layers = [BasicBlock(mid_channels, mid_channels, 1, False) for _ in range(3)]
        if self.stereo:
            # each stands for the reference's convolution WITH its BatchNorm; no ReLU between or behind them
            self.cost_volumn_net = nn.ModuleList(nn.Conv2d(depth_channels, depth_channels, 3, 2, 1) for _ in range(2))
            layers[0] = BasicBlock(mid_channels + depth_channels, mid_channels, 1, False)
            layers[0].downsample = nn.Conv2d(mid_channels + depth_channels, mid_channels, 1)      # plain, biased, no BatchNorm
        if use_aspp:
            layers.append(ASPP(mid_channels, mid_channels if aspp_mid_channels < 0 else aspp_mid_channels))
        if use_dcn:
            layers.append(DeformConv2dPack(mid_channels, mid_channels))
        layers.append(nn.Conv2d(mid_channels, depth_channels, 1))
        self.depth_conv = nn.ModuleList(layers)          # (the reference's nn.Sequential: the same indices)
        self.use_aspp, self.use_dcn = use_aspp, bool(use_dcn)

    @property
    def aspp(self):
        return self.depth_conv[3] if self.use_aspp else None

    @property
    def dcn(self):
        return self.depth_conv[-2] if self.use_dcn else None

    # ---- plain: DepthNet.forward :680-712
    def gates(self, mlp_input):
        """(depth gate, context gate), each [n, mid, 1, 1], in mlp_input's dtype."""
        v = self.bn(mlp_input.reshape(-1, mlp_input.shape[-1]))
        return (self.depth_se.gate(self.depth_mlp(v)[..., None, None]),
                self.context_se.gate(self.context_mlp(v)[..., None, None]))

    def cost_volume(self, stereo_metas, like):
        """calculate_cost_volumn :651-678 (or the first frame's zeros :690-702) from the reference's `stereo_metas`:
        -> [B N, D, Hc, Wc] in `like`'s dtype on its device, by the torch statements of functions.stereo."""
        from .functions import stereo as S
        prev, curr = stereo_metas["cv_feat_list"]
        if prev is None:
            n, _, H, W = like.shape
            scale = float(stereo_metas["downsample"]) / stereo_metas["cv_downsample"]
            return like.new_zeros((n, self.depth_channels, int(H * scale), int(W * scale)))
        D, H, W, _ = stereo_metas["frustum"].shape
        consts = S.stereo_calibration(stereo_metas["k2s_sensor"], stereo_metas["intrins"], stereo_metas["post_rots"],
                                      stereo_metas["post_trans"]).to(curr.device)
        tables = S.stereo_frustum_tables(stereo_metas["frustum"].to(curr.device))
        grid = S.stereo_grid_plain(consts, tables)
        n = consts.shape[0]
        return S.stereo_cost_volume_plain(prev.reshape(n, -1, H, W), curr.reshape(n, -1, H, W), grid, self.bias)

    def forward(self, x, mlp_input, stereo_metas=None):
        if self.stereo != (stereo_metas is not None):
            raise ValueError("DepthNet: stereo_metas goes with stereo=True, and only with it")
        gate_d, gate_c = self.gates(mlp_input.to(x.dtype))
        x = F.relu(self.reduce_conv(x))
        context = self.context_conv(x * gate_c)
        depth = x * gate_d
        if self.stereo:
            with torch.no_grad():
                cv = self.cost_volume(stereo_metas, x).to(x.dtype)
            for m in self.cost_volumn_net:
                cv = m(cv)
            depth = torch.cat([depth, cv], dim=1)
        for m in self.depth_conv:
            if isinstance(m, BasicBlock):
                idt = depth if m.downsample is None else m.downsample(depth)
                depth = F.relu(m.conv2(F.relu(m.conv1(depth))) + idt)
            else:
                depth = m(depth)
        return torch.cat([depth, context], dim=1)

    # ---- fast
    def row_layout(self):
        """The row buffer lss_depth_split reads: features in columns 0 .. C, the depth logits from C rounded up to 8,
        D padded to a multiple of 8 with zero weight rows (exact zero columns): `merge_depth_net`'s layout."""
        off = (self.context_channels + 7) // 8 * 8
        dpad = (self.depth_channels + 7) // 8 * 8
        return dict(row_stride=off + dpad, feat_offset=0, depth_offset=off, depth_padded=dpad)

    def fast_operands(self, build=True):
        """The derived operands of `forward_hip` on the weights' device: the packed gate block, conv1 split into its
        four-branch part and the pooled branch's columns, the padded last convolution, and the taps-major weights of
        every conv_slice layer.  Cached on the stamps of every parameter and buffer, rebuilt when one changes.
        build=False: None when missing or stale.  Never built under capture (RuntimeError)."""
        from .functions import lss_depthnet as G
        from .functions import yolox_ops as Y
        stamp = tuple(_TensorCache._stamp(t) for t in list(self.parameters()) + list(self.buffers()))
        hit = self.__dict__.get("_fast_operands")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if not build:
            return None
        w = self.reduce_conv.weight
        if w.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("DepthNet: the packed operands are missing or stale and the stream is capturing; call "
                               "BEVDet.prepare_bev_half() (or the model once, eagerly) before the capture")
        lay, mid = self.row_layout(), self.mid_channels
        last = self.depth_conv[-1]
        wd = w.new_zeros((lay["depth_padded"], mid, 1, 1))
        wd[:self.depth_channels] = last.weight.detach()
        bd = w.new_zeros((lay["depth_padded"],))
        bd[:self.depth_channels] = last.bias.detach()
        ops = dict(gate=G.camera_gate_packed(self.bn, self.depth_mlp, self.depth_se, self.context_mlp, self.context_se),
                   wd=wd, bd=bd, layout=lay)
        slices = [(self.context_conv.weight, mid, lay["depth_offset"]), (wd, mid, lay["depth_padded"])]
        if self.use_aspp:
            a = self.aspp
            amid = a.aspp1.out_channels
            if amid % 8:
                raise NotImplementedError("DepthNet fast path: aspp_mid_channels must be a multiple of 8")
            ops["conv1_main"] = a.conv1.weight.detach()[:, :4 * amid].contiguous()
            ops["conv1_pool"] = a.conv1.weight.detach().flatten(1)[:, 4 * amid:].contiguous()
            ops["pool_w"] = a.global_avg_pool.weight.detach().flatten(1).contiguous()
            slices += [(m.weight, mid, amid) for m in a.branches()] + [(ops["conv1_main"], 4 * amid, mid)]
        if self.stereo:
            dp = self.stereo_padded()
            ops["cv_bias"] = []
            for m in self.cost_volumn_net:
                b = w.new_zeros((dp,))
                b[:self.depth_channels] = m.bias.detach()
                ops["cv_bias"].append(b)
                slices.append((m.weight, dp, dp))
            blk = self.depth_conv[0]
            slices += [(blk.conv1.weight, mid + dp, mid), (blk.downsample.weight, mid + dp, mid)]
        if w.is_cuda and w.dtype == torch.float16:
            for t, cin, cout in slices:
                Y.conv_slice_packed_weight(t, cin, cout)
            if self.use_dcn:
                self.dcn.prepack()
        self.__dict__["_fast_operands"] = (stamp, ops)
        return ops

    def stereo_padded(self):
        """Dpad: D rounded up so that mid + Dpad is a multiple of 32 (conv_slice's Cin % 32 rule; mid % 32 == 0).  The
        cost volume, `cost_volumn_net` and the first block's input run at this width; the pad channels carry zero
        weight rows and columns and stay exact zeros."""
        return (self.depth_channels + 31) // 32 * 32

    def forward_hip(self, x, mlp_input, ops, stereo=None):
        """x [n, Cin, H, W] channels-last fp16, mlp_input [n, 27] fp32 on x's device -> (rows [n H W, row_stride] fp16,
        layout): the operand of lss_depth_split.  stereo (DepthNet(stereo=True)): (prev or None, curr, consts, tables)
        -- the stride-4 features [n, C, Hc, Wc] channels-last fp16, `stereo_calibration`'s block and the frustum
        tables, both on x's device."""
        from .functions.yolox_ops import nhwc_empty
        P = self.fast_operands(build=False)
        if P is None:
            P = self.fast_operands()
        lay, mid = P["layout"], self.mid_channels
        n, _, H, W = x.shape
        gates = ops.lss_camera_gate(mlp_input, P["gate"], mid)                                    # 1 launch
        r = ops.conv_nhwc(x, self.reduce_conv.weight, self.reduce_conv.bias, True)
        if self.stereo != (stereo is not None):
            raise ValueError("DepthNet.forward_hip: `stereo` goes with stereo=True, and only with it")
        if self.stereo:
            dp = self.stereo_padded()
            both = nhwc_empty(n, mid + dp, H, W, x.device)           # gated depth copy | reduced cost volume | zeros
            _, context = ops.se_gate2_nhwc(r, gates, out_a=both[:, :mid])                         # 1 launch
            prev, curr, consts, tables = stereo
            cv = ops.stereo_cost_volume(prev, curr, consts, self.depth_channels, self.bias, frustum_tables=tables,
                                        dpad=dp)                                                  # 1 launch
            c0, c1 = self.cost_volumn_net
            cv = ops.conv_slice_nhwc(cv, c0.weight, P["cv_bias"][0], "none", stride=2,
                                     out=nhwc_empty(n, dp, (cv.shape[2] + 1) // 2, (cv.shape[3] + 1) // 2, x.device))
            if ((cv.shape[2] + 1) // 2, (cv.shape[3] + 1) // 2) != (H, W):
                raise ValueError("DepthNet.forward_hip: the stereo map is four times the depth map's size")
            ops.conv_slice_nhwc(cv, c1.weight, P["cv_bias"][1], "none", stride=2, out=both[:, mid:])
            depth = both
        else:
            depth, context = ops.se_gate2_nhwc(r, gates)                                          # 1 launch
        rows = nhwc_empty(n, lay["row_stride"], H, W, x.device)
        o = lay["depth_offset"]             # (the feature columns up to here: zero weight rows behind channel C)
        ops.conv_slice_nhwc(context, self.context_conv.weight, self.context_conv.bias, "none", out=rows[:, :o])
        for m in self.depth_conv[:3]:
            if m.downsample is None:
                t = ops.conv_nhwc(depth, m.conv1.weight, m.conv1.bias, True)
                idt = depth
            else:                           # the stereo block: both convolutions read all mid + Dpad columns
                t = ops.conv_slice_nhwc(depth, m.conv1.weight, m.conv1.bias, "relu")
                idt = ops.conv_slice_nhwc(depth, m.downsample.weight, m.downsample.bias, "none")
            depth = ops.conv_nhwc(t, m.conv2.weight, m.conv2.bias, True, idt)
        if self.use_aspp:
            a = self.aspp
            amid = a.aspp1.out_channels
            cat = nhwc_empty(n, 4 * amid, H, W, x.device)
            for i, (m, d) in enumerate(zip(a.branches(), ASPP_DILATIONS)):
                ops.conv_slice_nhwc(depth, m.weight, m.bias, "relu", out=cat[:, i * amid:(i + 1) * amid], dilation=d)
            pooled = ops.global_avgpool_nhwc(depth)                                               # [n, mid]
            g = ops.dense_auto(pooled, P["pool_w"], a.global_avg_pool.bias, None, True)           # [n, amid]
            image_bias = ops.dense_auto(g, P["conv1_pool"], a.conv1.bias, None, False)            # [n, mid]
            depth = ops.conv_slice_nhwc(cat, P["conv1_main"], None, "relu", image_bias=image_bias)
        if self.use_dcn:
            depth = self.dcn.forward_hip(depth, ops)                                              # 2 launches
        ops.conv_slice_nhwc(depth, P["wd"], P["bd"], "none", out=rows[:, o:o + lay["depth_padded"]])
        return rows.permute(0, 2, 3, 1).reshape(n * H * W, lay["row_stride"]), lay


class LSSViewTransformerBEVDepth(LSSViewTransformer):
    """LSSViewTransformer with the DepthNet as depth_net.  The calibration row carries the DepthNet's inputs behind
    the parent's: `calibration_matrices` -> [N * 24 + 9 | N * 27] = [N * 51 + 9] floats (batched: [B, N * 51 + 9]), so
    BEVDetRunner still uploads ONE row per frame; the transformer splits it."""

    def __init__(self, grid_config, input_size, downsample, in_channels, out_channels, ops=None, seed=0, bev_half=None,
                 depthnet_cfg=None):
        super().__init__(grid_config, input_size, downsample, in_channels, out_channels, ops=ops, seed=seed,
                         bev_half=bev_half)
        self.depth_net = DepthNet(in_channels, in_channels, out_channels, self.D, **(depthnet_cfg or {}))

    # ---- view_transformer.py:793-818 (pure gathers)
    def get_mlp_input(self, sensor2ego, ego2global, intrin, post_rot, post_tran, bda):
        B, N, _, _ = sensor2ego.shape
        bda = bda.view(B, 1, 3, 3).repeat(1, N, 1, 1)
        mlp_input = torch.stack([intrin[:, :, 0, 0], intrin[:, :, 1, 1], intrin[:, :, 0, 2], intrin[:, :, 1, 2],
                                 post_rot[:, :, 0, 0], post_rot[:, :, 0, 1], post_tran[:, :, 0], post_rot[:, :, 1, 0],
                                 post_rot[:, :, 1, 1], post_tran[:, :, 1], bda[:, :, 0, 0], bda[:, :, 0, 1],
                                 bda[:, :, 1, 0], bda[:, :, 1, 1], bda[:, :, 2, 2]], dim=-1)
        sensor2ego = sensor2ego[:, :, :3, :].reshape(B, N, -1)
        return torch.cat([mlp_input, sensor2ego], dim=-1)

    def calibration_matrices(self, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        geo = super().calibration_matrices(sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda)
        s2e, K, pr, pt, b = (t.detach().to("cpu", torch.float32) for t in (sensor2ego, cam2imgs, post_rots, post_trans, bda))
        mlp = self.get_mlp_input(s2e, None, K, pr, pt, b)
        return torch.cat((geo, mlp.reshape(-1))).contiguous()

    @staticmethod
    def split_calibration(calib):
        """The packed row(s) -> (the parent's [N * 24 + 9] part, the MLP inputs [B * N, 27]).  1-D: two views.  2-D: the
        index build needs dense rows and the gate a dense [B * N, 27] table: two small device copies."""
        L = calib.shape[-1]
        if (L - 9) % 51:
            raise ValueError(f"a BEVDepth calibration row holds N * 51 + 9 floats, got {L}")
        cut = (L - 9) // 51 * 24 + 9
        if calib.dim() == 1:
            return calib[:cut], calib[cut:].view(-1, MLP_INPUTS)
        return calib[:, :cut].contiguous(), calib[:, cut:].reshape(-1, MLP_INPUTS)

    def lidar_coor_plain(self, calib):
        return super().lidar_coor_plain(self.split_calibration(calib)[0])

    def prepare_calibrated(self, calib, padded=True):
        return super().prepare_calibrated(self.split_calibration(calib)[0], padded=padded)

    # ---- the fast path's switches: the parent's names, so that BEVDet.prepare_bev_half / _bev_half_ready serve both
    def _hip_on(self, x):
        need = ("lss_depth_split", "dense_auto", "conv_nhwc", "conv_slice_nhwc", "lss_camera_gate", "se_gate2_nhwc",
                "global_avgpool_nhwc")
        if self.depth_net.use_dcn:
            need += ("conv_offset_nhwc", "deform_conv2d_nhwc")
        if self.depth_net.stereo:
            need += ("stereo_cost_volume",)
        return self.bev_half == "hip" and x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 \
            and x.is_contiguous(memory_format=torch.channels_last) and all(hasattr(self.ops, f) for f in need)

    def depth_net_merged(self, build=True):
        return self.depth_net.fast_operands(build=build)

    def _stereo_operands(self, stereo_metas, x):
        """None for a transformer without the stereo branch."""
        if stereo_metas is not None:
            raise ValueError(f"{type(self).__name__} takes no stereo_metas (LSSViewTransformerBEVStereo does)")
        return None

    def _depth_feat(self, x, mlp_input, stereo_metas=None):
        """-> (depth [n, D, H, W] softmax, feat [n, H, W, C], fast?)"""
        n, _, h, w = x.shape
        if self._stereo_fast(stereo_metas) and self._hip_on(x):
            if self.depth_net.fast_operands(build=False) is None and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LSSViewTransformerBEVDepth: the DepthNet's packed operands are missing or stale and "
                                   "the stream is capturing; call BEVDet.prepare_bev_half() first")
            stereo = self._stereo_operands(stereo_metas, x)
            with _rule_dispatch():
                rows, lay = self.depth_net.forward_hip(x, mlp_input.to(x.device, torch.float32), self.ops,
                                                       **({} if stereo is None else dict(stereo=stereo)))
            depth, feat = self.ops.lss_depth_split(rows, n, self.D, self.out_channels, lay["depth_offset"],
                                                   lay["feat_offset"], spatial=(h, w))
            return depth, feat, True
        y = self.depth_net(x, mlp_input.to(x.device), **({} if stereo_metas is None else dict(stereo_metas=stereo_metas)))
        depth = y[:, :self.D].softmax(dim=1)
        feat = y[:, self.D:self.D + self.out_channels].permute(0, 2, 3, 1)
        return depth.contiguous(), feat.contiguous(), False

    def _stereo_fast(self, stereo_metas):
        return True

    @torch.no_grad()
    def view_transform_calibrated(self, x, calib, stereo_metas=None):
        geo, mlp = self.split_calibration(calib)
        if mlp.shape[0] != x.shape[0]:
            raise ValueError(f"calib {tuple(calib.shape)} does not describe the {x.shape[0]} camera images of x")
        rb, rd, rf, ist, il, counts = super().prepare_calibrated(geo)
        bev_h, bev_w = int(self.grid_size[1]), int(self.grid_size[0])
        kw = dict(batch=calib.shape[0]) if calib.dim() == 2 else {}
        depth, feat, fast = self._depth_feat(x, mlp, stereo_metas)
        out = self.ops.bev_pool_v2_indirect(depth, feat, rd, rf, rb, ist, il, counts, bev_h, bev_w, **kw).permute(0, 3, 1, 2)
        return out if fast else out.contiguous()

    @torch.no_grad()
    def view_transform(self, x, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, mlp_input=None,
                       stereo_metas=None):
        if mlp_input is None:
            raise ValueError("LSSViewTransformerBEVDepth.view_transform needs mlp_input (get_mlp_input of the frame)")
        depth, feat, fast = self._depth_feat(x, mlp_input.reshape(-1, MLP_INPUTS), stereo_metas)
        out = self.ops.bev_pool_v2_2(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths,
                                     int(self.grid_size[1]), int(self.grid_size[0])).permute(0, 3, 1, 2)
        return out if fast else out.contiguous()


STEREO_META_KEYS = ("cv_feat_list", "k2s_sensor", "intrins", "post_rots", "post_trans", "frustum", "downsample",
                    "cv_downsample")


class LSSViewTransformerBEVStereo(LSSViewTransformerBEVDepth):
    """LSSViewTransformerBEVDepth with `cv_frustum`, the frustum of the stride-4 stereo features
    (view_transformer.py:898-904), and `stereo_metas` -- the reference's dict (STEREO_META_KEYS) -- handed through to
    the DepthNet.  `stereo_metas(...)` builds one from the frame's tensors.

    On the fast path the metas may carry two prepared entries, `consts` ([n, 40] fp32 on the features' device:
    functions.stereo_calibration of the frame, uploaded by the caller) and `tables` (the frustum tables there); without
    them they are derived from the reference's keys, which copies host tensors and cannot be captured."""
    CV_DOWNSAMPLE = CV_DOWNSAMPLE       # functions/stereo.py names it once: the stride gen_grid normalises by

    def __init__(self, grid_config, input_size, downsample, in_channels, out_channels, ops=None, seed=0, bev_half=None,
                 depthnet_cfg=None):
        cfg = dict(depthnet_cfg or {})
        if not cfg.get("stereo"):
            raise ValueError("LSSViewTransformerBEVStereo: depthnet_cfg with stereo=True")
        super().__init__(grid_config, input_size, downsample, in_channels, out_channels, ops=ops, seed=seed,
                         bev_half=bev_half, depthnet_cfg=cfg)
        # create_frustum sets self.D as a side effect (the reference's does too); the value is the same here -- the depth
        # axis does not depend on the stride -- and is put back all the same, so that nothing depends on that
        D = self.D
        self.register_buffer("cv_frustum", self.create_frustum(grid_config["depth"], input_size, self.CV_DOWNSAMPLE),
                             persistent=False)
        self.D = D
        self.downsample = downsample        # (the parent keeps it in the frustum only; stereo_metas carries it)

    def stereo_metas(self, prev, curr, k2s_sensor, intrins, post_rots, post_trans, prepare=False):
        """The reference's dict for one frame (curr None: BEVDet fills in the frame's own stride-4 features).
        prepare=True adds `consts` and `tables` on the transformer's device (two small uploads: before a capture, not
        inside one)."""
        metas = dict(cv_feat_list=[prev, curr], k2s_sensor=k2s_sensor, intrins=intrins, post_rots=post_rots,
                     post_trans=post_trans, frustum=self.cv_frustum, downsample=self.downsample,
                     cv_downsample=self.CV_DOWNSAMPLE)
        if prepare:
            from .functions import stereo as S
            metas["consts"] = S.stereo_calibration(k2s_sensor, intrins, post_rots, post_trans).to(self.cv_frustum.device)
            metas["tables"] = S.stereo_frustum_tables(self.cv_frustum)
        return metas

    @staticmethod
    def _check_metas(stereo_metas):
        if stereo_metas is None:
            raise ValueError("LSSViewTransformerBEVStereo needs stereo_metas (view.stereo_metas(...) of the frame)")
        lost = [k for k in STEREO_META_KEYS if k not in stereo_metas]
        if lost:
            raise ValueError(f"stereo_metas lacks {lost}")

    def _stereo_fast(self, stereo_metas):
        """The launch takes channels-last fp16 CUDA features; anything else goes the plain way."""
        self._check_metas(stereo_metas)
        prev, curr = stereo_metas["cv_feat_list"]
        ok = lambda t: t.is_cuda and t.dtype == torch.float16 and t.dim() == 4 and \
            t.is_contiguous(memory_format=torch.channels_last)
        return ok(curr) and (prev is None or ok(prev))

    def _stereo_operands(self, stereo_metas, x):
        from .functions import stereo as S
        self._check_metas(stereo_metas)
        prev, curr = stereo_metas["cv_feat_list"]
        consts, tables = stereo_metas.get("consts"), stereo_metas.get("tables")
        if consts is None or tables is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LSSViewTransformerBEVStereo: stereo_metas without `consts` / `tables` and the stream is "
                                   "capturing; build the metas with view.stereo_metas(..., prepare=True) before the capture")
            consts = S.stereo_calibration(stereo_metas["k2s_sensor"], stereo_metas["intrins"], stereo_metas["post_rots"],
                                          stereo_metas["post_trans"]).to(x.device)
            tables = S.stereo_frustum_tables(stereo_metas["frustum"].to(x.device))
        return prev, curr, consts, tables
