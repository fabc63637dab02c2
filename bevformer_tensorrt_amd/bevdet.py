"""BEVDet's view transformer on the MI355X operators (BASELINE config 5).

`LSSViewTransformer` restates the pieces of the reference's Lift-Splat-Shoot neck that surround
the bev_pool_v2 plugin:

  * frustum / calibration geometry -- create_grid_infos, create_frustum, get_lidar_coor,
    voxel_pooling_prepare_v2 (third_party/bev_mmdet3d/models/necks/view_transformer.py:66-168,
    239-312; det2trt/models/necks/view_transformer.py:8 `LSSViewTransformerTRT` adds nothing to
    them).  Index generation must be BIT-EXACT: same torch ops in the same order; the golden
    (tests/golden/bevdet_geometry.npz) is produced by executing the reference's own methods on the
    calibration the reference's test hard-codes.  The reference computes the ranks on the host and
    feeds them to the engine as inputs (tools/bevdet/evaluate_trt.py:107-127); `forward` takes them the
    same way.  `forward_calibrated` / `BEVDetRunner` instead build them ON THE DEVICE from the frame's
    calibration (csrc/lss_prepare.hip), inside the frame's HIP graph: only the twelve 3x3 matrices of
    `calibration_matrices` are host work;
  * `view_transform` -- the slice of BEVDetTRT.forward_trt between the image neck and the BEV
    encoder (det2trt/models/detector/bevdet.py:50-76): depth_net (1x1 conv) -> softmax over the D
    depth bins -> bev_pool_v2 (HIP) -> [B, C, bev_h, bev_w].

BEVDet-R50 config (configs/bevdet/bevdet-r50-cbgs.py:44-104): 6 cameras of 256x704, downsample 16
(16x44 features), 59 depth bins, 64 channels, 128x128 BEV cells of 0.8 m.
"""
import contextlib
import os

import torch
import torch.nn as nn

from . import functions as _hip_ops
from .functions import dispatch as _dispatch
from .functions.multi_scale_deformable_attn import _TensorCache
from .graph_runner import capture

# BEVDet(..., bev_half=...): "torch" = the framework statements between the image neck and the detections (depth_net
# through the library, softmax / slice / layout copies, F.interpolate + torch.cat, the heads' narrow convolutions
# through the library), "hip" = those on this package's kernels (see BEVDet.prepare_bev_half).  The environment
# variable overrides the DEFAULT, read at construction.
BEV_HALF_MODES = ("torch", "hip")


def default_bev_half():
    mode = os.environ.get("BEVOPS_BEVDET_BEV_HALF", "torch")
    if mode not in BEV_HALF_MODES:
        raise ValueError(f"BEVOPS_BEVDET_BEV_HALF = {mode!r}: 'torch' or 'hip'")
    return mode


def _rule_dispatch():
    """The dense / convolution dispatch by RULE for the calling thread (functions.dispatch.DETERMINISTIC): this package's
    kernels whatever the shipped table measured, no measurement at run time, no library fall-back under capture."""
    return _dispatch.using(rule=True)


DEPTH_NET_COLUMNS = 128   # the merged depth_net GEMM's row: [features | depth logits | zero pad]


def merge_depth_net(weight, bias, D, C):
    """depth_net ([D + C, Cin, 1, 1]: depth logits first, then the context features) as ONE GEMM operand whose output
    row the split kernel reads in place: weight [128, Cin] and bias [128] with the features in columns 0 .. C, the
    depth logits in columns `depth_offset` = C rounded up to 8 .. + D, zero columns behind them.  Both ranges start
    16-byte aligned.  -> (weight, bias, layout) with layout = dict(row_stride, feat_offset, depth_offset)."""
    cin = weight.shape[1]
    depth_offset = (C + 7) // 8 * 8
    if weight.shape[0] != D + C or depth_offset + D > DEPTH_NET_COLUMNS:
        raise ValueError(f"merge_depth_net: {weight.shape[0]} rows for D = {D}, C = {C} ({DEPTH_NET_COLUMNS} columns)")
    w2 = weight.detach().reshape(D + C, cin)
    w = w2.new_zeros((DEPTH_NET_COLUMNS, cin))
    b = w2.new_zeros((DEPTH_NET_COLUMNS,))
    w[:C].copy_(w2[D:])
    w[depth_offset:depth_offset + D].copy_(w2[:D])
    if bias is not None:
        b[:C].copy_(bias.detach()[D:])
        b[depth_offset:depth_offset + D].copy_(bias.detach()[:D])
    return w, b, dict(row_stride=DEPTH_NET_COLUMNS, feat_offset=0, depth_offset=depth_offset)


HEAD_PACK_CHANNELS = 32   # the packed head output: 20 channels in HEADS_R50 order, then zero channels


def merge_heads(first, final):
    """The six two-convolution heads as two convolutions.  first / final: lists of (weight, bias) in head order,
    weight [64, Cs, 3, 3] and [c_i, 64, 3, 3].  -> (w1 [6 * 64, Cs, 3, 3], b1, w2 [32, 6 * 64, 3, 3], b2, slices):
    w1 / b1 are the first convolutions stacked along the output channels; w2 is block-diagonal -- head i's final
    weights on input channels 64 i .. 64 i + 63, its c_i output channels at slices[i] = (start, stop), heads in order,
    zero rows behind channel sum(c_i).  A zero weight adds an exact zero to the fp32 accumulator, so every head's
    output is what its own two convolutions give."""
    mid = first[0][0].shape[0]
    n_out = sum(w.shape[0] for w, _ in final)
    if n_out > HEAD_PACK_CHANNELS:
        raise ValueError(f"merge_heads: {n_out} output channels, the packed output holds {HEAD_PACK_CHANNELS}")
    w0 = first[0][0].detach()
    w1 = w0.new_zeros((len(first) * mid,) + tuple(w0.shape[1:]))
    b1 = w0.new_zeros((len(first) * mid,))
    w2 = w0.new_zeros((HEAD_PACK_CHANNELS, len(first) * mid) + tuple(final[0][0].shape[2:]))
    b2 = w0.new_zeros((HEAD_PACK_CHANNELS,))
    slices, at = [], 0
    for i, ((wa, ba), (wb, bb)) in enumerate(zip(first, final)):
        if wa.shape[0] != mid or wb.shape[1] != mid:
            raise ValueError("merge_heads: every head needs the same middle width")
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

# data_config of configs/bevdet/bevdet-r50-cbgs.py:44-62, the entries the test pipeline reads
DATA_CONFIG_R50 = dict(input_size=(256, 704), src_size=(900, 1600), crop_h=(0.0, 0.0), resize_test=0.0)

BEVDET_R50 = dict(
    grid_config=dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 60.0, 1.0]),
    input_size=(256, 704), downsample=16, in_channels=256, out_channels=64)
# BEVDepth-R50: the same detector with the camera-aware DepthNet + ASPP in front of the pooling (bevdepth.py), without
# and with the reference's DCN layer behind the ASPP (DepthNet's default use_dcn=True: mmcv's DCNv1 pack, groups = 4)
BEVDEPTH_R50 = dict(BEVDET_R50, view_transformer="bevdepth", depthnet_cfg=dict(use_dcn=False))
BEVDEPTH_R50_DCN = dict(BEVDET_R50, view_transformer="bevdepth", depthnet_cfg=dict(use_dcn=True))
# BEVStereo-R50: BEVDepth's DepthNet with the temporal-stereo cost volume of the previous frame's stride-4 backbone
# features (bevdepth.LSSViewTransformerBEVStereo).  The reference tree has no BEVStereo config: bias = 5.0 and the finer
# depth grid of the original BEVStereo configs are recalled, not read from it; this keeps BEVDET_R50's grid (D = 59).
BEVSTEREO_R50 = dict(BEVDET_R50, view_transformer="bevstereo", depthnet_cfg=dict(use_dcn=False, stereo=True, bias=5.0))


class LSSViewTransformer(nn.Module):
    def __init__(self, grid_config, input_size, downsample, in_channels, out_channels, ops=None, seed=0, bev_half=None):
        super().__init__()
        torch.manual_seed(seed)
        self.ops = ops if ops is not None else _hip_ops
        self.bev_half = default_bev_half() if bev_half is None else bev_half
        if self.bev_half not in BEV_HALF_MODES:
            raise ValueError(f"bev_half = {self.bev_half!r}: 'torch' or 'hip'")
        self.create_grid_infos(**grid_config)
        self.frustum = self.create_frustum(grid_config["depth"], input_size, downsample)
        self.out_channels, self.in_channels = out_channels, in_channels
        self.depth_net = nn.Conv2d(in_channels, self.D + out_channels, kernel_size=1, padding=0)   # :59-61

    # ---- view_transformer.py:66-83
    def create_grid_infos(self, x, y, z, **kwargs):
        self.grid_lower_bound = torch.Tensor([cfg[0] for cfg in [x, y, z]])
        self.grid_interval = torch.Tensor([cfg[2] for cfg in [x, y, z]])
        self.grid_size = torch.Tensor([(cfg[1] - cfg[0]) / cfg[2] for cfg in [x, y, z]])

    # ---- view_transformer.py:85-124 (sid = False)
    def create_frustum(self, depth_cfg, input_size, downsample):
        H_in, W_in = input_size
        H_feat, W_feat = H_in // downsample, W_in // downsample
        d = torch.arange(*depth_cfg, dtype=torch.float).view(-1, 1, 1).expand(-1, H_feat, W_feat)
        self.D = d.shape[0]
        x = torch.linspace(0, W_in - 1, W_feat, dtype=torch.float).view(1, 1, W_feat).expand(self.D, H_feat, W_feat)
        y = torch.linspace(0, H_in - 1, H_feat, dtype=torch.float).view(1, H_feat, 1).expand(self.D, H_feat, W_feat)
        return torch.stack((x, y, d), -1)

    # ---- view_transformer.py:126-168
    def get_lidar_coor(self, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        B, N, _, _ = sensor2ego.shape
        points = self.frustum.to(sensor2ego) - post_trans.view(B, N, 1, 1, 1, 3)
        points = torch.inverse(post_rots).view(B, N, 1, 1, 1, 3, 3).matmul(points.unsqueeze(-1))
        points = torch.cat((points[..., :2, :] * points[..., 2:3, :], points[..., 2:3, :]), 5)
        combine = sensor2ego[:, :, :3, :3].matmul(torch.inverse(cam2imgs))
        points = combine.view(B, N, 1, 1, 1, 3, 3).matmul(points).squeeze(-1)
        points += sensor2ego[:, :, :3, 3].view(B, N, 1, 1, 1, 3)
        points = bda.view(B, 1, 1, 1, 1, 3, 3).matmul(points.unsqueeze(-1)).squeeze(-1)
        return points

    # ---- view_transformer.py:239-312
    def voxel_pooling_prepare_v2(self, coor):
        B, N, D, H, W, _ = coor.shape
        num_points = B * N * D * H * W
        ranks_depth = torch.arange(0, num_points, dtype=torch.int, device=coor.device)
        ranks_feat = torch.arange(0, num_points // D, dtype=torch.int, device=coor.device)
        ranks_feat = ranks_feat.reshape(B, N, 1, H, W).expand(B, N, D, H, W).flatten()
        coor = (coor - self.grid_lower_bound.to(coor)) / self.grid_interval.to(coor)
        coor = coor.long().view(num_points, 3)
        batch_idx = torch.arange(0, B).reshape(B, 1).expand(B, num_points // B).reshape(num_points, 1).to(coor)
        coor = torch.cat((coor, batch_idx), 1)
        kept = ((coor[:, 0] >= 0) & (coor[:, 0] < self.grid_size[0]) & (coor[:, 1] >= 0)
                & (coor[:, 1] < self.grid_size[1]) & (coor[:, 2] >= 0) & (coor[:, 2] < self.grid_size[2]))
        if len(kept) == 0:
            return None, None, None, None, None
        coor, ranks_depth, ranks_feat = coor[kept], ranks_depth[kept], ranks_feat[kept]
        ranks_bev = coor[:, 3] * (self.grid_size[2] * self.grid_size[1] * self.grid_size[0])
        ranks_bev += coor[:, 2] * (self.grid_size[1] * self.grid_size[0])
        ranks_bev += coor[:, 1] * self.grid_size[0] + coor[:, 0]
        order = ranks_bev.argsort()
        ranks_bev, ranks_depth, ranks_feat = ranks_bev[order], ranks_depth[order], ranks_feat[order]
        kept = torch.ones(ranks_bev.shape[0], device=ranks_bev.device, dtype=torch.bool)
        kept[1:] = ranks_bev[1:] != ranks_bev[:-1]
        interval_starts = torch.where(kept)[0].int()
        if len(interval_starts) == 0:
            return None, None, None, None, None
        interval_lengths = torch.zeros_like(interval_starts)
        interval_lengths[:-1] = interval_starts[1:] - interval_starts[:-1]
        interval_lengths[-1] = ranks_bev.shape[0] - interval_starts[-1]
        return (ranks_bev.int().contiguous(), ranks_depth.int().contiguous(), ranks_feat.int().contiguous(),
                interval_starts.int().contiguous(), interval_lengths.int().contiguous())

    def get_bev_pool_input(self, sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda):
        """BEVDetTRT.get_bev_pool_input (det2trt/models/detector/bevdet.py:14-27)."""
        coor = self.get_lidar_coor(sensor2keyegos, ego2globals, intrins, post_rots, post_trans, bda)
        return self.voxel_pooling_prepare_v2(coor)

    # ---- the same geometry split for the device index build (functions/lss_prepare.py, csrc/lss_prepare.hip)
    def calibration_matrices(self, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        """The small matrices of get_lidar_coor, by the reference's own torch ops on the host, as ONE packed fp32
        buffer [N * 24 + 9]: per camera [inverse(post_rots) 9 | post_trans 3 | combine 9 | trans 3] with
        combine = sensor2ego[:3,:3] @ inverse(cam2imgs), trans = sensor2ego[:3,3]; then bda 9.  Batch 1.
        `ego2global` is accepted and unused, as in the reference."""
        B, N, _, _ = sensor2ego.shape
        if B != 1:
            raise ValueError("calibration_matrices: batch 1 only (the pooling plugin is batch-1)")
        sensor2ego, cam2imgs, post_rots, post_trans, bda = (t.detach().to("cpu", torch.float32) for t in
                                                            (sensor2ego, cam2imgs, post_rots, post_trans, bda))
        inv_post = torch.inverse(post_rots)                                        # :143
        combine = sensor2ego[:, :, :3, :3].matmul(torch.inverse(cam2imgs))         # :150
        per_cam = torch.cat((inv_post.reshape(N, 9), post_trans.reshape(N, 3), combine.reshape(N, 9),
                             sensor2ego[:, :, :3, 3].reshape(N, 3)), 1)
        return torch.cat((per_cam.reshape(-1), bda.reshape(-1)[:9])).contiguous()

    def calibration_matrices_batched(self, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        """`calibration_matrices` for B samples: [B, N * 24 + 9], row b the packed buffer of sample b (its own cameras
        and its own bda), each row evaluated by that sample's own call -- so row 0 at B = 1 equals
        `calibration_matrices`, and a sample's row does not depend on its neighbours in the batch."""
        B = sensor2ego.shape[0]
        if B < 1 or any(t.shape[0] != B for t in (cam2imgs, post_rots, post_trans, bda)):
            raise ValueError("calibration_matrices_batched: every tensor carries the same leading B >= 1")
        return torch.stack([self.calibration_matrices(sensor2ego[b:b + 1], None, cam2imgs[b:b + 1], post_rots[b:b + 1],
                                                      post_trans[b:b + 1], bda[b:b + 1]) for b in range(B)]).contiguous()

    def lidar_coor_plain(self, calib):
        """get_lidar_coor from the packed `calibration_matrices` buffer in plain order: fp32, every product and sum
        rounded on its own, each 3x3 . 3x1 product summed in ascending k ((m0 p0 + m1 p1) + m2 p2).  This is the
        arithmetic of the device kernel; on the CPU it equals get_lidar_coor bit for bit.  -> [1, N, D, H, W, 3];
        the 2-D buffer [B, N * 24 + 9] of `calibration_matrices_batched` -> [B, N, D, H, W, 3]."""
        if calib.dim() == 2:
            return torch.cat([self.lidar_coor_plain(row) for row in calib], 0).contiguous()
        calib = calib.detach().to("cpu", torch.float32).view(-1)
        N = (calib.numel() - 9) // 24
        cam = calib[:N * 24].view(N, 1, 1, 1, 24)

        def mat3(m, p):
            return torch.stack([(m[..., 3 * r] * p[..., 0] + m[..., 3 * r + 1] * p[..., 1]) + m[..., 3 * r + 2] * p[..., 2]
                                for r in range(3)], -1)
        p = self.frustum.to(torch.float32).unsqueeze(0) - cam[..., 9:12]
        p = mat3(cam[..., 0:9], p)
        p = torch.stack((p[..., 0] * p[..., 2], p[..., 1] * p[..., 2], p[..., 2]), -1)
        p = mat3(cam[..., 12:21], p)
        p = p + cam[..., 21:24]
        p = mat3(calib[N * 24:].view(1, 1, 1, 1, 9), p)
        return p.unsqueeze(0).contiguous()

    def prepare_stable(self, coor):
        """voxel_pooling_prepare_v2 with argsort(stable=True): the CPU / torch statement of what the device build
        returns.  The reference's argsort leaves the order inside a cell unspecified; here it is ascending point index.
        Same ranks_bev, interval_starts and interval_lengths; ranks_depth / ranks_feat permuted inside intervals."""
        B, N, D, H, W, _ = coor.shape
        num_points = B * N * D * H * W
        ranks_depth = torch.arange(0, num_points, dtype=torch.int, device=coor.device)
        ranks_feat = torch.arange(0, num_points // D, dtype=torch.int, device=coor.device)
        ranks_feat = ranks_feat.reshape(B, N, 1, H, W).expand(B, N, D, H, W).flatten()
        coor = (coor - self.grid_lower_bound.to(coor)) / self.grid_interval.to(coor)
        coor = coor.long().view(num_points, 3)
        batch_idx = torch.arange(0, B).reshape(B, 1).expand(B, num_points // B).reshape(num_points, 1).to(coor)
        coor = torch.cat((coor, batch_idx), 1)
        kept = ((coor[:, 0] >= 0) & (coor[:, 0] < self.grid_size[0]) & (coor[:, 1] >= 0)
                & (coor[:, 1] < self.grid_size[1]) & (coor[:, 2] >= 0) & (coor[:, 2] < self.grid_size[2]))
        if len(kept) == 0:
            return None, None, None, None, None
        coor, ranks_depth, ranks_feat = coor[kept], ranks_depth[kept], ranks_feat[kept]
        ranks_bev = coor[:, 3] * (self.grid_size[2] * self.grid_size[1] * self.grid_size[0])
        ranks_bev += coor[:, 2] * (self.grid_size[1] * self.grid_size[0])
        ranks_bev += coor[:, 1] * self.grid_size[0] + coor[:, 0]
        order = ranks_bev.argsort(stable=True)
        ranks_bev, ranks_depth, ranks_feat = ranks_bev[order], ranks_depth[order], ranks_feat[order]
        kept = torch.ones(ranks_bev.shape[0], device=ranks_bev.device, dtype=torch.bool)
        kept[1:] = ranks_bev[1:] != ranks_bev[:-1]
        interval_starts = torch.where(kept)[0].int()
        if len(interval_starts) == 0:
            return None, None, None, None, None
        interval_lengths = torch.zeros_like(interval_starts)
        interval_lengths[:-1] = interval_starts[1:] - interval_starts[:-1]
        interval_lengths[-1] = ranks_bev.shape[0] - interval_starts[-1]
        return (ranks_bev.int().contiguous(), ranks_depth.int().contiguous(), ranks_feat.int().contiguous(),
                interval_starts.int().contiguous(), interval_lengths.int().contiguous())

    def _frustum_on(self, device):
        cache = self.__dict__.setdefault("_frustum_dev", {})
        if device not in cache:
            cache[device] = self.frustum.to(device, torch.float32).contiguous()
        return cache[device]

    def prepare_calibrated(self, calib, padded=True):
        """The five index arrays (+ counts when padded) from the packed calibration buffer ON THE DEVICE `calib` lives
        on: functions.lss_voxel_prepare with this transformer's frustum and grid.  A 2-D calib [B, N * 24 + 9]: the
        batched arrays of functions.lss_voxel_prepare_batched."""
        name = "lss_voxel_prepare_batched" if calib.dim() == 2 else "lss_voxel_prepare"
        prepare = getattr(self.ops, name, getattr(_hip_ops, name))   # (an INT8 operator set has none)
        return prepare(self._frustum_on(calib.device), calib, self.grid_lower_bound, self.grid_interval, self.grid_size,
                       padded=padded)

    # ---- bev_half = "hip": depth_net as one 128-column GEMM, softmax + split as one launch, no layout copies
    def _hip_on(self, x):
        """"hip" takes effect for channels-last fp16 CUDA activations on an operator set that has the new functions and
        a plain depth_net (an INT8 build's operator set / quantised layer keep the torch statements)."""
        return self.bev_half == "hip" and x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 \
            and x.is_contiguous(memory_format=torch.channels_last) and type(self.depth_net) is nn.Conv2d \
            and all(hasattr(self.ops, f) for f in ("lss_depth_split", "dense_auto"))

    def _depth_net_sources(self):
        return [self.depth_net.weight] + ([] if self.depth_net.bias is None else [self.depth_net.bias])

    def depth_net_merged(self, build=True):
        """(weight [128, Cin], bias [128], layout) of `merge_depth_net` on the device of depth_net's weight, cached and
        rebuilt when the weight or bias changes (stamped like functions.conv.pack_taps' cache).  build=False: None when
        the cached operand is missing or stale."""
        stamp = tuple(_TensorCache._stamp(t) for t in self._depth_net_sources())
        hit = self.__dict__.get("_depth_net_merged")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if not build:
            return None
        merged = merge_depth_net(self.depth_net.weight, self.depth_net.bias, self.D, self.out_channels)
        self.__dict__["_depth_net_merged"] = (stamp, merged)
        return merged

    def _depth_feat_hip(self, x):
        """x [N, Cin, H, W] channels-last fp16 -> (depth [N, D, H, W], feat [N, H, W, C]): two launches."""
        merged = self.depth_net_merged(build=False)
        if merged is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("LSSViewTransformer: the merged depth_net operand is missing or stale and the stream "
                                   "is capturing; call BEVDet.prepare_bev_half() (or the model once, eagerly) first")
            merged = self.depth_net_merged()
        w, b, lay = merged
        n, cin, h, wd = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(n * h * wd, cin)        # (a view: channels-last)
        with _rule_dispatch():
            y = self.ops.dense_auto(rows, w, b, None, False)
        return self.ops.lss_depth_split(y, n, self.D, self.out_channels, lay["depth_offset"], lay["feat_offset"],
                                        spatial=(h, wd))

    @torch.no_grad()
    def view_transform_calibrated(self, x, calib):
        """`view_transform` with the index build on the device: x as there, calib = the packed fp32 buffer of
        `calibration_matrices` on x's device.  No host synchronisation: capturable with the frame.
        calib [B, N * 24 + 9] (`calibration_matrices_batched`) with x [B * N_cams, ...]: B samples -> [B, C, h, w]."""
        rb, rd, rf, ist, il, counts = self.prepare_calibrated(calib)
        bev_h, bev_w = int(self.grid_size[1]), int(self.grid_size[0])
        # (batch is passed only when there is one, so an operator set written for one sample serves a 1-D calib as before)
        kw = dict(batch=calib.shape[0]) if calib.dim() == 2 else {}
        if calib.dim() == 2 and x.shape[0] * 24 != calib.shape[0] * (calib.shape[1] - 9):
            raise ValueError(f"calib {tuple(calib.shape)} does not describe the {x.shape[0]} camera images of x")
        if self._hip_on(x):
            depth, tran_feat = self._depth_feat_hip(x)
            out = self.ops.bev_pool_v2_indirect(depth, tran_feat, rd, rf, rb, ist, il, counts, bev_h, bev_w, **kw)
            return out.permute(0, 3, 1, 2)       # (channels-last view: what bev_encoder takes, no copy either way)
        x = self.depth_net(x)
        depth = x[:, : self.D].softmax(dim=1)
        tran_feat = x[:, self.D: self.D + self.out_channels].permute(0, 2, 3, 1)
        depth, tran_feat = depth.contiguous(), tran_feat.contiguous()
        bev_h, bev_w = int(self.grid_size[1]), int(self.grid_size[0])
        out = self.ops.bev_pool_v2_indirect(depth, tran_feat, rd, rf, rb, ist, il, counts, bev_h, bev_w, **kw)
        return out.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def view_transform(self, x, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths):
        """x [N_cams, in_channels, H_feat, W_feat] (image-neck output) -> BEV features
        [1, out_channels, bev_h, bev_w]: BEVDetTRT.forward_trt, det2trt/models/detector/bevdet.py:50-76."""
        if self._hip_on(x):
            depth, tran_feat = self._depth_feat_hip(x)
            out = self.ops.bev_pool_v2_2(depth, tran_feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                         interval_lengths, int(self.grid_size[1]), int(self.grid_size[0]))
            return out.permute(0, 3, 1, 2)
        x = self.depth_net(x)
        depth = x[:, : self.D].softmax(dim=1)
        tran_feat = x[:, self.D: self.D + self.out_channels].permute(0, 2, 3, 1)
        depth, tran_feat = depth.contiguous(), tran_feat.contiguous()
        bev_h, bev_w = int(self.grid_size[1]), int(self.grid_size[0])
        out = self.ops.bev_pool_v2_2(depth, tran_feat, ranks_depth, ranks_feat, ranks_bev, interval_starts,
                                     interval_lengths, bev_h, bev_w)
        return out.permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- the whole detector (BASELINE config 5)
# BEVDetTRT.forward_trt (det2trt/models/detector/bevdet.py:29-82) re-hosted without mmcv / mmdet, frozen BatchNorm
# folded into the convolution in front of it:
#   image [1, 6, 3, 256, 704] -> ResNet-50 (style "pytorch", out_indices (2, 3); configs/bevdet/bevdet-r50-cbgs.py:73-84)
#   -> CustomFPN (1024 / 2048 -> 256, top-down add, ONE 3x3 output convolution on the stride-16 level;
#      third_party/bev_mmdet3d/models/necks/fpn.py) -> depth_net -> depth softmax -> bev_pool_v2 (the plugin)
#   -> CustomResNet bev encoder (basic blocks, 64 -> 128 / 256 / 512, strides 2; models/backbone/bev_resnet.py)
#   -> FPN_LSS (bilinear x4 of the stride-8 level, concatenation with the stride-2 level, two 3x3 convolutions,
#      bilinear x2, 3x3 + 1x1; models/necks/lss_fpn.py) -> CenterHead.forward_trt (shared 3x3 convolution, one task,
#      six two-convolution heads with final_kernel 3; det2trt/models/dense_heads/centerpoint_head.py:42-53).
# Two data paths through the same weights, as in bevformer.py: `forward` (NCHW, library convolutions -- the reference
# op sequence, any device / dtype) and the channels-last fp16 path on this package's convolution / GEMM kernels.
from . import bevformer as _B   # noqa: E402  (ResNet and the channels-last convolution helpers)
import torch.nn.functional as F   # noqa: E402

HEADS_R50 = (("reg", 2), ("height", 1), ("dim", 3), ("rot", 2), ("vel", 2), ("heatmap", 10))
# bbox_coder of configs/bevdet/bevdet-r50-cbgs.py:138-147 (= test_cfg :167-178); norm_bbox=True (:152)
CENTERPOINT_CODER_R50 = dict(pc_range=[-51.2, -51.2], post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=500,
                             score_threshold=0.1, out_size_factor=8, voxel_size=[0.1, 0.1], code_size=9)
# test_cfg of configs/bevdet/bevdet-r50-cbgs.py:167-182 (the values the NMS reads; one task): rotated scale-NMS
CENTERPOINT_TEST_CFG_R50 = dict(nms_type="rotate", nms_thr=0.2, pre_max_size=1000, post_max_size=500,
                                nms_rescale_factor=[1.0, 0.7, 0.7, 0.4, 0.55, 1.1, 1.0, 1.0, 1.5, 3.5],
                                min_radius=[4, 12, 10, 1, 0.85, 0.175])


def _conv(ops, x, conv, relu=False, residual=None):
    """act(conv(x) + bias + residual) for a BN-folded nn.Conv2d: channels-last fp16 tensors take this package's
    kernels (1x1: GEMM over the pixel rows; 3x3: implicit GEMM), everything else the library convolution."""
    fast = x.is_cuda and x.dtype == torch.float16 and x.is_contiguous(memory_format=torch.channels_last) \
        and hasattr(ops, "conv3x3_auto") and conv.out_channels % 8 == 0    # (the heads' 1 / 2 / 3-channel outputs: library)
    if fast and conv.kernel_size == (1, 1):
        return _B._conv1x1_nhwc(ops, x, conv, relu, residual)
    if fast and conv.kernel_size == (3, 3) and conv.in_channels % 32 == 0:
        return _B._conv_nhwc(ops, x, conv, relu, residual)
    y = F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


class BasicBlock(nn.Module):
    """mmdet BasicBlock with the 3x3 downsample convolution CustomResNet gives the first block of a stage."""

    def __init__(self, cin, cout, stride, downsample):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(cin, cout, 3, stride, 1), nn.Conv2d(cout, cout, 3, 1, 1)
        self.downsample = nn.Conv2d(cin, cout, 3, stride, 1) if downsample else None

    def forward(self, x, ops):
        idt = x if self.downsample is None else _conv(ops, x, self.downsample)
        return _conv(ops, _conv(ops, x, self.conv1, True), self.conv2, True, idt)


class CustomFPN(nn.Module):
    """CustomFPN(in_channels=[1024, 2048], out_channels=256, num_outs=1, out_ids=[0]) of the BEVDet-R50 config
    (third_party/bev_mmdet3d/models/necks/fpn.py:158-183): two lateral 1x1 convolutions, nearest top-down add, one
    3x3 output convolution on the finer level."""

    def __init__(self, cins=(1024, 2048), cout=256):
        super().__init__()
        self.lateral = nn.ModuleList(nn.Conv2d(c, cout, 1) for c in cins)
        self.fpn_conv = nn.Conv2d(cout, cout, 3, 1, 1)

    def topdown_nhwc(self, lats, ops):
        """everything behind the lateral convolutions (the INT8 chain evaluates those itself); any layout"""
        l4, l5 = lats
        up_add = getattr(ops, "upsample_add_nhwc_", None)
        if up_add is not None and l4.is_cuda and l4.dtype == torch.float16 \
                and l4.is_contiguous(memory_format=torch.channels_last) and l5.is_contiguous(memory_format=torch.channels_last):
            up_add(l4, l5)
        else:
            l4 = l4 + F.interpolate(l5, size=l4.shape[2:], mode="nearest")
        return _conv(ops, l4, self.fpn_conv)

    def forward(self, feats, ops):
        return self.topdown_nhwc([_conv(ops, f, l) for l, f in zip(self.lateral, feats)], ops)


class BEVDet(nn.Module):
    """forward(image [1, 6, 3, H, W], ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths)
    -> (reg, height, dim, rot, vel, heatmap), each [1, c, 128, 128] -- BEVDetTRT.forward_trt."""

    def __init__(self, cfg=None, ops=None, seed=0, bev_half=None):
        super().__init__()
        torch.manual_seed(seed)
        cfg = cfg or BEVDET_R50
        self.cfg = cfg
        self.bev_half = default_bev_half() if bev_half is None else bev_half
        if self.bev_half not in BEV_HALF_MODES:
            raise ValueError(f"bev_half = {self.bev_half!r}: 'torch' or 'hip'")
        self.ops = ops = ops if ops is not None else _hip_ops
        self.stereo = cfg.get("view_transformer") == "bevstereo"
        # (BEVStereo: the stride-4 stage too, the features the cost volume is built from)
        self.backbone = _B.ResNet(50, (False,) * 4, (0, 2, 3) if self.stereo else (2, 3), ops, "pytorch")
        self.neck = CustomFPN()
        view_kw = dict({k: cfg[k] for k in ("grid_config", "input_size", "downsample", "in_channels", "out_channels")},
                       ops=ops, seed=seed, bev_half=self.bev_half)
        if cfg.get("view_transformer") == "bevdepth":      # BEVDEPTH_R50: the camera-aware DepthNet (bevdepth.py)
            from .bevdepth import LSSViewTransformerBEVDepth
            self.view = LSSViewTransformerBEVDepth(**view_kw, depthnet_cfg=cfg.get("depthnet_cfg"))
        elif self.stereo:                                  # BEVSTEREO_R50: the cost volume in front of the DepthNet's blocks
            from .bevdepth import LSSViewTransformerBEVStereo
            self.view = LSSViewTransformerBEVStereo(**view_kw, depthnet_cfg=cfg.get("depthnet_cfg"))
        elif cfg.get("view_transformer") not in (None, "lss"):
            raise ValueError(f"view_transformer = {cfg.get('view_transformer')!r}: 'lss', 'bevdepth' or 'bevstereo'")
        else:
            self.view = LSSViewTransformer(**view_kw)
        c = cfg["out_channels"]
        chans, cin, stages = [2 * c, 4 * c, 8 * c], c, []
        for ch in chans:
            stages.append(nn.ModuleList([BasicBlock(cin, ch, 2, True), BasicBlock(ch, ch, 1, False)]))
            cin = ch
        self.bev_stages = nn.ModuleList(stages)
        self.neck_conv = nn.ModuleList([nn.Conv2d(chans[2] + chans[0], 512, 3, 1, 1), nn.Conv2d(512, 512, 3, 1, 1)])
        self.up2_conv = nn.ModuleList([nn.Conv2d(512, 256, 3, 1, 1), nn.Conv2d(256, 256, 1)])
        self.shared_conv = nn.Conv2d(256, 64, 3, 1, 1)
        self.heads = nn.ModuleDict({k: nn.ModuleList([nn.Conv2d(64, 64, 3, 1, 1), nn.Conv2d(64, n, 3, 1, 1)])
                                    for k, n in HEADS_R50})
        self.eval()

    def _nhwc_weights(self):
        """Once per model: the 3x3 / 7x7 filters channels-last, like the activations of the fp16 path."""
        if not getattr(self, "_nhwc_ready", False):
            for m in self.modules():
                if isinstance(m, nn.Conv2d) and m.kernel_size != (1, 1):
                    m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
            self._nhwc_ready = True

    def image_features(self, image, stereo=False):
        """img_backbone + img_neck: [6, 3, H, W] -> [6, 256, H / 16, W / 16].  stereo=True (a BEVStereo model;
        image_encoder, third_party/bev_mmdet3d/models/detectors/bevdet.py:35-50): -> (that, the backbone's stride-4
        features [6, 256, H / 4, W / 4])."""
        if stereo and not self.stereo:
            raise ValueError("image_features(stereo=True): a BEVStereo model (cfg view_transformer='bevstereo')")
        ops = self.ops
        nhwc = image.is_cuda and image.dtype == torch.float16 and hasattr(ops, "conv3x3_auto")
        if nhwc:
            self._nhwc_weights()
            chain = getattr(self, "int8_chain", None)     # quantization.Int8ChainBackbone, after its freeze()
            if chain is not None and chain.ready:
                return chain(image)
            feats = self.backbone.forward_nhwc(image, ops)
        else:
            feats = self.backbone(image)
        if self.stereo:
            x = self.neck(feats[1:], ops)
            return (x, feats[0]) if stereo else x
        return self.neck(feats, ops)

    def _frame_features(self, image, stereo_metas):
        """-> (image features, the view transformer's keyword arguments).  A BEVStereo model: the metas' current
        features (cv_feat_list[1]) are this frame's stride-4 features when the caller left them None."""
        if not self.stereo:
            if stereo_metas is not None:
                raise ValueError("stereo_metas: a BEVStereo model (cfg view_transformer='bevstereo')")
            return self.image_features(image), {}
        if stereo_metas is None:
            raise ValueError("a BEVStereo model needs stereo_metas (view.stereo_metas(prev, None, ...) of the frame)")
        x, feat = self.image_features(image, stereo=True)
        prev, curr = stereo_metas["cv_feat_list"]
        return x, dict(stereo_metas=dict(stereo_metas, cv_feat_list=[prev, feat if curr is None else curr]))

    # ---- bev_half = "hip" (see the section in design/model.md)
    def _hip_on(self, x):
        """"hip" takes effect for fp16 CUDA tensors on an operator set that has the new functions; everything else
        (other dtypes, the CPU, the INT8 plugin set) keeps the torch statements."""
        return self.bev_half == "hip" and x.is_cuda and x.dtype == torch.float16 \
            and all(hasattr(self.ops, f) for f in ("upsample_bilinear_concat_nhwc", "lss_depth_split", "conv_nhwc",
                                                   "conv3x3_auto", "dense_auto")) \
            and all(type(c) is nn.Conv2d for h in self.heads.values() for c in h)

    def _head_sources(self):
        return [t for k, _ in HEADS_R50 for c in self.heads[k] for t in (c.weight, c.bias) if t is not None]

    def heads_merged(self, build=True):
        """(w1, b1, w2, b2, slices) of `merge_heads` for the six heads, on the device of their weights; cached and
        rebuilt when a source weight or bias changes.  build=False: None when missing or stale."""
        stamp = tuple(_TensorCache._stamp(t) for t in self._head_sources())
        hit = self.__dict__.get("_heads_merged")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        if not build:
            return None
        hs = [self.heads[k] for k, _ in HEADS_R50]
        w1, b1, w2, b2, slices = merge_heads([(h[0].weight, h[0].bias) for h in hs], [(h[1].weight, h[1].bias) for h in hs])
        # (taps-major kernels read channels-last weights; keep the layout the model's own 3x3 weights have)
        merged = (w1.contiguous(memory_format=torch.channels_last), b1, w2.contiguous(memory_format=torch.channels_last), b2,
                  slices)
        self.__dict__["_heads_merged"] = (stamp, merged)
        return merged

    def prepare_bev_half(self):
        """Build (or refresh) the merged operands of the "hip" BEV half on the device the weights live on: depth_net as
        a 128-column GEMM ([features | depth logits | zeros]), the six heads' first convolutions as one 64 -> 384
        convolution, their final convolutions as one block-diagonal 384 -> 32 convolution.  Allocates and copies, so it
        must run OUTSIDE stream capture; `forward` / `forward_calibrated` call it themselves when the operands are
        missing or a source weight changed, and raise RuntimeError when that happens on a capturing stream."""
        p = next(self.parameters())
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("BEVDet.prepare_bev_half() allocates: call it before the capture begins")
        if p.is_cuda and p.dtype == torch.float16 and hasattr(self.ops, "conv3x3_auto"):
            self._nhwc_weights()      # (what the first fp16 frame does to the filters; the merged operands follow them)
        self.view.depth_net_merged()
        self.heads_merged()
        return self

    def _bev_half_ready(self, x):
        """True when the "hip" BEV half runs for activations like `x`, with its merged operands in place."""
        if not self._hip_on(x):
            return False
        if self.view.depth_net_merged(build=False) is None or self.heads_merged(build=False) is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("BEVDet(bev_half='hip'): the merged operands are missing or stale and the stream is "
                                   "capturing; call prepare_bev_half() (or the model once, eagerly) before the capture")
            self.prepare_bev_half()
        return True

    def _heads_hip(self, feat):
        """shared_conv, then the six heads as two launches of the tiled implicit GEMM BY RULE (functions.conv_nhwc, not
        the measured dispatch: these shapes are in no table).  -> six channel slices [1, c, H, W] of the packed
        [1, H, W, 32] result (no copy); functions.centerpoint_decode reads such slices in place."""
        ops = self.ops
        w1, b1, w2, b2, slices = self.heads_merged(build=False)
        s = _conv(ops, feat, self.shared_conv, True)
        packed = ops.conv_nhwc(ops.conv_nhwc(s, w1, b1, True), w2, b2, False)
        return tuple(packed[:, a:b] for a, b in slices)

    def bev_encoder(self, x):
        ops = self.ops
        hip = self._hip_on(x) and x.is_contiguous(memory_format=torch.channels_last)
        if x.is_cuda and x.dtype == torch.float16:
            x = x.contiguous(memory_format=torch.channels_last)
        feats = []
        for stage in self.bev_stages:
            for blk in stage:
                x = blk(x, ops)
            feats.append(x)
        if hip:
            # cat([feats[0], x4 bilinear of feats[2]]) as ONE launch, channels-last, no intermediate; then the x2 step
            x = ops.upsample_bilinear_concat_nhwc(feats[0], feats[2])
            x = _conv(ops, _conv(ops, x, self.neck_conv[0], True), self.neck_conv[1], True)
            x = ops.upsample_bilinear_concat_nhwc(None, x, scale_factor=2)
            return _conv(ops, _conv(ops, x, self.up2_conv[0], True), self.up2_conv[1])
        x1 = F.interpolate(feats[2], scale_factor=4, mode="bilinear", align_corners=True)
        x = torch.cat([feats[0], x1], dim=1)
        if feats[0].is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        x = _conv(ops, _conv(ops, x, self.neck_conv[0], True), self.neck_conv[1], True)
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        return _conv(ops, _conv(ops, x, self.up2_conv[0], True), self.up2_conv[1])

    @torch.no_grad()
    def forward(self, image, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, mlp_input=None,
                stereo_metas=None):
        """mlp_input: the BEVDepth transformer's `get_mlp_input` of the frame (view_transformer="bevdepth" /
        "bevstereo" only); stereo_metas: the BEVStereo transformer's (view_transformer="bevstereo" only)."""
        kw = {} if mlp_input is None else dict(mlp_input=mlp_input)
        hip = self._bev_half_ready(image)      # (first: under capture a missing operand raises before anything is launched)
        if hip:
            with _rule_dispatch():      # (the image half too: see forward_calibrated)
                x, skw = self._frame_features(image.flatten(0, 1), stereo_metas)
                bev = self.view.view_transform(x, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths,
                                               **kw, **skw)
                return self._heads_hip(self.bev_encoder(bev))
        x, skw = self._frame_features(image.flatten(0, 1), stereo_metas)
        kw.update(skw)
        bev = self.view.view_transform(x, ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths, **kw)
        feat = self.bev_encoder(bev)
        ops = self.ops
        s = _conv(ops, feat, self.shared_conv, True)
        return tuple(_conv(ops, _conv(ops, s, h[0], True), h[1]) for h in (self.heads[k] for k, _ in HEADS_R50))

    def _heads(self, bev):
        feat = self.bev_encoder(bev)
        ops = self.ops
        s = _conv(ops, feat, self.shared_conv, True)
        return tuple(_conv(ops, _conv(ops, s, h[0], True), h[1]) for h in (self.heads[k] for k, _ in HEADS_R50))

    @torch.no_grad()
    def forward_calibrated(self, image, calib, stereo_metas=None):
        """`forward` from the frame's calibration instead of ready-made ranks: calib = the packed fp32 buffer of
        `view.calibration_matrices` on the image's device; the index build and the pooling run on the device.
        B samples at once: image [B, N, 3, H, W] with calib [B, N * 24 + 9] (`view.calibration_matrices_batched`) ->
        six maps [B, c, h, w]; a 1-D calib is the one-sample call, unchanged.  stereo_metas (a BEVStereo model only):
        view.stereo_metas(prev, None, ...) -- the current stride-4 features are this frame's own."""
        if calib.dim() == 2 and image.shape[0] != calib.shape[0]:
            raise ValueError(f"image holds {image.shape[0]} samples, calib {calib.shape[0]}")
        hip = self._bev_half_ready(image)
        # "hip" also takes the image half's dispatch by rule: two library convolutions of ResNet stage 4 that the shipped
        # table prefers are not run-to-run reproducible on the MI355X, and the frame's bits would differ between runs
        with _rule_dispatch() if hip else contextlib.nullcontext():
            x, skw = self._frame_features(image.flatten(0, 1), stereo_metas)
        return self.bev_half_calibrated(x, calib, hip, **skw)

    @torch.no_grad()
    def bev_half_calibrated(self, x, calib, hip=None, stereo_metas=None):
        """Everything of `forward_calibrated` behind `image_features`: x = its [cams, 256, H / 16, W / 16] result.
        hip = None: as `bev_half` and the tensors decide.  calib [B, N * 24 + 9]: x holds B * cams images.
        stereo_metas (a BEVStereo model): complete, cv_feat_list = [previous or None, current]."""
        skw = {} if stereo_metas is None else dict(stereo_metas=stereo_metas)
        if self._bev_half_ready(x) if hip is None else hip:
            with _rule_dispatch():
                return self._heads_hip(self.bev_encoder(self.view.view_transform_calibrated(x, calib, **skw)))
        return self._heads(self.view.view_transform_calibrated(x, calib, **skw))

    # ---- CenterHead.get_bboxes up to the NMS (centerpoint_head.py:716-746), configs/bevdet/bevdet-r50-cbgs.py:138-147
    @property
    def bbox_coder(self):
        from .postprocess import CenterPointBBoxCoder
        if getattr(self, "_bbox_coder", None) is None:
            self._bbox_coder = CenterPointBBoxCoder(**CENTERPOINT_CODER_R50)
        return self._bbox_coder

    def get_candidates(self, outputs, padded=False):
        """outputs = `forward`'s (reg, height, dim, rot, vel, heatmap): the top 500 heat-map cells decoded to boxes
        (x, y, z, w, l, h, yaw, vx, vy), those with score > 0.1 inside post_center_range kept -- the input of
        the rotated scale-NMS of CenterHead.get_task_detections (`get_bboxes`).  padded=True: (boxes
        [B, 500, 9], scores [B, 500], labels [B, 500] int32, count [B] int32) without a host synchronisation; else one
        {"bboxes", "scores", "labels"} per batch item, trimmed (labels float32, as the reference's)."""
        reg, height, dim, rot, vel, heatmap = outputs
        out = self.bbox_coder.decode_heads(reg, height, dim, rot, vel, heatmap, norm_bbox=True)
        if padded:
            return out
        from .postprocess import _dicts
        return _dicts(out, 9, torch.float32, heatmap.device)

    test_cfg = CENTERPOINT_TEST_CFG_R50

    def get_bboxes(self, outputs, padded=False):
        """CenterHead.get_bboxes (centerpoint_head.py:704-806) for the one task of the R50 configuration:
        `get_candidates`, then the NMS of `test_cfg` (rotated scale-NMS: threshold 0.2, per-class rescale factors,
        pre_max_size 1000, post_max_size 500; "circle" takes min_radius[0]), the size restore and z -= h / 2.
        padded=True: (boxes [B, 500, 9], scores [B, 500], labels [B, 500] int32, count [B] int32, index [B, 500] int32 =
        rows of `get_candidates(padded=True)`) without a host synchronisation, so the call can be captured; else one
        [bboxes [n, 9], scores [n], labels [n] int32] per batch item, as the reference returns them -- the boxes as a
        plain tensor: the `box_type_3d` wrapper class of the reference is not re-hosted.  A multi-task head would add
        its class offset to the labels (centerpoint_head.py:800-804); that bookkeeping is the caller's."""
        from .functions.nms import bev_nms
        cfg = self.test_cfg
        boxes, scores, labels, count = self.get_candidates(outputs, padded=True)
        circle = cfg["nms_type"] == "circle"
        out = bev_nms(boxes, scores, labels, count, nms_type=cfg["nms_type"],
                      threshold=cfg["min_radius"][0] if circle else cfg["nms_thr"],
                      pre_max_size=None if circle else cfg["pre_max_size"],
                      post_max_size=min(cfg["post_max_size"], boxes.shape[1]),
                      rescale_factor=None if circle else cfg.get("nms_rescale_factor"), bottom_center=True, padded=True)
        if padded:
            return out
        return [[out[0][b, :n], out[1][b, :n], out[2][b, :n]] for b, n in enumerate(out[3].tolist())]


class BEVDetRunner:
    """Frame loop of tools/bevdet/evaluate_trt.py:107-140 with the calibration as a per-FRAME input, the BEVDet
    counterpart of bevformer.FrameRunner: `step` computes the small matrices of the frame's calibration on the host
    (`calibration_matrices`), copies them into ONE static device buffer (N * 24 + 9 floats: 612 bytes for six cameras)
    and, with graph=True, replays ONE captured HIP graph that holds the index build, the whole forward and -- post =
    "candidates" / "bboxes" -- `get_candidates` / `get_bboxes` in their padded forms.  Inside `step` there is no host
    synchronisation, and a changed calibration needs no new capture.  The upload goes through a small ring of pinned
    host buffers (an asynchronous copy; a pageable source would make the copy wait for the previous frame): the host
    only waits when it is a whole ring of frames ahead of the device.

    raw_size=(H0, W0) adds `step_raw`: the frame from the RAW camera images.  The test branch of PrepareImageInputs
    (loading.py:747-792: PIL's resize, crop, flip; mmlabNormalize) then runs as the first launch of a second captured
    graph (functions.image_resize_crop_normalize, bit-exact to PIL), reading the static uint8 `raw_buffer` and writing
    `image_buffer`; flip / scale are sample_augmentation's arguments, data_config defaults to DATA_CONFIG_R50 with
    the model's input size.  `step` is unchanged and keeps its own graph, so a runner on which both `step` and
    `step_raw` are called holds two graphs and the frame's activations twice (see `step_raw`).

    batch=B > 1 (fixed at construction) runs B samples per graph: `step` / `step_raw` take a leading B on the image
    [B, cams, 3, H, W] (raw frames [B, cams, H0, W0, 3]) and on every calibration tensor; the static buffers are
    [B, cams, 3, H, W], [B * cams, H0, W0, 3] and calib [B, cams * 24 + 9]; still one upload through the ring and one
    graph per entry point; the maps come back as [B, c, h, w], the padded post-processing as [B, 500, ...] and count
    [B].  Another B raises ValueError.  batch=1 is the runner described above, unchanged."""
    RING = 4

    def __init__(self, model, device, graph=True, post=None, clone_outputs=True, raw_size=None, flip=None, scale=None,
                 data_config=None, batch=1):
        if post not in (None, "candidates", "bboxes"):
            raise ValueError(f"post = {post!r}: None, 'candidates' or 'bboxes'")
        if int(batch) != batch or batch < 1:
            raise ValueError(f"batch = {batch!r}: a positive integer")
        self.batch = int(batch)
        self.model, self.device, self.use_graph, self.post, self.clone_outputs = model, device, graph, post, clone_outputs
        dtype = next(model.parameters()).dtype
        H, W = view_input_size(model.view)
        self.n_cams = None
        self._image_shape, self._dtype = (3, H, W), dtype
        self._in, self._graph, self._outs = None, None, None
        self._ring, self._frame = None, 0
        self.raw_size, self._graph_raw, self._outs_raw = None, None, None
        if raw_size is not None:
            from .functions.image import bevdet_test_augmentation, bevdet_post_transform, image_resize_plan
            self.raw_size = (int(raw_size[0]), int(raw_size[1]))
            cfg = dict(DATA_CONFIG_R50 if data_config is None else data_config)
            if data_config is None:
                cfg["input_size"] = (H, W)
            if tuple(cfg["input_size"]) != (H, W):
                raise ValueError(f"data_config['input_size'] = {cfg['input_size']}, the model takes {(H, W)}")
            self.resize, self.resize_dims, self.crop, self.flip, rotate = bevdet_test_augmentation(
                *self.raw_size, cfg, flip=flip, scale=scale)
            self._plan = image_resize_plan(*self.raw_size, self.resize_dims, self.crop, device)
            self.post_rot, self.post_tran = bevdet_post_transform(self.resize, self.crop, self.flip)

    @property
    def image_buffer(self):
        """The static [batch, cams, 3, H, W] input buffer (after the first `step`): a caller that writes its images here
        and passes this very tensor to `step` saves the per-frame copy."""
        return None if self._in is None else self._in["image"]

    @property
    def raw_buffer(self):
        """The static [batch * cams, H0, W0, 3] uint8 buffer `step_raw` reads (after its first call): a caller that decodes its
        camera frames into it and passes this very tensor to `step_raw` saves the per-frame copy."""
        return None if self._in is None else self._in.get("raw")

    def _forward(self, raw=False):
        if raw:
            fn = getattr(self.model.ops, "image_resize_crop_normalize", _hip_ops.image_resize_crop_normalize)
            fn(self._in["raw"], self._plan, flip=self.flip, out=self._in["image"].flatten(0, 1))
        out = self.model.forward_calibrated(self._in["image"], self._in["calib"])
        if self.post == "candidates":
            return out + tuple(self.model.get_candidates(out, padded=True))
        if self.post == "bboxes":
            return out + tuple(self.model.get_bboxes(out, padded=True))
        return out

    def _capture(self, raw=False):
        graph, outs = capture(lambda: self._forward(raw))
        if raw:
            self._graph_raw, self._outs_raw = graph, outs
        else:
            self._graph, self._outs = graph, outs

    def step_raw(self, raw, sensor2ego, ego2global, cam2imgs, bda):
        """`step` from the RAW camera images [cams, H0, W0, 3] uint8 RGB on the device (raw_size=(H0, W0) at
        construction): resize, crop, flip and normalisation run on the device as the first launch of the frame's graph,
        post_rots / post_trans are the ones that augmentation implies (`bevdet_post_transform`).

        `step_raw` replays a captured graph of its own, whose activation pool lies beside that of `step`'s graph: a
        runner on which BOTH entry points are called holds the frame's activations twice.  A graph is captured at the
        first call of its entry point, so a runner that only ever calls one of them pays for one."""
        if self.raw_size is None:
            raise RuntimeError("step_raw needs BEVDetRunner(..., raw_size=(H0, W0))")
        n, B = sensor2ego.shape[1], self.batch
        lead = (n,) if B == 1 else (B, n)
        if raw.dtype != torch.uint8 or tuple(raw.shape) != lead + self.raw_size + (3,):
            raise ValueError(f"raw must be uint8 {list(lead) + [self.raw_size[0], self.raw_size[1], 3]}")
        post_rots = self.post_rot.view(1, 1, 3, 3).repeat(B, n, 1, 1)
        post_trans = self.post_tran.view(1, 1, 3).repeat(B, n, 1)
        host = self._host_calib(sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda)
        return self._run_frame("raw", raw, host, n)

    def _host_calib(self, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        """The packed host buffer of the frame: 1-D at batch 1, [B, cams * 24 + 9] otherwise."""
        B = self.batch
        if any(t.shape[0] != B for t in (sensor2ego, cam2imgs, post_rots, post_trans, bda)):
            raise ValueError(f"this runner was built for batch = {B}: every calibration tensor carries that leading B")
        if B == 1:
            return self.model.view.calibration_matrices(sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda)
        return self.model.view.calibration_matrices_batched(sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda)

    def step(self, image, sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda):
        """-> (reg, height, dim, rot, vel, heatmap) of `BEVDet.forward`, followed by the padded outputs of
        `get_candidates` (post="candidates") or `get_bboxes` (post="bboxes")."""
        host = self._host_calib(sensor2ego, ego2global, cam2imgs, post_rots, post_trans, bda)
        if image.shape[0] != self.batch:
            raise ValueError(f"this runner was built for batch = {self.batch}, the image holds {image.shape[0]} samples")
        return self._run_frame("image", image, host, sensor2ego.shape[1])

    def _run_frame(self, key, source, host, n_cams):
        """The shared tail of `step` (key = "image") and `step_raw` (key = "raw"): `source` into its static buffer, the
        calibration upload, the replay of that entry point's graph."""
        if self._in is None:
            self.n_cams = n_cams
            self._in = dict(image=torch.zeros((self.batch, self.n_cams) + self._image_shape, device=self.device,
                                              dtype=self._dtype),
                            calib=torch.zeros(host.shape, device=self.device))
            self._ring = [(torch.zeros(host.shape).pin_memory(), torch.cuda.Event()) for _ in range(self.RING)]
            if self.raw_size is not None:
                self._in["raw"] = torch.zeros((self.batch * self.n_cams,) + self.raw_size + (3,), device=self.device,
                                              dtype=torch.uint8)
        i = self._in
        if host.numel() != i["calib"].numel():
            raise ValueError("the number of cameras is fixed by the first frame")
        if source.data_ptr() != i[key].data_ptr():          # (the caller may have filled the static buffer itself)
            i[key].copy_(source.reshape(i[key].shape), non_blocking=True)
        staged, done = self._ring[self._frame % self.RING]
        self._frame += 1
        done.synchronize()                                  # (returns at once unless the host is RING frames ahead)
        staged.copy_(host)
        with torch.cuda.device(self.device):
            i["calib"].copy_(staged, non_blocking=True)     # one upload
            done.record()
        raw = key == "raw"
        if not self.use_graph:
            return self._forward(raw)
        if (self._graph_raw if raw else self._graph) is None:
            self._capture(raw)
        graph, outs = (self._graph_raw, self._outs_raw) if raw else (self._graph, self._outs)
        graph.replay()
        return tuple(t.clone() for t in outs) if self.clone_outputs else outs


def synthetic_rig(view, n_cams=6, seed=0):
    """A plausible six-camera calibration for timing and tests (no nuScenes data here): cameras on a ring, 60 degrees
    apart, looking outwards, the resize / crop augmentation of the test pipeline as post_rots / post_trans.
    Returns the six tensors of LSSViewTransformer.get_bev_pool_input."""
    import math
    H, W = view_input_size(view)
    s2e = torch.zeros(1, n_cams, 4, 4)
    for i in range(n_cams):
        yaw = math.radians(60.0 * i)
        # camera axes (x right, y down, z forward) in the ego frame (x forward, y left, z up)
        fwd = torch.tensor([math.cos(yaw), math.sin(yaw), 0.0])
        right = torch.tensor([math.sin(yaw), -math.cos(yaw), 0.0])
        down = torch.tensor([0.0, 0.0, -1.0])
        s2e[0, i, :3, 0], s2e[0, i, :3, 1], s2e[0, i, :3, 2] = right, down, fwd
        s2e[0, i, :3, 3] = torch.tensor([1.5 * math.cos(yaw), 1.5 * math.sin(yaw), 1.6])
        s2e[0, i, 3, 3] = 1.0
    e2g = torch.eye(4).view(1, 1, 4, 4).repeat(1, n_cams, 1, 1)
    K = torch.tensor([[1266.0, 0.0, 800.0], [0.0, 1266.0, 450.0], [0.0, 0.0, 1.0]]).view(1, 1, 3, 3).repeat(1, n_cams, 1, 1)
    scale = W / 1600.0
    post_rots = (torch.eye(3) * scale).view(1, 1, 3, 3).repeat(1, n_cams, 1, 1)
    post_rots[..., 2, 2] = 1.0
    post_trans = torch.zeros(1, n_cams, 3)
    post_trans[..., 1] = -(900.0 * scale - H)
    bda = torch.eye(3).view(1, 3, 3)
    return s2e, e2g, K, post_rots, post_trans, bda


def jittered_rig(view, seed, n_cams=6):
    """`synthetic_rig` perturbed the way real BEVDet input varies from sample to sample: camera translation and
    focal length (another vehicle), a yawed, scaled and possibly flipped `bda` (the per-sample BEV augmentation), a
    resize and crop offset in post_rots / post_trans (the per-image augmentation).  Deterministic in `seed`."""
    import math
    s2e, e2g, K, post_rots, post_trans, bda = synthetic_rig(view, n_cams)
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    s2e[0, :, :3, 3] += 0.05 * r(n_cams, 3)
    K[0, :, 0, 0] *= 1 + 0.02 * r(n_cams)
    K[0, :, 1, 1] = K[0, :, 0, 0]
    K[0, :, :2, 2] += 5.0 * r(n_cams, 2)
    post_rots[0, :, :2, :2] *= (1 + 0.06 * r(n_cams)).view(n_cams, 1, 1)
    post_trans[0, :, 0] -= 10.0 * (1 + r(n_cams))
    post_trans[0, :, 1] += 4.0 * r(n_cams)
    yaw, scale = math.radians(22.5) * float(r(1)), 1 + 0.05 * float(r(1))
    rot = torch.tensor([[math.cos(yaw), -math.sin(yaw), 0.0], [math.sin(yaw), math.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    flip = torch.diag(torch.tensor([-1.0 if seed % 2 else 1.0, -1.0 if seed % 3 == 0 else 1.0, 1.0]))
    bda = (flip @ (rot * scale)).view(1, 3, 3)
    return s2e, e2g, K, post_rots, post_trans, bda


def view_input_size(view):
    """(H, W) of the camera images the frustum of `view` was built for."""
    x, y = view.frustum[0, 0, :, 0], view.frustum[0, :, 0, 1]
    return int(round(float(y[-1]))) + 1, int(round(float(x[-1]))) + 1
