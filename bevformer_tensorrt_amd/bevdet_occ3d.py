"""The 3-D BEV half of BEVDet-Occ (BEVDetOCC with LSSViewTransformer(collapse_z=False), CustomResNet3D, LSSFPN3D and a 3-D
final_conv; bevdet.BEVDET_OCC_R50, design/conv3d.md).  Imported by bevdet.BEVDet only for cfg bev_encoder="3d".  The
reference tree has no BEVDet-Occ code or config: module names and values are recalled from the BEVDet library, parity
with it is unpinned.

Every BatchNorm3d is folded into the convolution in front of it (checkpoint.occ3d_key_map), as the 2-D blocks keep theirs.
Two data paths through the same weights: hip (fp16 channels-last volumes on functions.conv3d_taps, every layer ONE launch
of bevops_conv3d_slice_f16, level 0 writing its slice of LSSFPN3D's concatenation buffer) and the torch statements
(functions.conv3d_plain: F.conv3d, any device / dtype).  The two trilinear up-samplings stay F.interpolate on both paths."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functions as _hip_ops
from .functions.conv3d import conv3d_plain, conv3d_taps_weight, ndhwc_empty

NUM_LAYER, STRIDES = (1, 2, 4), (1, 2, 2)


class BasicBlock3D(nn.Module):
    """conv3 + BN + ReLU, conv3 + BN, identity (a strided 3 x 3 x 3 conv + BN where stride or width changes), ReLU."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv3d(cin, cout, 3, stride, 1), nn.Conv3d(cout, cout, 3, 1, 1)
        self.downsample = nn.Conv3d(cin, cout, 3, stride, 1) if (stride != 1 or cin != cout) else None


class BEVEncoderOcc3D(nn.Module):
    """CustomResNet3D (num_layer [1, 2, 4], channels [c, 2c, 4c], strides [1, 2, 2]) + LSSFPN3D (levels 1 and 2 up-sampled
    x 2 and x 4, concatenated with level 0 to 7c channels, 1 x 1 x 1 conv + BN + ReLU to c) + final_conv (3 x 3 x 3, bias,
    ReLU) + predicter Linear(c, hidden) + Softplus + Linear(hidden, classes), one row per voxel."""

    def __init__(self, c, dz, num_classes, hidden):
        super().__init__()
        self.c, self.dz, self.num_classes = c, dz, num_classes
        stages, cin = [], c
        for n, mult, s in zip(NUM_LAYER, (1, 2, 4), STRIDES):
            stages.append(nn.ModuleList([BasicBlock3D(cin if j == 0 else c * mult, c * mult, s if j == 0 else 1)
                                         for j in range(n)]))
            cin = c * mult
        self.stages = nn.ModuleList(stages)
        self.fpn_conv = nn.Conv3d(7 * c, c, 1)
        self.final_conv = nn.Conv3d(c, c, 3, 1, 1)
        self.predicter = nn.Sequential(nn.Linear(c, hidden), nn.Softplus(), nn.Linear(hidden, num_classes))

    def convs(self):
        return [m for m in self.modules() if isinstance(m, nn.Conv3d)]

    def prepare(self, build=True):
        """The taps-major operands of every convolution (functions.conv3d_taps_weight's cache).  build=False: False when
        one is missing or stale.  Building allocates: never under capture."""
        return all(conv3d_taps_weight(m.weight, build=build) is not None for m in self.convs())

    def _conv(self, ops, hip, x, conv, act, residual=None, out=None):
        if hip:
            return ops.conv3d_taps(x, conv3d_taps_weight(conv.weight), conv.bias, act, residual, conv.stride[0], out)
        return conv3d_plain(x, conv.weight, conv.bias, act, residual, conv.stride[0])

    def _block(self, ops, hip, x, blk, out=None):
        idt = x if blk.downsample is None else self._conv(ops, hip, x, blk.downsample, "none")
        return self._conv(ops, hip, self._conv(ops, hip, x, blk.conv1, "relu"), blk.conv2, "relu", idt, out)

    def encode(self, pooled, ops, hip, levels=None):
        """pooled [B, c, Dz * Dy, Dx] (the pooling's map with out_height = Dz * Dy: the volume, no collapse) -> final_conv's
        [B, c, Dz, Dy, Dx].  levels: a list that receives the three backbone levels."""
        B, c, H, X = pooled.shape
        vol = pooled.reshape(B, c, self.dz, H // self.dz, X)         # (a view of either layout)
        cat = ndhwc_empty(B, 7 * c, *vol.shape[2:], vol.device, vol.dtype) if hip else None
        feats, x = [], vol
        for s, stage in enumerate(self.stages):
            for j, blk in enumerate(stage):
                last0 = hip and s == 0 and j == len(stage) - 1       # level 0 writes its slice of the concatenation
                x = self._block(ops, hip, x, blk, cat[:, :c] if last0 else None)
            feats.append(x)
        if levels is not None:
            levels.extend(feats)
        ups = [F.interpolate(f, size=vol.shape[2:], mode="trilinear", align_corners=True) for f in feats[1:]]
        if hip:
            cat[:, c:3 * c].copy_(ups[0])
            cat[:, 3 * c:].copy_(ups[1])
        else:
            cat = torch.cat([feats[0]] + ups, dim=1)
        return self._conv(ops, hip, self._conv(ops, hip, cat, self.fpn_conv, "relu"), self.final_conv, "relu")

    def head_weights(self):
        p = self.predicter
        return p[0].weight, p[0].bias, p[2].weight, p[2].bias, 1, self.num_classes

    def head(self, y, ops, packed=None, logits=False):
        """y = `encode`'s volume -> occ [B, Dx, Dy, Dz] uint8, the axis order FLASHOCC_R50 returns (and, logits=True, the
        pre-arg-max logits [B, Dz, Dy, Dx, classes]).  packed = functions.pack_occ_head of `head_weights`: functions.
        occ_head_nhwc with one row per voxel, one launch per sample that writes the permuted bytes itself; None: the torch
        statement (functions.occ_head_plain)."""
        B, c, Dz, Dy, Dx = y.shape
        if packed is None:
            occ, lg = _hip_ops.occ_head_plain(y.reshape(B, c, Dz * Dy, Dx), *self.head_weights(), logits=True)
            occ = occ.view(B, Dz, Dy, Dx).permute(0, 3, 2, 1).contiguous()
            return (occ, lg.view(B, Dz, Dy, Dx, -1)) if logits else occ
        y = y.contiguous(memory_format=torch.channels_last_3d)
        occ = torch.empty((B, Dx, Dy, Dz), dtype=torch.uint8, device=y.device)
        lg = torch.empty((B, Dz, Dy, Dx, self.num_classes), dtype=torch.float16, device=y.device) if logits else None
        for b in range(B):             # the z planes of a sample as the launch's images: [Dz, c, Dy, Dx] channels-last
            ops.occ_head_nhwc(y[b].permute(1, 0, 2, 3), packed, logits=lg[b] if logits else False,
                              out=occ[b].permute(2, 1, 0).unsqueeze(-1))
        return (occ, lg) if logits else occ
