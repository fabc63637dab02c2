"""BEVStereo's temporal-stereo cost volume (csrc/stereo_cost.hip; the reference's DepthNet.gen_grid and
calculate_cost_volumn, third_party/bev_mmdet3d/models/necks/view_transformer.py:613-678).  Not reference plugins
(TensorRT owns these layers there), so none is in TRT_FUNCTIONS.

  * `stereo_calibration`  the per-camera constants of the warp grid, [n, 40] fp32 on the CPU: the two inversions stay on
                          the host in torch fp32, as `calibration_matrices` keeps its own;
  * `stereo_frustum_tables`  the three axes (xs [Wc], ys [Hc], ds [D]) of a `create_frustum(..., downsample=4)` volume;
  * `stereo_grid`         gen_grid: the reference's op sequence in torch for CPU tensors, bevops_stereo_grid for CUDA ones;
  * `stereo_cost_volume`  fp16 channels-last CUDA tensors take the one launch (bevops_stereo_cost_volume_f16), anything
                          else the reference's op sequence in torch (`stereo_cost_volume_plain`).

The launch allocates a fixed-size output and never synchronises: it can be captured."""
import torch
import torch.nn.functional as F

from ..utils import lib as _lib
from .linear import _call
from .yolox_ops import _dest, slice_pitch

STEREO_CONSTS = 40          # floats per camera
STEREO_MAX_D = 128
GROUP_SIZE = 4              # calculate_cost_volumn's channel groups
CV_DOWNSAMPLE = 4           # the stride of the stereo feature map: gen_grid normalises by (4 Hc, 4 Wc).  The one Python
                            # name of it (bevdepth.py imports it); csrc/stereo_cost.hip states it as kStCvDown


def stereo_calibration(k2s_sensor, intrins, post_rots, post_trans):
    """k2s_sensor [..., 4, 4], intrins [..., 3, 3], post_rots [..., 3, 3], post_trans [..., 3] (any leading camera
    dimensions, flattened to n) -> [n, 40] fp32 on the CPU:
    inverse(post_rots) 9 | post_trans 3 | k2s_R @ inverse(intrins) 9 | k2s_t 3 | intrins 9 | post_rots[:2,:2] 4 |
    post_trans[:2] 2 | 0.  The inversions and the product are the reference's torch fp32 ops, evaluated on the CPU."""
    k2s, K, pr, pt = (t.detach().to("cpu", torch.float32) for t in (k2s_sensor, intrins, post_rots, post_trans))
    k2s, K, pr, pt = k2s.reshape(-1, 4, 4), K.reshape(-1, 3, 3), pr.reshape(-1, 3, 3), pt.reshape(-1, 3)
    n = K.shape[0]
    if not (k2s.shape[0] == pr.shape[0] == pt.shape[0] == n):
        raise ValueError("stereo_calibration: one k2s_sensor, intrins, post_rots and post_trans per camera")
    rots = k2s[:, :3, :3].contiguous()
    trans = k2s[:, :3, 3].contiguous()
    combine = rots.matmul(torch.inverse(K))
    parts = [torch.inverse(pr).reshape(n, 9), pt, combine.reshape(n, 9), trans, K.reshape(n, 9),
             pr[:, :2, :2].reshape(n, 4), pt[:, :2], torch.zeros(n, 1)]
    out = torch.cat(parts, dim=1).contiguous()
    assert out.shape == (n, STEREO_CONSTS)
    return out


def stereo_frustum_tables(frustum):
    """frustum [D, Hc, Wc, 3] as create_frustum builds it (x along W, y along H, d along D) -> (xs [Wc], ys [Hc], ds [D])
    fp32 contiguous, on the frustum's device."""
    if frustum.dim() != 4 or frustum.shape[-1] != 3:
        raise ValueError(f"stereo_frustum_tables: a [D, Hc, Wc, 3] frustum, got {tuple(frustum.shape)}")
    f = frustum.detach().to(torch.float32)
    return f[0, 0, :, 0].contiguous(), f[0, :, 0, 1].contiguous(), f[:, 0, 0, 2].contiguous()


def _tables(frustum_tables, device):
    xs, ys, ds = frustum_tables
    for t in (xs, ys, ds):
        if not (torch.is_tensor(t) and t.dim() == 1 and t.dtype == torch.float32 and t.is_contiguous() and t.device == device):
            raise ValueError(f"stereo: frustum tables (xs [Wc], ys [Hc], ds [D]) contiguous fp32 on {device}")
    return xs, ys, ds


def stereo_grid_plain(consts, frustum_tables):
    """gen_grid in torch, the reference's op sequence on its operands of `stereo_calibration` (the host-side inversions
    are part of the constants): -> [n, D, Hc, Wc, 2], normalised by the image the stride-4 map stands for."""
    xs, ys, ds = frustum_tables
    n = consts.shape[0]
    D, H, W = ds.numel(), ys.numel(), xs.numel()
    hi, wi = H * CV_DOWNSAMPLE, W * CV_DOWNSAMPLE
    c = consts.view(1, n, STEREO_CONSTS)
    frustum = torch.stack((xs.view(1, 1, W).expand(D, H, W), ys.view(1, H, 1).expand(D, H, W),
                           ds.view(D, 1, 1).expand(D, H, W)), -1)
    points = frustum - c[..., 9:12].view(1, n, 1, 1, 1, 3)
    points = c[..., 0:9].reshape(1, n, 1, 1, 1, 3, 3).matmul(points.unsqueeze(-1))
    points = torch.cat((points[..., :2, :] * points[..., 2:3, :], points[..., 2:3, :]), 5)
    points = c[..., 12:21].reshape(1, n, 1, 1, 1, 3, 3).matmul(points)
    points += c[..., 21:24].reshape(1, n, 1, 1, 1, 3, 1)
    neg_mask = points[..., 2, 0] < 1e-3
    points = c[..., 24:33].reshape(1, n, 1, 1, 1, 3, 3).matmul(points)
    points = points[..., :2, :] / points[..., 2:3, :]
    points = c[..., 33:37].reshape(1, n, 1, 1, 1, 2, 2).matmul(points).squeeze(-1)
    points += c[..., 37:39].reshape(1, n, 1, 1, 1, 2)
    px = points[..., 0] / (wi - 1.0) * 2.0 - 1.0
    py = points[..., 1] / (hi - 1.0) * 2.0 - 1.0
    px[neg_mask] = -2
    py[neg_mask] = -2
    return torch.stack([px, py], dim=-1).view(n, D, H, W, 2)


def stereo_grid(consts, frustum_tables, out=None):
    """consts [n, 40] fp32 (`stereo_calibration`), frustum_tables (xs [Wc], ys [Hc], ds [D]) on the same device ->
    the warp grid [n, D, Hc, Wc, 2] fp32.  CPU: `stereo_grid_plain`.  CUDA: bevops_stereo_grid, one launch, the device
    function the fused cost-volume launch evaluates when it is given the constants instead of a grid."""
    if not (torch.is_tensor(consts) and consts.dim() == 2 and consts.shape[1] == STEREO_CONSTS and
            consts.dtype == torch.float32 and consts.is_contiguous()):
        raise ValueError(f"stereo_grid: consts a contiguous fp32 [n, {STEREO_CONSTS}] tensor")
    xs, ys, ds = _tables(frustum_tables, consts.device)
    if not consts.is_cuda:
        return stereo_grid_plain(consts, (xs, ys, ds))
    n, D, H, W = consts.shape[0], ds.numel(), ys.numel(), xs.numel()
    if not 1 <= D <= STEREO_MAX_D:
        raise _lib.BevopsError(f"bevops_stereo_grid: 1 <= D <= {STEREO_MAX_D}", _lib.NOT_SUPPORTED)
    shape = (n, D, H, W, 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=consts.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != consts.device:
        raise ValueError(f"stereo_grid: out a contiguous fp32 {shape} tensor on the constants' device")
    if n and H * W:
        _call("bevops_stereo_grid", consts.device, consts.data_ptr(), xs.data_ptr(), ys.data_ptr(), ds.data_ptr(),
              out.data_ptr(), n, D, H, W)
    return out


def stereo_cost_volume_plain(prev, curr, grid, bias):
    """calculate_cost_volumn behind gen_grid, the reference's op sequence: prev, curr [n, C, Hc, Wc], grid
    [n, D, Hc, Wc, 2] -> [n, D, Hc, Wc] in curr's dtype.  The channels are taken in groups of four; the reference drops
    C % 4 trailing channels silently, this statement does the same (the launch refuses such a C)."""
    n, _, H, W = curr.shape
    D = grid.shape[1]
    grid = grid.to(curr.dtype).view(n, D * H, W, 2)
    cost_volumn = 0
    wrap_prev = None
    for fid in range(curr.shape[1] // GROUP_SIZE):
        prev_curr = prev[:, fid * GROUP_SIZE:(fid + 1) * GROUP_SIZE, ...]
        wrap_prev = F.grid_sample(prev_curr, grid, align_corners=True, padding_mode="zeros")
        curr_tmp = curr[:, fid * GROUP_SIZE:(fid + 1) * GROUP_SIZE, ...]
        cost_volumn_tmp = curr_tmp.unsqueeze(2) - wrap_prev.view(n, -1, D, H, W)
        cost_volumn_tmp = cost_volumn_tmp.abs().sum(dim=1)
        cost_volumn = cost_volumn + cost_volumn_tmp
    if wrap_prev is None:
        raise ValueError("stereo_cost_volume: fewer than four channels")
    if not bias == 0:
        invalid = wrap_prev[:, 0, ...].view(n, D, H, W) == 0
        cost_volumn[invalid] = cost_volumn[invalid] + bias
    cost_volumn = -cost_volumn
    return cost_volumn.softmax(dim=1)


def _is_fast(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16 and t.dim() == 4


def stereo_cost_volume(prev, curr, grid_or_consts, D, bias, frustum_tables=None, out=None, dpad=None):
    """softmax over d of -(sum_c |curr - warp(prev)| + bias [gate == 0]), gate = the warped channel C - 4.

    prev, curr [n, C, Hc, Wc]; grid_or_consts either the grid [n, D, Hc, Wc, 2] fp32 (`stereo_grid`) or the constants
    [n, 40] fp32 (`stereo_calibration`, with `frustum_tables`: the grid is then computed inside the launch / by
    `stereo_grid_plain`).  prev None (the first frame): zeros.

    fp16 CUDA channel slices of channels-last tensors take ONE launch and return a channels-last [n, dpad, Hc, Wc]
    fp16 tensor (dpad: D rounded up to 8 when not given; columns D .. dpad exact zeros; `out`: a channel slice to
    write).  Anything else: the reference's op sequence in torch, [n, D, Hc, Wc] in curr's dtype."""
    D, bias = int(D), float(bias)
    if not torch.is_tensor(curr) or curr.dim() != 4:
        raise ValueError("stereo_cost_volume: curr a [n, C, Hc, Wc] tensor")
    n, C, H, W = curr.shape
    fast = _is_fast(curr) and (prev is None or _is_fast(prev))
    if fast:
        dpad = (D + 7) // 8 * 8 if dpad is None else int(dpad)
    if prev is None:
        if fast:
            out = _dest(out, (n, dpad, H, W), curr, "stereo_cost_volume")
            out.zero_()
            return out
        return curr.new_zeros((n, D, H, W))
    if tuple(prev.shape) != tuple(curr.shape) or prev.dtype != curr.dtype or prev.device != curr.device:
        raise ValueError("stereo_cost_volume: prev and curr of one shape, dtype and device")
    g = grid_or_consts
    if not (torch.is_tensor(g) and g.dtype == torch.float32 and g.is_contiguous() and g.device == curr.device):
        raise ValueError("stereo_cost_volume: the grid / the constants a contiguous fp32 tensor on the features' device")
    is_grid = g.dim() == 5
    if is_grid:
        if tuple(g.shape) != (n, D, H, W, 2):
            raise ValueError(f"stereo_cost_volume: grid {(n, D, H, W, 2)}, got {tuple(g.shape)}")
    else:
        if tuple(g.shape) != (n, STEREO_CONSTS) or frustum_tables is None:
            raise ValueError(f"stereo_cost_volume: constants [n, {STEREO_CONSTS}] come with frustum_tables")
        xs, ys, ds = _tables(frustum_tables, curr.device)
        if (xs.numel(), ys.numel(), ds.numel()) != (W, H, D):
            raise ValueError("stereo_cost_volume: frustum tables of (Wc, Hc, D) values")
    if not fast:
        grid = g if is_grid else stereo_grid_plain(g, (xs, ys, ds))
        return stereo_cost_volume_plain(prev, curr, grid, bias)
    if C % 8:
        raise _lib.BevopsError("bevops_stereo_cost_volume_f16: C % 8 == 0 (the reference drops C % 4 trailing channels; "
                               "this entry refuses)", _lib.NOT_SUPPORTED)
    if not 1 <= D <= STEREO_MAX_D or dpad % 8 or dpad < D:
        raise _lib.BevopsError(f"bevops_stereo_cost_volume_f16: 1 <= D <= {STEREO_MAX_D}, dpad % 8 == 0, dpad >= D",
                               _lib.NOT_SUPPORTED)
    pp, cp = slice_pitch(prev, "prev"), slice_pitch(curr, "curr")
    out = _dest(out, (n, dpad, H, W), curr, "stereo_cost_volume")
    op = slice_pitch(out, "out")
    if n and H * W:
        ptrs = (g.data_ptr(), None, None, None, None) if is_grid else (None, g.data_ptr(), xs.data_ptr(), ys.data_ptr(), ds.data_ptr())
        _call("bevops_stereo_cost_volume_f16", curr.device, prev.data_ptr(), pp, curr.data_ptr(), cp, *ptrs, out.data_ptr(),
              op, n, H, W, C, D, dpad, bias)
    return out
