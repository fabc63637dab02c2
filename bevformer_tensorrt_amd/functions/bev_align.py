"""BEVDet4D's temporal BEV alignment and stacking (csrc/bev_align.hip; gen_grid / shift_feature of BEVDet4D as
recalled: the reference tree has no BEVDet4D code, see design/bevdet4d.md).  Not reference plugins, so none is in
TRT_FUNCTIONS.

  * `bev_align_transform`   the affine map from a pixel of the current BEV map to the pixel of a past frame's map,
                            [B, 2, 3] fp32 on the CPU: the inversions stay on the host in torch fp32, as
                            `calibration_matrices` keeps its own;
  * `pack_bev_align_meta`   the per-frame buffer of the launch (include/bevops.h fixes its layout), built on the host;
  * `bev_align_stack`       fp16 channels-last CUDA tensors take the one launch (bevops_bev_align_stack_f16): the current
                            map, the T aligned past maps behind it on the channel axis, and the current map kept in the
                            ring's free slot.  int8 channels-last CUDA tensors take the int8 launch
                            (bevops_bev_align_stack_s8: 16 channels per lane, bytes in, bytes out, no scale: static PTQ
                            scales and a convex blend keep the ring, the stack and curr in ONE scale).  int8 anywhere
                            else: `bev_align_stack_q_plain`, the exact statement of that launch.  Anything else:
                            `bev_align_stack_plain`, the same positions, then F.grid_sample, the copies and the cat.

The launch allocates a fixed-size output and never synchronises: it can be captured; `meta` is a static device buffer
the host rewrites between replays."""
import torch
import torch.nn.functional as F

from ..utils import lib as _lib
from .linear import _call
from .yolox_ops import _dest, slice_pitch

BEV_ALIGN_MAX_T = 15
META_HEAD, META_ENTRY = 4, 8      # 4-byte words: [write_slot, 0, 0, 0], then per (b, t) [slot, valid, a00 a01 a02 a10 a11 a12]


def bev_align_meta_words(B, T):
    return META_HEAD + META_ENTRY * int(B) * int(T)


def bev_align_transform(sensor2ego_curr, ego2global_curr, sensor2ego_prev, ego2global_prev, bda, grid_lower_bound,
                        grid_interval):
    """sensor2ego_* / ego2global_* [B, N, 4, 4] of the current and of a past frame, bda [B, 3, 3], the BEV grid's lower
    bound and cell size (x, y first) -> [B, 2, 3] fp32 on the CPU: rows 0 and 1 of the map that takes the pixel (x, y, 1)
    of the CURRENT feature map to the pixel of the PAST frame's map showing the same place.  BEVDet4D's gen_grid in torch
    fp32 in its order, camera 0 only: s2k = inverse(ego2global_curr) . ego2global . sensor2ego for either frame,
    c02l0 = bda4 . s2k_curr, c12l0 = bda4 . s2k_prev, l02l1 = c02l0 . inverse(c12l0) without row and column z,
    tf = inverse(feat2bev) . l02l1 . feat2bev."""
    s2e_c, e2g_c, s2e_p, e2g_p, bda = (t.detach().to("cpu", torch.float32) for t in
                                       (sensor2ego_curr, ego2global_curr, sensor2ego_prev, ego2global_prev, bda))
    B = s2e_c.shape[0]
    if any(t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (4, 4) for t in (s2e_c, e2g_c, s2e_p, e2g_p)) \
            or tuple(bda.shape) != (B, 3, 3):
        raise ValueError("bev_align_transform: sensor2ego / ego2global [B, N, 4, 4] of both frames and bda [B, 3, 3]")
    lower, interval = (torch.as_tensor(t, dtype=torch.float32).cpu() for t in (grid_lower_bound, grid_interval))
    key_inv = torch.inverse(e2g_c[:, 0])
    s2k_c = key_inv.matmul(e2g_c[:, 0]).matmul(s2e_c[:, 0])
    s2k_p = key_inv.matmul(e2g_p[:, 0]).matmul(s2e_p[:, 0])
    bda4 = torch.zeros(B, 4, 4)
    bda4[:, :3, :3] = bda
    bda4[:, 3, 3] = 1
    c02l0, c12l0 = bda4.matmul(s2k_c), bda4.matmul(s2k_p)
    l02l1 = c02l0.matmul(torch.inverse(c12l0))
    keep = [0, 1, 3]
    l02l1 = l02l1[:, keep][:, :, keep]
    feat2bev = torch.zeros(3, 3)
    feat2bev[0, 0], feat2bev[1, 1] = interval[0], interval[1]
    feat2bev[0, 2], feat2bev[1, 2] = lower[0], lower[1]
    feat2bev[2, 2] = 1
    tf = torch.inverse(feat2bev).view(1, 3, 3).matmul(l02l1).matmul(feat2bev.view(1, 3, 3))
    return tf[:, :2, :].contiguous()


def pack_bev_align_meta(transforms, slots, valid, write_slot):
    """transforms [B, T, 2, 3] fp32, slots and valid [B, T] (or [T]: the same for every sample), write_slot -> the
    launch's meta buffer, an int32 CPU tensor of 4 + 8 B T words in include/bevops.h's layout.  Checked here, because the
    launch cannot: every slot and write_slot inside the ring 0 .. T, no valid slice reading write_slot."""
    tf = torch.as_tensor(transforms, dtype=torch.float32).detach().cpu()
    if tf.dim() != 4 or tuple(tf.shape[2:]) != (2, 3):
        raise ValueError("pack_bev_align_meta: transforms [B, T, 2, 3]")
    B, T = tf.shape[:2]
    slots = torch.as_tensor(slots).to(torch.int32).cpu().expand(B, T)
    valid = torch.as_tensor(valid).to(torch.int32).cpu().ne(0).expand(B, T)
    write_slot = int(write_slot)
    if not 1 <= T <= BEV_ALIGN_MAX_T:
        raise ValueError(f"pack_bev_align_meta: 1 <= T <= {BEV_ALIGN_MAX_T}")
    if not 0 <= write_slot <= T or bool(((slots < 0) | (slots > T)).any()):
        raise ValueError(f"pack_bev_align_meta: write_slot and every slot inside the ring 0 .. {T}")
    if bool((valid & (slots == write_slot)).any()):
        raise ValueError("pack_bev_align_meta: a valid slice reads write_slot, the slot this frame overwrites")
    meta = torch.zeros(bev_align_meta_words(B, T), dtype=torch.int32)
    meta[0] = write_slot
    body = meta[META_HEAD:].view(B, T, META_ENTRY)
    body[..., 0] = slots
    body[..., 1] = valid.to(torch.int32)
    body[..., 2:] = tf.reshape(B, T, 6).contiguous().view(torch.int32)
    return meta


def unpack_bev_align_meta(meta, B, T):
    """-> (write_slot, slots [B, T] int32, valid [B, T] bool, transforms [B, T, 2, 3] fp32) of a meta buffer (CPU copies)."""
    meta = meta.detach().cpu()
    if meta.dtype != torch.int32 or meta.dim() != 1 or meta.numel() != bev_align_meta_words(B, T):
        raise ValueError(f"bev_align: meta an int32 tensor of {bev_align_meta_words(B, T)} words for B = {B}, T = {T}")
    body = meta[META_HEAD:].view(B, T, META_ENTRY)
    return (int(meta[0]), body[..., 0].clone(), body[..., 1] != 0,
            body[..., 2:].contiguous().view(torch.float32).reshape(B, T, 2, 3).clone())


def bev_align_stack_plain(curr, hist, meta, T):
    """The torch statement: curr [B, C, H, W], hist [T + 1, B, C, H, W] (slot `write_slot` is overwritten with curr),
    meta as packed -> [B, (T + 1) C, H, W].  The positions are the launch's (fp32, each product and sum rounded on its
    own); F.grid_sample then takes them normalised, so it un-normalises them again: a few ulps of the position apart."""
    B, C, H, W = curr.shape
    write_slot, slots, valid, tf = unpack_bev_align_meta(meta, B, T)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    parts = [curr]
    for t in range(T):
        rows = []
        for b in range(B):
            if not bool(valid[b, t]):
                rows.append(curr[b])
                continue
            a = tf[b, t]
            sx = (a[0, 0] * xs + a[0, 1] * ys) + a[0, 2]
            sy = (a[1, 0] * xs + a[1, 1] * ys) + a[1, 2]
            grid = torch.stack((sx / max(W - 1, 1) * 2 - 1, sy / max(H - 1, 1) * 2 - 1), -1)
            grid = grid.view(1, H, W, 2).to(curr.device, curr.dtype)
            rows.append(F.grid_sample(hist[int(slots[b, t])][b:b + 1], grid, mode="bilinear", padding_mode="zeros",
                                      align_corners=True)[0])
        parts.append(torch.stack(rows))
    out = torch.cat(parts, dim=1)
    hist[write_slot].copy_(curr)
    return out


def bev_align_stack_q_plain(curr, hist, meta, T):
    """The statement of the int8 launch for int8 tensors on any device: curr [B, C, H, W], hist [T + 1, B, C, H, W] (slot
    `write_slot` is overwritten with curr), meta as packed -> int8 [B, (T + 1) C, H, W].  The positions are the launch's
    (fp32, each product and sum rounded on its own); corner validity on those floats; weights and blend in float64 on
    the integer values; round half to even, clamp to +-127.  A slot outside the ring gives zeros, a write_slot outside
    it keeps nothing.  (No F.grid_sample: int8 has none, and the tests need the exact statement.)"""
    if curr.dtype != torch.int8 or hist.dtype != torch.int8:
        raise ValueError("bev_align_stack_q_plain: int8 curr and hist")
    B, C, H, W = curr.shape
    write_slot, slots, valid, tf = unpack_bev_align_meta(meta, B, T)
    c, h = curr.detach().cpu(), hist.detach().cpu()
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    out = torch.zeros(B, (T + 1) * C, H, W, dtype=torch.int8)
    out[:, :C] = c
    for b in range(B):
        for t in range(T):
            sl, slot = slice((t + 1) * C, (t + 2) * C), int(slots[b, t])
            if not bool(valid[b, t]):
                out[b, sl] = c[b]
                continue
            if not 0 <= slot <= T:
                continue
            a = tf[b, t]
            sx = ((a[0, 0] * xs + a[0, 1] * ys) + a[0, 2]).double()
            sy = ((a[1, 0] * xs + a[1, 1] * ys) + a[1, 2]).double()
            x0, y0 = sx.floor(), sy.floor()
            fx, fy = sx - x0, sy - y0
            src, val = h[slot, b].double(), torch.zeros(C, H, W, dtype=torch.float64)
            for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
                xc, yc = x0 + dx, y0 + dy
                ok = (xc >= 0) & (xc <= W - 1) & (yc >= 0) & (yc <= H - 1)          # false for NaN and infinities
                xi, yi = torch.where(ok, xc, 0.0).long(), torch.where(ok, yc, 0.0).long()
                val += torch.where(ok, w, 0.0) * torch.where(ok, src[:, yi, xi], 0.0)
            out[b, sl] = val.round().clamp(-127, 127).to(torch.int8)
    if 0 <= write_slot <= T:
        hist[write_slot].copy_(curr)
    return out.to(curr.device)


def bev_align_stack(curr, hist, meta, T, out=None):
    """curr [B, C, H, W], hist [T + 1, B, C, H, W] (the ring: T past frames and one free slot), meta = the int32 buffer of
    `pack_bev_align_meta` on curr's device -> [B, (T + 1) C, H, W]: curr, then slice t = hist[slot(b, t)] sampled
    bilinearly at the transformed pixel (or curr where the slice is invalid); curr is also written into
    hist[write_slot].

    fp16 and int8 CUDA channel slices of channels-last tensors take ONE launch and return a channels-last tensor (`out`:
    a channel slice to write); int8 blends bytes into bytes of the same scale (C % 16 == 0).  int8 elsewhere:
    `bev_align_stack_q_plain`.  Anything else: `bev_align_stack_plain`."""
    T = int(T)
    if not torch.is_tensor(curr) or curr.dim() != 4:
        raise ValueError("bev_align_stack: curr a [B, C, H, W] tensor")
    B, C, H, W = curr.shape
    if not (torch.is_tensor(hist) and tuple(hist.shape) == (T + 1, B, C, H, W) and hist.dtype == curr.dtype and
            hist.device == curr.device):
        raise ValueError(f"bev_align_stack: hist {(T + 1, B, C, H, W)} of curr's dtype and device")
    if not (torch.is_tensor(meta) and meta.dtype == torch.int32 and meta.dim() == 1 and
            meta.numel() == bev_align_meta_words(B, T) and meta.device == curr.device and meta.is_contiguous()):
        raise ValueError(f"bev_align_stack: meta a contiguous int32 tensor of {bev_align_meta_words(B, T)} words on curr's device")
    q8 = curr.dtype == torch.int8
    if not (curr.is_cuda and (q8 or curr.dtype == torch.float16)):
        res = (bev_align_stack_q_plain if q8 else bev_align_stack_plain)(curr, hist, meta, T)
        return res if out is None else out.copy_(res)
    vec, entry = (16, "bevops_bev_align_stack_s8") if q8 else (8, "bevops_bev_align_stack_f16")
    if C % vec or not 1 <= T <= BEV_ALIGN_MAX_T:
        raise _lib.BevopsError(f"{entry}: C % {vec} == 0 and 1 <= T <= {BEV_ALIGN_MAX_T}", _lib.NOT_SUPPORTED)
    cp, hp = slice_pitch(curr, "curr"), slice_pitch(hist[0], "hist[0]")
    if hist.stride(0) != B * H * W * hp:
        raise ValueError("bev_align_stack: the ring's slots lie B H W pitch elements apart")
    if meta.data_ptr() % 16:
        raise ValueError("bev_align_stack: meta starts on a 16-byte boundary")
    out = _dest(out, (B, (T + 1) * C, H, W), curr, "bev_align_stack")
    op = slice_pitch(out, "out")
    if B and H * W:
        _call(entry, curr.device, *(() if q8 else (_lib.F16,)), curr.data_ptr(), cp, hist.data_ptr(), hp, out.data_ptr(), op,
              meta.data_ptr(), B, H, W, C, T)
    return out
