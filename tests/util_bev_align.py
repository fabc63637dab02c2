"""The float64 statement of bevops_bev_align_stack_f16 (csrc/bev_align.hip) for its tests: the positions in numpy float32
in the op order the file header states, then corner selection, weights and blend in float64."""
import numpy as np
import torch

F32 = np.float32


def positions(a, H, W):
    """a = (a00, a01, a02, a10, a11, a12) -> (sx, sy) [H, W] float32: sx = add(add(mul(a00, x), mul(a01, y)), a02)."""
    a = [F32(v) for v in a]
    x = np.arange(W, dtype=F32).reshape(1, W)
    y = np.arange(H, dtype=F32).reshape(H, 1)
    with np.errstate(all="ignore"):
        sx = ((a[0] * x).astype(F32) + (a[1] * y).astype(F32)).astype(F32) + a[2]
        sy = ((a[3] * x).astype(F32) + (a[4] * y).astype(F32)).astype(F32) + a[5]
    return np.broadcast_to(sx.astype(F32), (H, W)), np.broadcast_to(sy.astype(F32), (H, W))


def sample(src, sx, sy):
    """src [C, H, W] float64, fp32 positions -> (value [C, H, W], sum_k w_k |p_k| [C, H, W]) in float64; zeros padding,
    align_corners=True on pixel coordinates; a non-finite or outside corner counts as zero."""
    C, H, W = src.shape
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(sx.astype(np.float64)), np.floor(sy.astype(np.float64))
        fx, fy = sx - x0, sy - y0
    val, mag = np.zeros((C, H, W)), np.zeros((C, H, W))
    for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        with np.errstate(all="ignore"):
            xc, yc = x0 + dx, y0 + dy
            ok = (xc >= 0) & (xc <= W - 1) & (yc >= 0) & (yc <= H - 1)
        xi, yi = np.where(ok, xc, 0).astype(np.int64), np.where(ok, yc, 0).astype(np.int64)
        p = np.where(ok[None], src[:, yi, xi], 0.0)
        wk = np.where(ok, w, 0.0)[None]
        val += wk * p
        mag += wk * np.abs(p)
    return val, mag


def ref_align(curr, hist, tf, slots, valid):
    """curr [B, C, H, W], hist [S, B, C, H, W] torch tensors of fp16-exact values; tf [B, T, 2, 3], slots / valid [B, T]
    -> (out [B, (T + 1) C, H, W], mag likewise) float64 tensors (mag is 0 where a slice is a copy)."""
    B, C, H, W = curr.shape
    T = len(tf[0])
    c64, h64 = curr.double().numpy(), hist.double().numpy()
    out, mag = np.zeros((B, (T + 1) * C, H, W)), np.zeros((B, (T + 1) * C, H, W))
    out[:, :C] = c64
    for b in range(B):
        for t in range(T):
            sl = slice((t + 1) * C, (t + 2) * C)
            if not bool(valid[b][t]):
                out[b, sl] = c64[b]
                continue
            sx, sy = positions(np.asarray(tf[b][t], dtype=F32).reshape(6), H, W)
            out[b, sl], mag[b, sl] = sample(h64[int(slots[b][t]), b], sx, sy)
    return torch.from_numpy(out), torch.from_numpy(mag)


def general_bound(want, mag):
    """design/bevdet4d.md section 4: six counted fp32 roundings (1 - f, the weight product, w p, three additions), eight
    allowed for the second-order terms; the final fp16 rounding; half the smallest fp16 subnormal."""
    return 2.0 ** -11 * want.abs() + 8 * 2.0 ** -24 * mag + 2.0 ** -25


def shift(dx, dy):
    return (1.0, 0.0, dx, 0.0, 1.0, dy)


def rot90(H, W):
    """a quarter turn about the map centre: on the half-pixel lattice, exact in fp32"""
    cx, cy = (W - 1) / 2, (H - 1) / 2
    return (0.0, -1.0, cx + cy, 1.0, 0.0, cy - cx)


def rotation(H, W, angle, dx, dy):
    cx, cy = (W - 1) / 2, (H - 1) / 2
    c, s = float(np.cos(angle)), float(np.sin(angle))
    return (c, -s, cx - c * cx + s * cy + dx, s, c, cy - s * cx - c * cy + dy)


def dyadic(shape, gen):
    """multiples of 1 / 8 below 4"""
    return torch.randint(-31, 32, shape, generator=gen).double().div(8).float()
