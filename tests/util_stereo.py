"""Float64 statement and input generators for the BEVStereo cost-volume tests (csrc/stereo_cost.hip,
bevformer_tensorrt_amd/functions/stereo.py).  design/bevstereo.md section 4 derives the bounds."""
import torch

EPS32 = 2.0 ** -24          # half an ulp of fp32, relative
HALF_ULP16 = 2.0 ** -11     # half an ulp of fp16, relative (normal range)
SUB16 = 2.0 ** -25          # half an ulp of fp16 in its subnormal range, absolute


def relu_like(shape, gen, scale=1.0):
    """Post-ReLU-like features: non-negative, about half exact zeros, fp16-exact.  The zeros come in 2 x 2 patches, as
    the dead regions of a real activation map do, so that all four corners of a sample are zero often enough for
    gate == 0 to fire inside the image."""
    n, c, h, w = shape
    keep = torch.rand((n, c, (h + 1) // 2, (w + 1) // 2), generator=gen) < 0.5
    keep = keep.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :h, :w]
    return (torch.randn(shape, generator=gen).abs() * scale * keep).half().float()


def dyadic(shape, gen, zeros=True):
    """Multiples of 1/8 in [0, 4) (about half of them zero with zeros=True): exact in fp16, products with weights k/16
    and sums over hundreds of channels exact in fp32."""
    v = torch.randint(0, 32, shape, generator=gen).float() / 8
    if zeros:
        v = v * (torch.rand(shape, generator=gen) < 0.5)
    return v


def source_pos(grid, Hc, Wc):
    """The fp32 un-normalisation the kernel applies (align_corners=True): ((g + 1) * 0.5) * (size - 1), each step one
    fp32 operation.  grid [..., 2] fp32 -> (ix, iy) fp32."""
    g = grid.float()
    ix = ((g[..., 0] + 1.0) * 0.5) * float(Wc - 1)
    iy = ((g[..., 1] + 1.0) * 0.5) * float(Hc - 1)
    return ix, iy


def lattice_grid(tx, ty, Hc, Wc):
    """Normalised fp32 grid whose fp32 un-normalisation lands EXACTLY on the targets tx, ty (multiples of 1/4, any
    shape): g = 2 t / (size - 1) - 1 or one of its four fp32 neighbours; a target no neighbour hits becomes -1 (pixel
    0, on the lattice too).  A one-pixel axis maps every g to 0: targets there must be 0."""
    def axis(t, size):
        t = t.float()
        if size == 1:
            return torch.full_like(t, -1.0)
        g0 = (2.0 * t.double() / (size - 1) - 1.0).float()
        best = torch.full_like(t, -1.0)
        done = torch.zeros_like(t, dtype=torch.bool)
        cand = g0
        for step in (0, 1, -1, 2, -2):
            cand = g0
            for _ in range(abs(step)):
                cand = torch.nextafter(cand, torch.full_like(cand, float("inf") if step > 0 else float("-inf")))
            hit = (((cand + 1.0) * 0.5) * float(size - 1) == t) & ~done
            best = torch.where(hit, cand, best)
            done |= hit
        return best
    return torch.stack([axis(tx, Wc), axis(ty, Hc)], dim=-1)


def ref_cost_volume(prev, curr, grid, bias):
    """Float64 statement on the SAME fp32 grid, the pixel un-normalisation in fp32 as the kernel does it.
    prev, curr [n, C, Hc, Wc] (fp16-exact values), grid [n, D, Hc, Wc, 2] fp32.
    -> dict(prob [n, D, Hc, Wc] float64, cost (with bias), mag = sum_c (|curr| + sum_k w_k |p_k|) per (n, d, h, w): the
    magnitude the fp32 rounding errors of a cost scale with, gate [n, D, Hc, Wc] bool, touched: list of 4 (valid, yi,
    xi) corner index tensors)."""
    n, C, H, W = curr.shape
    D = grid.shape[1]
    ix, iy = source_pos(grid, H, W)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    ixd, iyd = ix.double(), iy.double()
    wts = [((x1.double() - ixd) * (y1.double() - iyd), x0, y0), ((ixd - x0.double()) * (y1.double() - iyd), x1, y0),
           ((x1.double() - ixd) * (iyd - y0.double()), x0, y1), ((ixd - x0.double()) * (iyd - y0.double()), x1, y1)]
    P = prev.double().permute(0, 2, 3, 1)                      # [n, H, W, C]
    warp = torch.zeros(n, D, H, W, C, dtype=torch.float64)
    mag = curr.double().abs().sum(1)[:, None].expand(n, D, H, W).clone()
    img = torch.arange(n).view(n, 1, 1, 1).expand(n, D, H, W)
    touched = []
    for wt, xf, yf in wts:
        valid = (xf >= 0) & (xf <= W - 1) & (yf >= 0) & (yf <= H - 1)          # NaN / inf: outside
        xi = torch.where(valid, xf, torch.zeros_like(xf)).long()
        yi = torch.where(valid, yf, torch.zeros_like(yf)).long()
        vals = P[img, yi, xi]                                   # [n, D, H, W, C]
        term = torch.where(valid[..., None], wt[..., None] * vals, torch.zeros_like(vals))
        warp = warp + term
        mag = mag + torch.where(valid, wt.abs() * vals.abs().sum(-1), torch.zeros_like(wt))
        touched.append((valid, yi, xi))
    cost = (curr.double().permute(0, 2, 3, 1)[:, None] - warp).abs().sum(-1)
    gate = warp[..., C - 4] == 0
    if bias != 0:
        cost = cost + float(bias) * gate
    return dict(prob=torch.softmax(-cost, dim=1), cost=cost, mag=mag, gate=gate, touched=touched)


def softmax_bound(want):
    """|fp16 output - float64 softmax| when the COSTS are exact: x - m exact or one rounding, expf within 1 ulp, a
    butterfly sum of at most 128 terms (8 roundings), one division: below 16 half-ulps of fp32 relative; then the fp16
    rounding (half an ulp relative, 2^-25 absolute in the subnormal range)."""
    return want * (HALF_ULP16 + 16 * EPS32 * (1 + HALF_ULP16)) + SUB16


def general_bound(want, mag, chunks=1):
    """With fp32 costs: every cost carries an error of at most gamma * mag, gamma = (20 + chunks) 2^-24 -- four roundings
    in the blend, one in the difference, four in the lane's sum, six in the butterfly, one per further chunk, second
    order terms in the slack -- and a softmax moves by at most the factor exp(2 max_d error)."""
    delta = (20 + chunks) * EPS32 * mag.max(dim=1, keepdim=True).values
    grow = torch.expm1(2 * delta)
    return want * (grow + (1 + grow) * (HALF_ULP16 + 16 * EPS32)) + SUB16
