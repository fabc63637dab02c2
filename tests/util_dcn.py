"""DCNv2 forward stated from its definition in float64, and "lattice" inputs on which a correct
kernel makes no rounding before its final store.

`dcn_ref` is a second, independent statement of the operator (it never touches oracle/): the tests
compare the HIP kernels with it, and test_dcn_reference_cpu.py compares it with the C oracle.

    h = ho * stride - pad + i * dil + off_h          (w likewise; tap = i * K + j)
    offset channels [dg][2 * tap (h), 2 * tap + 1 (w)], mask channels [dg][tap]
    a tap contributes iff -1 < h < H and -1 < w < W
    each of its four corners contributes iff it lies inside the image: an in-image corner is multiplied
    even when its weight is 0 (0 * inf = NaN), an out-of-image corner is skipped, never multiplied
    col = (sum of the corners) * mask;  out = grouped weights . col + bias;  optional ReLU
"""
import torch

KK = 9   # every generator below is for 3 x 3 kernels


def out_size(n, stride, pad, dil, k=3):
    return (n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def dcn_ref(x, offset, mask, weight, bias, stride, pad, dil, groups, deform_groups, relu=False, return_col=False):
    """float64 DCNv2.  x [B, Cin, H, W], offset [B, dg * 2 * K * K, Ho, Wo], mask [B, dg * K * K, Ho, Wo],
    weight [Cout, Cin / groups, K, K], bias [Cout] or None -> out [B, Cout, Ho, Wo] (float64);
    return_col: also the sampled, masked values col [B, Cin, K * K, Ho, Wo]."""
    x, offset, mask, weight = (t.detach().cpu().double() for t in (x, offset, mask, weight))
    B, Cin, H, W = x.shape
    Cout, cin_g, Kh, Kw = weight.shape
    kk = Kh * Kw
    Ho, Wo = out_size(H, stride, pad, dil, Kh), out_size(W, stride, pad, dil, Kw)
    assert offset.shape == (B, deform_groups * 2 * kk, Ho, Wo) and mask.shape == (B, deform_groups * kk, Ho, Wo)
    assert cin_g * groups == Cin and Cout % groups == 0 and Cin % deform_groups == 0
    cpd = Cin // deform_groups
    base_h = (torch.arange(Ho, dtype=torch.float64) * stride - pad).view(1, Ho, 1)
    base_w = (torch.arange(Wo, dtype=torch.float64) * stride - pad).view(1, 1, Wo)
    col = torch.zeros(B, Cin, kk, Ho, Wo, dtype=torch.float64)
    xf = x.reshape(B, Cin, H * W)
    for dg in range(deform_groups):
        xg = xf[:, dg * cpd:(dg + 1) * cpd]
        for tap in range(kk):
            i, j = divmod(tap, Kw)
            h = base_h + i * dil + offset[:, (dg * kk + tap) * 2]
            w = base_w + j * dil + offset[:, (dg * kk + tap) * 2 + 1]
            live = (h > -1) & (h < H) & (w > -1) & (w < W)
            h0, w0 = torch.floor(h), torch.floor(w)
            lh, lw = h - h0, w - w0
            acc = torch.zeros(B, cpd, Ho, Wo, dtype=torch.float64)
            for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                hc, wc = h0 + dh, w0 + dw
                inside = live & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
                idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long().view(B, 1, Ho * Wo).expand(B, cpd, Ho * Wo)
                v = torch.gather(xg, 2, idx).view(B, cpd, Ho, Wo)
                acc = acc + torch.where(inside.unsqueeze(1), wt.unsqueeze(1) * v, torch.zeros((), dtype=torch.float64))
            col[:, dg * cpd:(dg + 1) * cpd, tap] = acc * mask[:, dg * kk + tap].unsqueeze(1)
    cout_g = Cout // groups
    out = torch.empty(B, Cout, Ho, Wo, dtype=torch.float64)
    for g in range(groups):
        wg = weight[g * cout_g:(g + 1) * cout_g].reshape(cout_g, cin_g * kk)                 # k = (ci, tap)
        cg = col[:, g * cin_g:(g + 1) * cin_g].reshape(B, cin_g * kk, Ho * Wo)
        out[:, g * cout_g:(g + 1) * cout_g] = torch.matmul(wg.unsqueeze(0), cg).view(B, cout_g, Ho, Wo)
    if bias is not None:
        out = out + bias.detach().cpu().double().view(1, Cout, 1, 1)
    if relu:
        out = torch.where(out < 0, torch.zeros((), dtype=torch.float64), out)   # keeps NaN, as fmaxf(NaN, 0) does not:
        # the tests compare non-finite outputs as a set, never by value
    return (out, col) if return_col else out


def unpack_offset_mask(om, kk=KK):
    """The raw channels-last output [B, OC, Ho, Wo] of the pack's offset convolution (one deform group):
    offsets = channels [0, 2 kk), mask = sigmoid of the logits in [2 kk, 3 kk), computed in float64 from the
    fp16 logits; channels >= 3 kk are padding and ignored."""
    om = om.detach().cpu()
    assert om.dtype == torch.float16 and om.shape[1] >= 3 * kk
    return om[:, :2 * kk].double(), torch.sigmoid(om[:, 2 * kk:3 * kk].double())


# ---- lattice inputs -------------------------------------------------------------------------------------------
# x in (1/8) Z within [-4, 4], bilinear fractions in {0, 1/2}, masks in (1/4) Z within [0, 1], weights in (1/8) Z within
# [-1, 1], bias in (1/8) Z: a column element is a multiple of 2^-7 of magnitude <= 4 (exact in fp16, as is every
# partial blend), an output before its final rounding a multiple of 2^-10 below 9 * 128 * 4 + 2 < 2^14 (exact in
# fp32, as is every partial sum in any order).  test_dcn_reference_cpu.py checks this premise on dcn_ref's own
# column tensor and output, not on any kernel.

def row_classes(n):
    """Tap targets along an axis of length n: both sides of -1, 0, n - 1 and n, on them and half a pixel off."""
    return [-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, n - 1.5, n - 1.0, n - 0.5, float(n), n + 0.5]


FAR = (1000.0, -1000.0, 60000.0, -60000.0)     # offsets (not targets: these are the fp16-exact quantities)
OM_LOGITS = (-30.0, 0.0, 20.0)                 # the kernel's fp16 sigmoid must give exactly 0, 1/2, 1


def lattice(B, Cin, Cout, H, W, stride, pad, dil, groups=1, deform_groups=1, seed=0):
    """dict of float32 CPU tensors, every value exactly representable in fp16:
    x, weight, bias, offset, mask (planar, values {0, 1/4, 1/2, 3/4, 1}), and -- deform_groups == 1 only --
    om32 / om28 [B, OC, Ho, Wo]: the same offsets, mask LOGITS from OM_LOGITS and non-zero junk in the padding
    channels >= 27; plus the integer class indices cls_h / cls_w [B, dg * 9, Ho, Wo] (-1 where a far offset
    replaced the class)."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_size(H, stride, pad, dil), out_size(W, stride, pad, dil)
    x = torch.randint(-32, 33, (B, Cin, H, W), generator=g).float() / 8
    weight = torch.randint(-8, 9, (Cout, Cin // groups, 3, 3), generator=g).float() / 8
    bias = torch.randint(-16, 17, (Cout,), generator=g).float() / 8
    rows, cols = torch.tensor(row_classes(H)), torch.tensor(row_classes(W))
    nr, nc = len(rows), len(cols)
    # n numbers the (image, pixel, tap) triples; (n % 11, n // 11 % 11) walks all 121 class pairs
    n = torch.arange(B * Ho * Wo * KK).view(B, Ho, Wo, KK).permute(0, 3, 1, 2)          # [B, 9, Ho, Wo]
    base_h = (torch.arange(Ho).float() * stride - pad).view(1, 1, Ho, 1) + (torch.arange(KK) // 3).float().view(1, KK, 1, 1) * dil
    base_w = (torch.arange(Wo).float() * stride - pad).view(1, 1, 1, Wo) + (torch.arange(KK) % 3).float().view(1, KK, 1, 1) * dil
    offset = torch.empty(B, deform_groups, KK, 2, Ho, Wo)
    mask = torch.empty(B, deform_groups, KK, Ho, Wo)
    cls_h = torch.empty(B, deform_groups, KK, Ho, Wo, dtype=torch.long)
    cls_w = torch.empty_like(cls_h)
    for dg in range(deform_groups):
        m = n + 17 * dg
        ch, cw = m % nr, (m // nr) % nc
        off_h = rows[ch] - base_h
        off_w = cols[cw] - base_w
        far_h, far_w = (m % 13 == 5) & (n >= nr * nc), (m % 17 == 7) & (n >= nr * nc)    # the first 121 keep every pair
        off_h = torch.where(far_h, torch.tensor(FAR)[(m // 13) % 4].expand_as(off_h), off_h)
        off_w = torch.where(far_w, torch.tensor(FAR)[(m // 17) % 4].expand_as(off_w), off_w)
        offset[:, dg, :, 0], offset[:, dg, :, 1] = off_h, off_w
        cls_h[:, dg], cls_w[:, dg] = torch.where(far_h, -1, ch), torch.where(far_w, -1, cw)
        mask[:, dg] = ((m * 3 + m // 5) % 5).float() / 4
    out = dict(x=x, weight=weight, bias=bias, offset=offset.view(B, deform_groups * 2 * KK, Ho, Wo),
               mask=mask.view(B, deform_groups * KK, Ho, Wo), cls_h=cls_h.view(B, -1, Ho, Wo), cls_w=cls_w.view(B, -1, Ho, Wo))
    if deform_groups == 1:
        logits = torch.tensor(OM_LOGITS)[(n + n // 3) % 3]
        for oc in (32, 28):
            om = torch.empty(B, oc, Ho, Wo)
            om[:, :2 * KK] = out["offset"]
            om[:, 2 * KK:3 * KK] = logits
            om[:, 3 * KK:] = torch.randint(1, 9, (B, oc - 3 * KK, Ho, Wo), generator=g).float() * 2.5    # junk, never 0
            out[f"om{oc}"] = om
    for k, v in out.items():
        if v.dtype == torch.float32:
            assert torch.equal(v.half().float(), v), k      # the generator's own promise
    return out


def lattice_int8(lat, scale_offset=0.5):
    """The lattice's tap targets as int8 offsets with scale_offset = 1/2 (far offsets saturate at +-127 = +-63.5
    pixels, still far outside the image), masks {0, 1/4, ..., 1} as int8 with scale 1/4, x and weights as their
    integer numerators with scale 1/8."""
    q = lambda t, s: torch.clamp(torch.round(t / s), -127, 127).to(torch.int8)
    return dict(x=q(lat["x"], 0.125), offset=q(lat["offset"], scale_offset), mask=q(lat["mask"], 0.25),
                weight=q(lat["weight"], 0.125), bias=lat["bias"].clone(),
                s_x=0.125, s_o=scale_offset, s_m=0.25, s_w=0.125)


def expect(out64, dtype):
    """dcn_ref's float64 output rounded to nearest-even in the output type.  (On lattice inputs out64 is exact in
    fp32, so no double rounding can occur on the way to fp16.)"""
    return out64.to(dtype)


# (stride, pad, dil) triples and channel counts of the lattice cases: the smallest shapes at which each code path of
# the fused kernels can still go wrong.  B * H * W = 84 pixels = two 64-pixel tiles, the second ragged and crossing
# the batch boundary; Cin 64 / 128 = one / two K chunks per tap; Cout 8, 10 (not a multiple of 4: the scalar
# channels-last store), 260 (two Cout tiles, weight rows past Cout).
LATTICE_B, LATTICE_H, LATTICE_W = 2, 6, 7
LATTICE_GEOM = [(1, 1, 1), (2, 1, 1), (1, 2, 2)]
LATTICE_CHANNELS = [(64, 8), (64, 10), (128, 260)]
