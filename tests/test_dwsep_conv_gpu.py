"""bevops_dwsep_conv_f16 (csrc/dwsep_conv.hip) through functions.yolox_ops.dwsep_conv_taps in the guarded arena of
tests/util_arena.py, against the float64 statement of tests/util_dwsep.py.  Exact tests: x, w_dw, w_pw integers in
[-8, 8] * 2^-4, bias_dw in [-32, 32] * 2^-6, bias_pw in [-256, 256] * 2^-6, identity in [-512, 512] * 2^-5: the depthwise
sum (<= 704 units of 2^-8) is exact in fp32 and an fp16 number, the pointwise sum (< 2^24 units of 2^-12) exact; only
the final rounding is left.  The lattice and the SiLU bound are derived in design/yolox_depthwise.md."""
import functools

import pytest
import torch

from util_arena import POISONS, Arena
from util_dwsep import bound, statement

pytestmark = pytest.mark.gpu
F16 = torch.float16


def _bits(t):
    return t.contiguous().view(torch.int16)


def launch(poison, x, wd, bd, wp, bp, act_dw, act_pw, res=None, stride=1, same=False, alias=False):
    """One call in a fresh arena: x channels 8 .. of a buffer 40 wider, out channels 16 .. of one 24 wider, the identity a
    slice of its own (alias: the output slice); same: x and out disjoint slices of ONE buffer.  -> out on the host."""
    from bevformer_tensorrt_amd.functions import dwsep_conv_taps
    A = Arena(8 << 20, poison)
    (B, C, H, W), Co = x.shape, wp.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if same:
        obuf, c0 = A.empty((B, C + Co + 8, H, W), F16, 16, "x|out", channels_last=True), C
        xs = obuf[:, :C]
    else:
        xs = A.empty((B, C + 40, H, W), F16, 16, "x", channels_last=True)[:, 8:8 + C]
        obuf, c0 = A.empty((B, Co + 24, Ho, Wo), F16, 16, "out", channels_last=True), 16
    xs.copy_(x)
    out, rs = obuf[:, c0:c0 + Co], None
    if res is not None:
        rs = out if alias else A.empty((B, Co + 8, Ho, Wo), F16, 16, "identity", channels_last=True)[:, :Co]
        rs.copy_(res)
    dev = lambda t, name, align=16: None if t is None else A.place(t.contiguous(), align, name)      # noqa: E731
    before = obuf.clone()
    got = dwsep_conv_taps(xs, dev(wd[:, 0].permute(1, 2, 0), "w_dw"), dev(bd, "bias_dw"), dev(wp[:, :, 0, 0], "w_pw"),
                          dev(bp, "bias_pw", 2), act_dw, act_pw, rs, stride, out=out)
    A.check()
    other = torch.ones(obuf.shape[1], dtype=torch.bool)
    other[c0:c0 + Co] = False
    assert torch.equal(_bits(obuf[:, other]), _bits(before[:, other])), "bytes outside the output slice were written"
    return got.cpu()


def both_poisons(*args, **kw):
    a, b = (launch(p, *args, **kw) for p in POISONS)
    assert torch.equal(_bits(a), _bits(b)), "results differ between the two poisons"
    return a


def ints(g, shape, amp, step):
    return (torch.randint(-amp, amp + 1, shape, generator=g) * step).to(F16)


@functools.lru_cache(maxsize=None)
def lattice(H, W, C, Co, stride, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * Co + H + seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return (ints(g, (2, C, H, W), 8, 2.0 ** -4), ints(g, (C, 1, 3, 3), 8, 2.0 ** -4), ints(g, (C,), 32, 2.0 ** -6),
            ints(g, (Co, C, 1, 1), 8, 2.0 ** -4), ints(g, (Co,), 256, 2.0 ** -6), ints(g, (2, Co, Ho, Wo), 512, 2.0 ** -5))


# (H, W, Cin, Cout, stride, x and out in one buffer), B = 2: 1 x 1; 3 x 5; 12 x 11 = a row tile plus four pixels, the second
# tile straddles the images; stride 2 on odd sizes; 1, 3, 5 chunks; Cout below, across and beyond a 64- / 128-column tile
CASES = ((1, 1, 32, 8, 1, False), (3, 5, 96, 72, 1, True), (12, 11, 160, 136, 1, False), (7, 9, 96, 136, 2, False),
         (12, 11, 32, 72, 2, False), (12, 11, 160, 8, 1, True))


@pytest.mark.parametrize("acts", [("none", "relu"), ("relu", "none")], ids="-".join)
@pytest.mark.parametrize("identity", ["absent", "present", "alias"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(case, identity, acts):
    H, W, C, Co, stride, same = case
    x, wd, bd, wp, bp, res = lattice(H, W, C, Co, stride)
    plain = identity == "absent"                     # (also: no biases)
    bd, bp, res = (None, None, None) if plain else (bd, bp, res)
    e, _, t, _ = statement(x, wd, bd, wp, bp, *acts, res, stride)
    assert torch.equal(e.float().double(), e) and t.any() and e.any()          # every intermediate is an fp32 number
    got = both_poisons(x, wd, bd, wp, bp, *acts, res, stride, same, identity == "alias")
    assert torch.equal(_bits(got), _bits(e.to(F16))), f"{int((_bits(got) != _bits(e.to(F16))).sum())} outputs differ"


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("tap", range(9))
def test_one_hot_tap_moves_its_pixel(tap, stride):
    """w_dw = 1 at tap (ky, kx) only, w_pw = I: out[yo, xo] = x[s yo + ky - 1, s xo + kx - 1], 0 outside the image -- at
    every corner, edge and interior pixel of a 5 x 6 map."""
    B, C, H, W, ky, kx = 2, 32, 5, 6, tap // 3, tap % 3
    x = ((1 + torch.arange(B * H * W).view(B, 1, H, W) + 64 * torch.arange(C).view(1, C, 1, 1) % 512) / 64.0).to(F16)
    wd = torch.zeros((C, 1, 3, 3), dtype=F16)
    wd[:, 0, ky, kx] = 1.0
    wp = torch.eye(C, dtype=F16).view(C, C, 1, 1)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    want = torch.zeros((B, C, Ho, Wo), dtype=F16)
    for yo in range(Ho):
        for xo in range(Wo):
            y, xx = stride * yo + ky - 1, stride * xo + kx - 1
            if 0 <= y < H and 0 <= xx < W:
                want[:, :, yo, xo] = x[:, :, y, xx]
    got = both_poisons(x, wd, None, wp, None, "none", "none", None, stride)
    assert torch.equal(_bits(got), _bits(want)) and want.any()


@pytest.mark.parametrize("stride,bad", [(1, float("nan")), (2, float("inf"))])
def test_a_non_finite_pixel_reaches_its_windows_only(stride, bad):
    H, W, C, Co = 7, 9, 96, 136
    x, wd, bd, wp, bp, res = lattice(H, W, C, Co, stride)
    clean = both_poisons(x, wd, bd, wp, bp, "none", "none", res, stride)
    xi, (b0, y0, x0) = x.clone(), (1, 3, 4)
    xi[b0, 37, y0, x0] = bad
    got = both_poisons(xi, wd, bd, wp, bp, "none", "none", res, stride)
    reached = torch.zeros(got.shape, dtype=torch.bool)
    for yo in range(got.shape[2]):
        for xo in range(got.shape[3]):
            reached[b0, :, yo, xo] = abs(stride * yo - y0) <= 1 and abs(stride * xo - x0) <= 1
    assert int(reached[b0, 0].sum()) == (9 if stride == 1 else 2)
    assert not torch.isfinite(got[reached]).any() and torch.equal(_bits(got[~reached]), _bits(clean[~reached]))


@pytest.mark.parametrize("geom", [(11, 12, 96, 136, 1, True), (9, 9, 160, 72, 2, False)], ids=lambda g: "x".join(map(str, g)))
def test_silu_on_gaussian_operands_within_the_derived_bound(geom):
    H, W, C, Co, stride, with_res = geom
    g = torch.Generator().manual_seed(C + Co)
    n = lambda *s: torch.randn(s, generator=g)                                                     # noqa: E731
    x, wd, bd = n(2, C, H, W).to(F16), (2.0 * n(C, 1, 3, 3) / 3.0).to(F16), (0.5 * n(C)).to(F16)
    wp, bp = (2.0 * n(Co, C, 1, 1) / C ** 0.5).to(F16), (0.5 * n(Co)).to(F16)
    res = n(2, Co, (H - 1) // stride + 1, (W - 1) // stride + 1).to(F16) if with_res else None
    e, s, t, mag = statement(x, wd, bd, wp, bp, "silu", "silu", res, stride)
    lim = bound(e, s, t, mag, wp)
    import torch.nn.functional as Fn                  # the statement in float32 on the CPU: inside half the bound
    t32 = Fn.silu(Fn.conv2d(x.float(), wd.float(), bd.float(), stride, 1, 1, C)).half().float()
    e32 = Fn.silu(Fn.conv2d(t32, wp.float(), bp.float())) + (0.0 if res is None else res.float())
    assert bool(((e32.half().double() - e).abs() <= 0.5 * lim).all()), "the operands leave no room inside the bound"
    got = both_poisons(x, wd, bd, wp, bp, "silu", "silu", res, stride).double()
    err = (got - e).abs()
    print(f"SiLU Gaussian {geom}: max |err| {float(err.max()):.3e}, max err / bound {float((err / lim).max()):.3f}")
    assert bool((err <= lim).all()), f"{int((err > lim).sum())} outputs beyond the bound"


def test_wrapper_pads_channels_and_replays_the_eager_bits():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    x, wd, bd, wp, bp, _ = (t.cuda() for t in lattice(12, 11, 32, 72, 1))
    xs = Y.nhwc_empty(2, 32, 12, 11, "cuda")
    xs.copy_(x)
    xs[:, 16:] = 0
    w16, p16 = wd[:16].contiguous(), wp[:16, :16].contiguous()      # a 16-channel layer at 32: pad channels exact zeros
    out = Y.nhwc_empty(2, 32, 12, 11, "cuda")
    eager = bev.dwsep_conv_nhwc(xs, w16, bd[:16], p16, bp[:16], out=out).clone()
    e, s, t, mag = statement(xs[:, :16], w16, bd[:16], p16, bp[:16], "silu", "silu")
    assert torch.count_nonzero(eager[:, 16:]) == 0
    assert bool(((eager[:, :16].double().cpu() - e).abs() <= bound(e, s, t, mag, p16)).all())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bev.dwsep_conv_nhwc(xs, w16, bd[:16], p16, bp[:16], out=out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        assert torch.equal(_bits(out), _bits(eager))
    w16.mul_(2.0)                                                    # a changed weight: never repacked in a capture
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        out.add_(1.0)
        with pytest.raises(RuntimeError, match="capturing"):
            bev.dwsep_conv_nhwc(xs, w16, bd[:16], p16, bp[:16], out=out)
