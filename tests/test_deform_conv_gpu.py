"""bevops_deform_conv3x3_nhwc_f16 (csrc/deform_conv.hip) through the C ABI in the guarded arena of tests/util_arena.py,
under both poisons, guards intact, equal bits under both: exact on the lattice of tests/util_dcn.py against the float64
statement `dcn_ref` with a ones mask, one-hot taps, Gaussian operands within the bound derived from the operation order
(design/bevdepth_dcn.md section 3), non-finite containment; and the wrapper `deform_conv2d_nhwc`: cache, capture guard,
replay, empty batch."""
import functools

import pytest
import torch

import util_dcn as U
from bevformer_tensorrt_amd.functions import deform_conv2d_nhwc, deform_conv_packed_weight
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 6 << 20
SHAPES = [(2, 6, 7), (3, 9, 15)]          # 84 pixels: a ragged 64-pixel tile across the image boundary; 405: several + tail
CHANNELS = [(32, 32, 1), (64, 64, 2), (128, 128, 4), (256, 256, 4), (256, 128, 4), (128, 256, 4)]


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def run(lib, arena, x, om, weight, bias, relu, groups, status=0):
    """One call on arena buffers.  x [B, Cin, H, W], om [B, OC, H, W], weight [Cout, Cin / groups, 3, 3], bias [Cout] or
    None: CPU tensors of fp16-exact values -> the output [B, Cout, H, W] on the CPU (fp16)."""
    from bevformer_tensorrt_amd.utils import lib as L
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    xd = arena.place(x.half(), 16, "input", channels_last=True)
    od = arena.place(om.half(), 16, "offset", channels_last=True)
    wd = arena.place(weight.half().contiguous(), 16, "weight")
    nbytes = lib.bevops_mdconv_packed_weight_size(L.F16, Cout, Cin // groups, 3, 3)
    pk = arena.carve(nbytes, 16, "packed")
    bd = arena.place(bias.half(), 16, "bias") if bias is not None else None
    out = arena.empty((B, Cout, H, W), torch.float16, 16, "output", channels_last=True)
    stream = L.current_stream_ptr(torch.device("cuda"))
    assert lib.bevops_mdconv_pack_weight(L.F16, wd.data_ptr(), pk.data_ptr(), Cout, Cin // groups, 3, 3, stream) == 0
    st = lib.bevops_deform_conv3x3_nhwc_f16(xd.data_ptr(), od.data_ptr(), om.shape[1], pk.data_ptr(),
                                            bd.data_ptr() if bd is not None else None, out.data_ptr(), int(relu), B, H, W,
                                            Cin, Cout, groups, stream)
    assert st == status
    arena.check()
    return out.cpu().contiguous()


def run_both(lib, *args):
    """Under both poisons; the two results must have equal bits."""
    a, b = (run(lib, Arena(CAPACITY, p), *args) for p in POISONS)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    return a


@functools.lru_cache(maxsize=None)
def lattice_case(shape, channels):
    B, H, W = shape
    cin, cout, groups = channels
    lat = U.lattice(B, cin, cout, H, W, 1, 1, 1, groups, 1)
    ones = torch.ones(B, 9, H, W)
    want = {(b, r): U.expect(U.dcn_ref(lat["x"], lat["offset"], ones, lat["weight"], lat["bias"] if b else None, 1, 1, 1,
                                       groups, 1, r), torch.float16)
            for b in (False, True) for r in (False, True)}
    return lat, ones, want


@pytest.mark.parametrize("channels", CHANNELS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lattice_exact(lib, shape, channels):
    from bevformer_tensorrt_amd.functions import modulated_deformable_conv2d, modulated_deformable_conv2d_nhwc
    from bevformer_tensorrt_amd.utils.lib import BevopsError
    lat, ones, want = lattice_case(shape, channels)
    groups = channels[2]
    for with_bias in (False, True):
        for relu in (False, True):
            for om in ("om32", "om28"):      # mask logits in channels 18 .. 26 and junk behind them: never read
                got = run_both(lib, lat["x"], lat[om], lat["weight"], lat["bias"] if with_bias else None, relu, groups)
                w = want[(with_bias, relu)]
                assert torch.equal(got.view(torch.int16), w.view(torch.int16)), (with_bias, relu, om, (got.float() - w.float()).abs().max())
    assert (want[(False, False)] != 0).float().mean().item() >= 0.5
    # the package's DCNv2 operator on the same inputs, planar offsets and a ones mask
    x = lat["x"].half().cuda().contiguous(memory_format=torch.channels_last)
    off, one, wt, bias = lat["offset"].half().cuda(), ones.half().cuda(), lat["weight"].half().cuda(), lat["bias"].half().cuda()
    try:
        for with_bias in (False, True):
            for relu in (False, True):
                v2 = modulated_deformable_conv2d_nhwc(x, off, one, wt, bias if with_bias else None, 1, 1, 1, groups, 1, relu)
                assert torch.equal(v2.cpu().contiguous().view(torch.int16), want[(with_bias, relu)].view(torch.int16))
    except BevopsError:
        # the channels-last DCNv2 entry walks K in 64-channel chunks: 32 channels per group are outside its domain, and
        # the comparison is made with the planar entry (no bias / ReLU there)
        assert (channels[0] // groups) % 64 != 0
        v2 = modulated_deformable_conv2d(x.contiguous(), off, one, wt, None, 1, 1, 1, groups, 1)
        assert torch.equal(v2.cpu().view(torch.int16), want[(False, False)].view(torch.int16))


ONE_HOT_OFF_H = (2, -1, 0, 1, -2, 0, 1, 2, -1)
ONE_HOT_OFF_W = (-1, 1, 2, -2, 1, -1, 0, 0, 2)          # never the h offset of the same tap: a transposed read shows


def test_one_hot_taps(lib):
    """weight[co, ci, tap] = 1 alone in its row, integer offsets: output channel co is input channel ci shifted by the
    tap's position, zero outside.  Every tap in every group (co = 32 g + tap), offsets that also depend on the pixel."""
    B, H, W, C, G = 2, 6, 7, 128, 4
    g = torch.Generator().manual_seed(5)
    x = (torch.randint(-64, 65, (B, C, H, W), generator=g).float() / 16)
    weight = torch.zeros(C, C // G, 3, 3)
    src = {}
    for grp in range(G):
        for tap in range(9):
            ci = (7 * tap + 3 * grp + 1) % (C // G)
            weight[32 * grp + tap, ci, tap // 3, tap % 3] = 1.0
            src[(grp, tap)] = ci
    ys, xs = torch.arange(H).view(H, 1).expand(H, W), torch.arange(W).view(1, W).expand(H, W)
    wob = (ys + 2 * xs) % 3 - 1                                                   # pixel-dependent part, in {-1, 0, 1}
    om = torch.full((B, 32, H, W), 7.5)
    want = torch.zeros(B, C, H, W)
    for tap in range(9):
        oh, ow = ONE_HOT_OFF_H[tap] + wob, ONE_HOT_OFF_W[tap] - wob
        om[:, 2 * tap], om[:, 2 * tap + 1] = oh.float(), ow.float()
        hh, ww = ys - 1 + tap // 3 + oh, xs - 1 + tap % 3 + ow
        inside = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)
        for grp in range(G):
            v = x[:, 32 * grp + src[(grp, tap)]][:, hh.clamp(0, H - 1), ww.clamp(0, W - 1)]
            want[:, 32 * grp + tap] = torch.where(inside, v, torch.zeros(()))
    got = run_both(lib, x, om, weight, None, False, G)
    assert torch.equal(got.float(), want)
    assert (want[:, :9] != 0).float().mean().item() > 0.3


@functools.lru_cache(maxsize=None)
def gaussian_case():
    B, H, W, C, G = 2, 9, 15, 256, 4
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, H, W, generator=g).half().float()
    weight = (torch.randn(C, C // G, 3, 3, generator=g) * 0.05).half().float()
    bias = torch.randn(C, generator=g).half().float()
    off = torch.randint(-256, 256, (B, 18, H, W), generator=g).float() / 64        # multiples of 1/64 in [-4, 4)
    om = torch.zeros(B, 32, H, W)
    om[:, :18] = off
    ones = torch.ones(B, 9, H, W)
    want = U.dcn_ref(x, off, ones, weight, bias, 1, 1, 1, G, 1)
    return dict(x=x, weight=weight, bias=bias, off=off, om=om, ones=ones, want=want, G=G)


def test_gaussian_within_the_derived_bound(lib):
    """|got - out| <= (2^-11 + (K + 8) 2^-24) A + 2^-11 |out| + 2^-25 (W1 + 1) for EVERY output, in float64:
    A = sum_k |w_k| sum_c a_c |x_c| (the statement itself on |x| and |w|: the corner weights are non-negative),
    W1 = sum_k |w_k|: the fp16 subnormal spacing of a sample and of the result (design/bevdepth_dcn.md section 3)."""
    c = gaussian_case()
    G = c["G"]
    got = run_both(lib, c["x"], c["om"], c["weight"], c["bias"], False, G).double()
    A = U.dcn_ref(c["x"].abs(), c["off"], c["ones"], c["weight"].abs(), c["bias"].abs(), 1, 1, 1, G, 1)
    K = 9 * c["weight"].shape[1]
    W1 = c["weight"].abs().double().sum(dim=(1, 2, 3)).view(1, -1, 1, 1)
    want = c["want"]
    bound = (2.0 ** -11 + (K + 8) * 2.0 ** -24) * A + 2.0 ** -11 * want.abs() + 2.0 ** -25 * (W1 + 1)
    err = (got - want).abs()
    print(f"max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}, rms out {want.pow(2).mean().sqrt().item():.3f}")
    assert bool(torch.isfinite(got).all()) and bool((err <= bound).all())
    assert want.pow(2).mean().sqrt().item() > 0.3


def test_non_finite_containment(lib):
    c = gaussian_case()
    G, x = c["G"], c["x"]
    B, C, H, W = x.shape
    b0, c0, y0, x0 = 1, 70, 4, 7                                                # group 1
    bad = x.clone()
    bad[b0, c0, y0, x0] = float("nan")
    clean = run_both(lib, x, c["om"], c["weight"], c["bias"], True, G)
    dirty = run_both(lib, bad, c["om"], c["weight"], c["bias"], True, G)
    cg = C // G
    grp = c0 // cg
    other = [ch for ch in range(C) if ch // cg != grp]
    assert torch.equal(clean[:, other].view(torch.int16), dirty[:, other].view(torch.int16))
    # the same group: pixels whose nine positions all lie 2 or more pixels from (y0, x0), and the other image
    ys, xs = torch.arange(H).view(H, 1).float(), torch.arange(W).view(1, W).float()
    far = torch.ones(H, W, dtype=torch.bool)
    for tap in range(9):
        h = ys - 1 + tap // 3 + c["off"][b0, 2 * tap]
        w = xs - 1 + tap % 3 + c["off"][b0, 2 * tap + 1]
        far &= ((h - y0).abs() >= 2) | ((w - x0).abs() >= 2)
    assert 10 <= int(far.sum()) < H * W
    same = slice(grp * cg, (grp + 1) * cg)
    assert torch.equal(clean[b0, same][:, far].view(torch.int16), dirty[b0, same][:, far].view(torch.int16))
    assert torch.equal(clean[1 - b0].view(torch.int16), dirty[1 - b0].view(torch.int16))
    assert bool(torch.isfinite(clean).all()) and not torch.equal(clean[b0, same].view(torch.int16), dirty[b0, same].view(torch.int16))


def test_wrapper_cache_capture_replay_and_empty_batch():
    from bevformer_tensorrt_amd.functions import conv_offset_nhwc
    lat, ones, want = lattice_case((2, 6, 7), (128, 128, 4))
    cl = torch.channels_last
    x = lat["x"].half().cuda().contiguous(memory_format=cl)
    om = lat["om32"].half().cuda().contiguous(memory_format=cl)
    w, bias = lat["weight"].half().cuda(), lat["bias"].half().cuda()
    assert deform_conv_packed_weight(w, build=False) is None
    out = deform_conv2d_nhwc(x, om, w, bias, groups=4, relu=True)
    assert out.is_contiguous(memory_format=cl) and out.shape == (2, 128, 6, 7)
    assert torch.equal(out.cpu().contiguous().view(torch.int16), want[(True, True)].view(torch.int16))
    packed = deform_conv_packed_weight(w, build=False)
    assert packed is not None
    deform_conv2d_nhwc(x, om, w, None, groups=4)
    assert deform_conv_packed_weight(w, build=False) is packed                   # reused, not rebuilt
    # a weight never seen, under capture: refused, nothing packed; the known weight replays with the eager bits
    w2 = (lat["weight"] * 0.5).half().cuda()
    static = torch.empty_like(out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            deform_conv2d_nhwc(x, om, w2, None, groups=4)
        static.copy_(deform_conv2d_nhwc(x, om, w, bias, groups=4, relu=True))
    assert deform_conv_packed_weight(w2, build=False) is None
    static.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.view(torch.int16), out.view(torch.int16))
    # an in-place change of the weight: the pack follows its version
    with torch.no_grad():
        w.mul_(0.5)
    assert deform_conv_packed_weight(w, build=False) is None
    half = deform_conv2d_nhwc(x, om, w, None, groups=4)
    assert torch.equal(half.cpu().contiguous().double(), (U.dcn_ref(lat["x"], lat["offset"], ones, lat["weight"] * 0.5, None,
                                                                   1, 1, 1, 4, 1)).half().double())
    # an empty batch, and the rows of the package's offset convolution as they come
    empty = deform_conv2d_nhwc(x[:0], om[:0], w, None, groups=4)
    assert empty.shape == (0, 128, 6, 7)
    wo = torch.zeros(18, 128, 3, 3, dtype=torch.float16, device="cuda")
    bo = (torch.arange(18, device="cuda").float() / 8 - 1).half()
    rows = conv_offset_nhwc(x, wo, bo)                                           # constant offsets = the bias
    got = deform_conv2d_nhwc(x, rows, w, None, groups=4)
    off = bo.float().cpu().view(1, 18, 1, 1).expand(2, 18, 6, 7)
    ref = U.dcn_ref(lat["x"], off, ones, lat["weight"] * 0.5, None, 1, 1, 1, 4, 1)
    A = U.dcn_ref(lat["x"].abs(), off, ones, (lat["weight"] * 0.5).abs(), None, 1, 1, 1, 4, 1)
    bound = (2.0 ** -11 + (9 * 32 + 8) * 2.0 ** -24) * A + 2.0 ** -11 * ref.abs() + 2.0 ** -25 * 10
    assert bool(((got.cpu().double() - ref).abs() <= bound).all())
    with pytest.raises(ValueError):
        deform_conv2d_nhwc(x.contiguous(), om, w, None, groups=4)                # not channels-last
