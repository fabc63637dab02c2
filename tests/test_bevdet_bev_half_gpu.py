"""BEVDet's BEV half on this package's kernels (BEVDet(bev_half="hip")): the two glue kernels of csrc/lss_split.hip
against float64 references computed here from the fp16 inputs, the merged heads and the decode on channel slices bit
for bit against the per-head / contiguous forms, the whole frame against the fp32 reference path, the absence of
framework glue behind the image neck, and the capture guard."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden
from util_bevpool import index_add_reference

pytestmark = pytest.mark.gpu

F16 = 1
MARGIN = 64        # poisoned halves in front of and behind every output (a multiple of 8: the payload stays 16-byte aligned)


def _lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _poisoned(numel):
    """A NaN-filled fp16 buffer with `numel` payload halves between two margins -> (buffer, payload view)."""
    buf = torch.full((numel + 2 * MARGIN,), float("nan"), dtype=torch.float16, device="cuda")
    return buf, buf[MARGIN:MARGIN + numel]


def _margins_intact(buf, numel):
    return bool(torch.isnan(buf[:MARGIN]).all()) and bool(torch.isnan(buf[MARGIN + numel:]).all())


# ------------------------------------------------------------------------------------------ (a) lss_depth_split
SPLIT_CASES = [  # n, hw, D, C, row_stride, depth_offset, feat_offset
    (2, 15, 5, 8, 16, 8, 0),
    (1, 1, 59, 64, 128, 64, 0),
    (3, 77, 64, 16, 96, 16, 0),
    (2, 33, 118, 64, 192, 64, 0),
    (6, 704, 59, 64, 128, 64, 0),          # the R50 frame: 6 cameras of 16 x 44 pixels
    (1, 70, 59, 64, 128, 0, 64),           # the features BEHIND the depth columns
]


def _split_input(n, hw, D, C, stride, doff, foff, seed):
    """Rows of normal logits and features; the first rows are the edge cases; every unused column is NaN."""
    g = torch.Generator().manual_seed(seed)
    rows = n * hw
    x = torch.full((rows, stride), float("nan"), dtype=torch.float16)
    x[:, doff:doff + D] = (torch.randn(rows, D, generator=g) * 3).half()
    x[:, foff:foff + C] = torch.randn(rows, C, generator=g).half()
    special = [torch.full((D,), 1.25),                                               # all equal
               torch.cat([torch.tensor([30.0]), torch.zeros(D - 1)]) - 2.0,          # one entry 30 above the rest
               torch.tensor([65504.0, -65504.0]).repeat(D)[:D],                      # the ends of binary16
               torch.zeros(D)]                                                       # a row of zeros
    if D > 2:
        special[1] = special[1].roll(D // 2)
    for i, row in enumerate(special[: min(4, rows)]):
        x[(i * 7) % rows if rows >= 28 else i, doff:doff + D] = row.half()
    if rows == 1:
        x[0, doff:doff + D] = special[2].half()
    return x


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_lss_depth_split(case):
    n, hw, D, C, stride, doff, foff = case
    x = _split_input(*case, seed=hw + D).cuda()
    x0 = x.clone()
    dbuf, depth = _poisoned(n * D * hw)
    fbuf, feat = _poisoned(n * hw * C)
    st = _lib().bevops_lss_depth_split(F16, x.data_ptr(), depth.data_ptr(), feat.data_ptr(), n, hw, stride, doff, D,
                                       foff, C, _stream())
    torch.cuda.synchronize()
    assert st == 0
    assert _margins_intact(dbuf, n * D * hw) and _margins_intact(fbuf, n * hw * C)
    assert torch.equal(x.view(torch.int16), x0.view(torch.int16))                     # the input, pad columns included
    # features: bit for bit
    assert torch.equal(feat.view(n * hw, C).view(torch.int16), x0[:, foff:foff + C].contiguous().view(torch.int16))
    # depth: the float64 softmax of the fp16 logits, rounded once (numpy rounds float64 -> float16 directly), or one of
    # that value's two binary16 neighbours
    z = x0[:, doff:doff + D].cpu().numpy().astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    r = p.astype(np.float16)
    lo, hi = np.nextafter(r, np.float16(-np.inf)), np.nextafter(r, np.float16(np.inf))
    got = depth.view(n, D, hw).permute(0, 2, 1).reshape(n * hw, D).cpu().numpy()       # back to pixel rows
    assert np.isfinite(got).all()
    ok = (got == r) | (got == lo) | (got == hi)
    off = int((got != r).sum())
    print(f"lss_depth_split {case}: {off} of {got.size} values one binary16 step from the rounded float64 softmax")
    assert ok.all(), (int((~ok).sum()), np.abs(got.astype(np.float64) - p)[~ok].max())
    sums = got.astype(np.float64).sum(axis=1)
    print(f"  row sums in [{sums.min():.6f}, {sums.max():.6f}], bound 1 +- {D * 2.0 ** -11:.6f}")
    assert np.abs(sums - 1.0).max() <= D * 2.0 ** -11
    # the wrapper returns the same bits in the shapes the pooling takes
    from bevformer_tensorrt_amd import functions as fn
    d2, f2 = fn.lss_depth_split(x0, n, D, C, doff, foff)
    assert d2.shape == (n, D, hw) and f2.shape == (n, hw, C)
    assert torch.equal(d2.view(-1).view(torch.int16), depth.view(torch.int16))
    assert torch.equal(f2.view(-1).view(torch.int16), feat.view(torch.int16))


def test_lss_depth_split_status_codes():
    lib = _lib()
    x = torch.zeros(64, 512, dtype=torch.float16, device="cuda")
    d = torch.zeros(64 * 512, dtype=torch.float16, device="cuda")
    f = torch.zeros(64 * 512, dtype=torch.float16, device="cuda")
    call = lambda dt, n, hw, stride, doff, D, foff, C: lib.bevops_lss_depth_split(
        dt, x.data_ptr(), d.data_ptr(), f.data_ptr(), n, hw, stride, doff, D, foff, C, _stream())
    assert call(0, 2, 15, 16, 8, 5, 0, 8) == 3               # BEVOPS_F32
    assert call(F16, 2, 15, 512, 0, 257, 264, 8) == 3        # D = 257
    assert call(F16, 2, 15, 32, 16, 5, 0, 12) == 2           # C = 12
    assert call(F16, 2, 15, 32, 16, 5, 4, 8) == 2            # feat_offset = 4
    assert call(F16, 2, 15, 16, 4, 5, 0, 8) == 2             # overlapping ranges
    assert call(F16, 2, 0, 16, 8, 5, 0, 8) == 0              # hw = 0
    assert call(F16, 2, 15, 16, 8, 5, 0, 8) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ (b) upsample_bilinear_concat_nhwc
UPSAMPLE_CASES = [  # (hb, wb), (h, w), (ca, cb), n
    ((3, 2), (12, 8), (8, 16), 2),
    ((5, 7), (10, 14), (0, 8), 1),
    ((3, 3), (7, 5), (16, 8), 1),           # non-integer factor
    ((1, 4), (4, 4), (8, 8), 1),            # one source row
    ((2, 2), (1, 1), (0, 8), 1),            # h = w = 1
    ((4, 4), (4, 4), (8, 8), 1),            # identity: b bit for bit
    ((16, 16), (64, 64), (128, 512), 1),    # R50: the x4 step with the concatenation
    ((64, 64), (128, 128), (0, 512), 1),    # R50: the x2 step
]


def _axis64(dst, src):
    """Output index -> (i0, i1, weight of i1) of align_corners=True in exact integer / float64 arithmetic."""
    o = torch.arange(dst, dtype=torch.int64, device="cuda")
    if dst == 1:
        z = torch.zeros(1, dtype=torch.int64, device="cuda")
        return z, z, torch.zeros(1, dtype=torch.float64, device="cuda")
    num = o * (src - 1)
    i0 = num // (dst - 1)
    lam = (num - i0 * (dst - 1)).double() / (dst - 1)
    return i0, torch.clamp(i0 + 1, max=src - 1), lam


def _ulps(a, b):
    """Distance in binary16 steps between two finite fp16 tensors."""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("case", UPSAMPLE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}c{c[2][0]}+{c[2][1]}")
def test_upsample_bilinear_concat(case):
    (hb, wb), (h, w), (ca, cb), n = case
    g = torch.Generator().manual_seed(hb * 100 + h)
    b = torch.randn(n, hb, wb, cb, generator=g).half().cuda()                          # NHWC memory
    a = torch.randn(n, h, w, ca, generator=g).half().cuda() if ca else None
    ct = ca + cb
    obuf, out = _poisoned(n * h * w * ct)
    st = _lib().bevops_upsample_bilinear_concat_nhwc(F16, a.data_ptr() if ca else None, b.data_ptr(), out.data_ptr(),
                                                     n, h, w, ca, hb, wb, cb, _stream())
    torch.cuda.synchronize()
    assert st == 0
    assert _margins_intact(obuf, n * h * w * ct)
    out = out.view(n, h, w, ct)
    if ca:
        assert torch.equal(out[..., :ca].contiguous().view(torch.int16), a.view(torch.int16))
    got = out[..., ca:]
    assert torch.isfinite(got).all()
    # float64 reference from the fp16 inputs
    y0, y1, ly = _axis64(h, hb)
    x0, x1, lx = _axis64(w, wb)
    b64 = b.double()
    c00, c01 = b64[:, y0][:, :, x0], b64[:, y0][:, :, x1]
    c10, c11 = b64[:, y1][:, :, x0], b64[:, y1][:, :, x1]
    ly, lx = ly.view(1, h, 1, 1), lx.view(1, 1, w, 1)
    ref = (1 - ly) * ((1 - lx) * c00 + lx * c01) + ly * ((1 - lx) * c10 + lx * c11)
    cmax = torch.stack([c00.abs(), c01.abs(), c10.abs(), c11.abs()]).amax(0)
    bound = 2.0 ** -11 * ref.abs() + 2.0 ** -14 * cmax + 2.0 ** -24
    err = (got.double() - ref).abs()
    print(f"upsample {case}: max err / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err - bound).max().item()
    # align_corners: the corner pixels of the output are the corner pixels of b
    for yo, ys in ((0, 0), (h - 1, hb - 1 if h > 1 else 0)):
        for xo, xs in ((0, 0), (w - 1, wb - 1 if w > 1 else 0)):
            assert torch.equal(got[:, yo, xo].contiguous().view(torch.int16), b[:, ys, xs].contiguous().view(torch.int16))
    if (hb, wb) == (h, w):
        assert torch.equal(got.contiguous().view(torch.int16), b.view(torch.int16))
    # the wrapper: the same bits as a channels-last [n, ct, h, w] tensor
    from bevformer_tensorrt_amd import functions as fn
    a4 = a.permute(0, 3, 1, 2) if ca else None
    o2 = fn.upsample_bilinear_concat_nhwc(a4, b.permute(0, 3, 1, 2), size=(h, w))
    assert o2.shape == (n, ct, h, w) and o2.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(o2.permute(0, 2, 3, 1).contiguous().view(torch.int16), out.contiguous().view(torch.int16))
    # information only: the framework's own statement on the device
    want = F.interpolate(b.permute(0, 3, 1, 2), size=(h, w), mode="bilinear", align_corners=True)
    if ca:
        want = torch.cat([a4, want], 1)
    d = _ulps(o2.contiguous(), want.contiguous())
    print(f"  vs torch.cat / F.interpolate on the device: {(d != 0).float().mean().item() * 100:.3f} % of the elements "
          f"differ, by at most {int(d.max())} binary16 steps")


def test_upsample_bilinear_concat_status_codes():
    lib = _lib()
    t = torch.zeros(4096, dtype=torch.float16, device="cuda")
    p = t.data_ptr()
    up = lib.bevops_upsample_bilinear_concat_nhwc
    assert up(F16, p, p, p, 1, 4, 4, 8, 2, 2, 12, _stream()) == 2          # cb = 12
    assert up(F16, None, p, p, 1, 4, 4, 8, 2, 2, 8, _stream()) == 2        # a == NULL with ca > 0
    assert up(0, p, p, p, 1, 4, 4, 8, 2, 2, 8, _stream()) == 3             # fp32
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (c) merged heads
@pytest.mark.parametrize("hw", [(9, 11), (128, 128)], ids=["9x11", "128x128"])
def test_merged_heads_equal_the_heads_alone(hw):
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.bevdet import HEADS_R50, merge_heads
    g = torch.Generator().manual_seed(5)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).half().cuda()
    first = [(r(64, 64, 3, 3, k=0.05), r(64, k=0.1)) for _ in HEADS_R50]
    final = [(r(c, 64, 3, 3, k=0.05), r(c, k=0.1)) for _, c in HEADS_R50]
    s = r(1, 64, *hw).contiguous(memory_format=torch.channels_last)
    w1, b1, w2, b2, slices = merge_heads(first, final)
    packed = fn.conv_nhwc(fn.conv_nhwc(s, w1, b1, True), w2, b2, False)
    assert packed.shape == (1, 32, *hw) and packed.is_contiguous(memory_format=torch.channels_last)
    for (name, c), (wa, ba), (wb, bb), (lo, hi) in zip(HEADS_R50, first, final, slices):
        c8 = (c + 7) // 8 * 8                     # padded to 8 output channels (the heat map's 10: to 16)
        wb8, bb8 = wb.new_zeros(c8, 64, 3, 3), bb.new_zeros(c8)
        wb8[:c], bb8[:c] = wb, bb
        alone = fn.conv_nhwc(fn.conv_nhwc(s, wa, ba, True), wb8, bb8, False)
        assert torch.equal(packed[:, lo:hi].contiguous().view(torch.int16), alone[:, :c].contiguous().view(torch.int16)), name
        assert not alone[:, c:].any()
    assert not packed[:, 20:].any()
    assert packed[:, :20].abs().max() > 0.1                                            # (not a comparison of zeros)


# ---------------------------------------------------------------------------------------------- (d) decode on slices
def _decode(maps, max_num):
    from bevformer_tensorrt_amd import functions as fn
    from bevformer_tensorrt_amd.bevdet import CENTERPOINT_CODER_R50 as K
    return fn.centerpoint_decode(*maps, max_num=max_num, post_center_range=K["post_center_range"], pc_range=K["pc_range"],
                                 out_size_factor=K["out_size_factor"], voxel_size=K["voxel_size"],
                                 score_threshold=K["score_threshold"], norm_bbox=True, padded=True)


@pytest.mark.parametrize("batch,hw,max_num", [(1, 16, 100), (1, 128, 500), (2, 16, 100)], ids=["16x16", "128x128", "batch2"])
def test_decode_on_channel_slices(batch, hw, max_num):
    from bevformer_tensorrt_amd.bevdet import HEADS_R50
    g = torch.Generator().manual_seed(7)
    packed = (torch.randn(batch, hw, hw, 32, generator=g) * 0.7).half().cuda().permute(0, 3, 1, 2)
    slices, at = [], 0
    for _, c in HEADS_R50:
        slices.append(packed[:, at:at + c])
        at += c
    assert not any(s.is_contiguous() or s.is_contiguous(memory_format=torch.channels_last) for s in slices)
    got = _decode(slices, max_num)
    want = _decode([s.contiguous() for s in slices], max_num)
    torch.cuda.synchronize()
    assert int(want[3].min()) > 0                                                      # boxes were kept
    for name, a, b in zip(("boxes", "scores", "labels", "count"), got, want):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ---------------------------------------------------------------------------------------------------- (e) the frame
class _OraclePoolOps:
    """Operator namespace of the REFERENCE data path of the whole detector: library convolutions (no fused entries
    here, so bevdet._conv takes F.conv2d) and the oracle statement of bev_pool_v2 (torch.index_add_, fp64)."""

    @staticmethod
    def bev_pool_v2_2(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, bev_h, bev_w):
        want = index_add_reference(depth.float().cpu().numpy(), feat.float().cpu().numpy(), ranks_depth.cpu().numpy(),
                                   ranks_feat.cpu().numpy(), ranks_bev.cpu().numpy(), bev_h, bev_w)
        return torch.from_numpy(want).to(depth.device, depth.dtype)


@pytest.fixture(scope="module")
def frame():
    """The two fp16 models on one state dict, the fp32 reference path's outputs, the frame's inputs: built once."""
    from bevformer_tensorrt_amd.bevdet import BEVDet
    g = golden("bevdet_geometry")
    t = lambda k: torch.from_numpy(g[k])
    hip = BEVDet(seed=0, bev_half="hip").cuda().half()
    tor = BEVDet(seed=0, bev_half="torch").cuda().half()
    tor.load_state_dict(hip.state_dict())
    ref = BEVDet(ops=_OraclePoolOps, seed=0, bev_half="torch").cuda().float()
    ref.load_state_dict({k: v.float() for k, v in hip.state_dict().items()})
    geom = (t("sensor2ego"), None, t("cam2imgs"), t("post_rots"), t("post_trans"), t("bda"))
    ranks = [r.cuda() for r in hip.view.get_bev_pool_input(*geom)]
    calib = hip.view.calibration_matrices(*geom).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda()
    want = ref(img, *ranks)
    del ref
    return dict(hip=hip, torch=tor, ranks=ranks, calib=calib, img=img.half(), want=want)


NAMES = ("reg", "height", "dim", "rot", "vel", "heatmap")


def test_frame_against_the_fp32_reference_path(frame):
    from bevformer_tensorrt_amd.bevdet import HEADS_R50
    # (a frame in front of the two that are compared; whether it has their bits too is printed, not asserted)
    first = [o.clone() for o in frame["hip"](frame["img"], *frame["ranks"])]
    got = frame["hip"](frame["img"], *frame["ranks"])
    again = frame["hip"](frame["img"], *frame["ranks"])
    plain = frame["torch"](frame["img"], *frame["ranks"])
    torch.cuda.synchronize()
    print("first frame of the process equal to the second:", [bool(torch.equal(a, b)) for a, b in zip(first, got)])
    # the BEV half alone, twice on the same image features: equal bits
    x = frame["hip"].image_features(frame["img"].flatten(0, 1))
    h1 = [o.clone() for o in frame["hip"].bev_half_calibrated(x, frame["calib"])]
    h2 = frame["hip"].bev_half_calibrated(x, frame["calib"])
    for n, a, b in zip(NAMES, h1, h2):
        assert torch.equal(a.view(torch.int16), b.contiguous().view(torch.int16)), n
    for (n, c), a, a2, b, p in zip(HEADS_R50, got, again, frame["want"], plain):
        assert a.shape == b.shape == p.shape == (1, c, 128, 128) and a.dtype == torch.float16, n
        err = (a.float() - b).abs().max().item()
        bar = 3e-2 * max(1.0, b.abs().max().item())
        print(f"{n}: hip vs fp32 reference {err:.4e} (bar {bar:.4e}); torch path vs reference "
              f"{(p.float() - b).abs().max().item():.4e}; hip vs torch fp16 {(a.float() - p.float()).abs().max().item():.4e}")
        assert err <= bar, (n, err, bar)
        assert torch.equal(a.contiguous().view(torch.int16), a2.contiguous().view(torch.int16)), n   # two eager runs: equal bits
    # the six outputs are channel slices of ONE packed tensor: no copy
    base = got[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in got)
    assert got[5].stride() == (128 * 128 * 32, 1, 128 * 32, 32)


def test_frame_replays_from_a_graph_to_the_same_bits(frame):
    model = frame["hip"]
    static, calib = frame["img"].clone(), frame["calib"].clone()
    eager = [o.clone() for o in model.forward_calibrated(static, calib)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.forward_calibrated(static, calib)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = model.forward_calibrated(static, calib)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, outs, eager):
        assert torch.equal(a.contiguous().view(torch.int16), b.view(torch.int16)), n
    # the decode reads the slices in place and agrees with their copies
    cand = model.get_candidates(outs, padded=True)
    cand2 = model.get_candidates(tuple(o.contiguous() for o in outs), padded=True)
    for a, b in zip(cand, cand2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------ (f) no framework glue
class _Probe(torch.overrides.TorchFunctionMode):
    """Counts, while `active`, the framework calls the issue names: library convolutions, interpolate, cat, softmax and
    every contiguous() that returns new storage."""
    CONV = (torch.conv2d, F.conv2d, torch.convolution, torch._convolution)
    SOFTMAX = (torch.Tensor.softmax, torch.softmax, F.softmax, torch._softmax)

    def __init__(self):
        super().__init__()
        self.active = False
        self.counts = dict(conv2d=0, interpolate=0, cat=0, softmax=0, contiguous=0)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if self.active:
            if func in self.CONV:
                self.counts["conv2d"] += 1
            elif func is F.interpolate:
                self.counts["interpolate"] += 1
            elif func in (torch.cat, torch.concat, torch.concatenate):
                self.counts["cat"] += 1
            elif func in self.SOFTMAX:
                self.counts["softmax"] += 1
            elif func is torch.Tensor.contiguous and \
                    out.untyped_storage().data_ptr() != args[0].untyped_storage().data_ptr():
                self.counts["contiguous"] += 1
        return out


def _probe_bev_half(model, img, calib):
    """The counts of one forward_calibrated, from the moment image_features returns."""
    probe = _Probe()
    inner = model.image_features

    def image_features(image):
        out = inner(image)
        probe.active = True
        return out

    model.image_features = image_features
    try:
        with probe:
            model.forward_calibrated(img, calib)
    finally:
        probe.active = False
        del model.image_features
    torch.cuda.synchronize()
    return probe.counts


def test_no_framework_glue_behind_the_image_neck(frame):
    from bevformer_tensorrt_amd.functions import conv as C
    for m in (frame["hip"], frame["torch"]):
        m.forward_calibrated(frame["img"], frame["calib"])           # (warm: choices made, merged operands built)
    misses = list(C.CONV_MISSES)
    counts = _probe_bev_half(frame["hip"], frame["img"], frame["calib"])
    print("hip  :", counts)
    assert counts == dict(conv2d=0, interpolate=0, cat=0, softmax=0, contiguous=0)
    assert C.CONV_MISSES == misses
    merged = [p for p in C.CONV_MISSES if ",64,384,3," in p or ",384,32,3," in p]
    assert not merged, merged
    counts = _probe_bev_half(frame["torch"], frame["img"], frame["calib"])
    print("torch:", counts)
    assert all(v >= 1 for v in counts.values()), counts              # the probe sees every one of them


# ------------------------------------------------------------------------------------------------ (g) capture guard
def test_capture_guard_and_weight_reload():
    from bevformer_tensorrt_amd.bevdet import BEVDet, synthetic_rig
    model = BEVDet(seed=0, bev_half="hip").cuda().half()
    calib = model.view.calibration_matrices(*synthetic_rig(model.view)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(2)).cuda().half()
    scratch = torch.zeros(8, device="cuda")
    assert model.heads_merged(build=False) is None and model.view.depth_net_merged(build=False) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.forward_calibrated(img, calib)                     # raises before it launches anything
        with pytest.raises(RuntimeError):
            model.prepare_bev_half()
    del graph
    assert model.heads_merged(build=False) is None                   # nothing was built inside the capture
    # after an eager call the capture succeeds
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [o.clone() for o in model.forward_calibrated(img, calib)]
    torch.cuda.current_stream().wait_stream(s)
    assert model.heads_merged(build=False) is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = model.forward_calibrated(img, calib)
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, outs, eager):
        assert torch.equal(a.contiguous().view(torch.int16), b.view(torch.int16)), n
    del graph, outs
    # new head weights: height's final convolution becomes the constant 0.5, every other head keeps its bits
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["heads.height.1.weight"].zero_()
    sd["heads.height.1.bias"].fill_(0.5)
    model.load_state_dict(sd)
    assert model.heads_merged(build=False) is None                   # stale
    new = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, new, eager):
        if n == "height":
            assert bool((a == 0.5).all())
        else:
            assert torch.equal(a.contiguous().view(torch.int16), b.view(torch.int16)), n
