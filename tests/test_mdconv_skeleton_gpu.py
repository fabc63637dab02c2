"""The fp16 LDS-DMA DCNv2 kernel's skeleton: sampling footprints from a per-block LDS table (128-pixel tiles) and
channels-last outputs stored as whole pixel rows through LDS, against the A/B partner that keeps the previous skeleton
(per-thread footprints, per-lane stores: bevops_mdconv_set_variant 10 / 14 / 15 = 0 / 4 / 5 with it; 20 / 24 / 25 = the
table with per-lane stores).  Both skeletons run the same arithmetic in the same order, so every comparison between
them is torch.equal; the float64 comparison uses the bound of test_mdconv_nhwc_gpu."""
import functools

import pytest
import torch

import util_dcn as U
from test_mdconv_gpu import make
from test_mdconv_nhwc_gpu import _cl, _fp16_bound, _mismatch, variant

pytestmark = pytest.mark.gpu

# (B, Cin, Cout, H, W, K, stride, pad, dil, groups, deform_groups): the smallest shapes at which each piece can go wrong
CASES = {
    "ragged-35px": (1, 64, 64, 5, 7, 3, 1, 1, 1, 1, 1),           # one tile, 93 of 128 pixels invalid
    "stride2-two-images": (2, 128, 128, 9, 13, 3, 2, 1, 1, 1, 1),  # 70 pixels, two k-chunks per tap
    "two-tiles": (2, 64, 64, 9, 13, 3, 1, 1, 1, 1, 1),             # 234 pixels: a full and a ragged 128-pixel tile
    "cout72": (1, 64, 72, 5, 7, 3, 1, 1, 1, 1, 1),                 # rows past cout_g in the Cout tile
    "cout260": (1, 64, 260, 5, 7, 3, 1, 1, 1, 1, 1),               # two Cout tiles; cout_g % 8 != 0: per-lane stores
    "groups2-dg2": (1, 128, 256, 7, 9, 3, 1, 1, 1, 2, 2),          # dg indexing of the table's offset loads
    "dilation2": (1, 64, 64, 9, 11, 3, 1, 2, 2, 1, 1),
    "k1": (1, 64, 64, 5, 7, 1, 1, 0, 1, 1, 1),                     # a one-tap table
    "k5": (1, 64, 64, 7, 9, 5, 1, 2, 1, 1, 1),                     # 25 taps do not fit: per-thread footprints
}
OFF_STD = 3.0    # against 5 .. 13 pixel images: many corners, and whole footprints, fall outside
PAIRS = ((0, 10), (5, 15), (20, 10), (25, 15))   # (skeleton under test, its parent-skeleton partner)


@pytest.fixture(scope="module")
def bev():
    import bevformer_tensorrt_amd as b
    return b


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """fp16 operands of a case (made once, shared, never modified): planar offset / mask and, for one deform group,
    the raw offset-convolution layout with 3 KK (+ 1 when odd) channels: offsets, mask logits, one channel of junk."""
    B, Cin, Cout, H, W, K, s, p, d, G, DG = CASES[name]
    x, off, mask, w, b = (t.half() for t in make(B, Cin, Cout, H, W, K, s, p, d, G, DG, seed=11, off_std=OFF_STD))
    om = None
    if DG == 1:
        kk = K * K
        gen = torch.Generator().manual_seed(12)
        om = torch.randn(B, 3 * kk + (3 * kk) % 2, off.shape[2], off.shape[3], generator=gen) * 1.5
        om[:, :2 * kk] = off
        om = om.half()
    return x, off, mask, w, b, om


def _outside_counts(name):
    """(whole footprints outside, footprints with some but not all corners outside) from the drawn fp16 offsets"""
    B, Cin, Cout, H, W, K, s, p, d, G, DG = CASES[name]
    off = _inputs(name)[1].double()
    Ho, Wo = off.shape[2:]
    base_h = (torch.arange(Ho, dtype=torch.float64) * s - p).view(1, Ho, 1)
    base_w = (torch.arange(Wo, dtype=torch.float64) * s - p).view(1, 1, Wo)
    whole = part = 0
    for t in range(DG * K * K):
        i, j = divmod(t % (K * K), K)
        h, w = base_h + i * d + off[:, 2 * t], base_w + j * d + off[:, 2 * t + 1]
        live = (h > -1) & (h < H) & (w > -1) & (w < W)
        h0, w0 = torch.floor(h), torch.floor(w)
        cut = (h0 < 0) | (h0 + 1 > H - 1) | (w0 < 0) | (w0 + 1 > W - 1)
        whole += int((~live).sum())
        part += int((live & cut).sum())
    return whole, part


def _runs(bev, name):
    """name -> callables (relu, with_bias) -> output, one per entry the case can take"""
    B, Cin, Cout, H, W, K, s, p, d, G, DG = CASES[name]
    x, off, mask, w, b, om = _inputs(name)
    xg, og, mg, wg, bg, xc = x.cuda(), off.cuda(), mask.cuda(), w.cuda(), b.cuda(), _cl(x)
    runs = {"nchw": lambda relu, wb: bev.modulated_deformable_conv2d(xg, og, mg, wg, bg if wb else None, s, p, d, G, DG)}
    if om is not None:
        omc = _cl(om)
        runs["nhwc-om"] = lambda relu, wb: bev.modulated_deformable_conv2d_nhwc(
            xc, None, None, wg, bg if wb else None, s, p, d, G, DG, relu=relu, offset_mask_nhwc=omc)
    else:   # the raw layout is that of ONE deform group: planar operands through the channels-last entry
        runs["nhwc-planar"] = lambda relu, wb: bev.modulated_deformable_conv2d_nhwc(
            xc, og, mg, wg, bg if wb else None, s, p, d, G, DG, relu=relu)
    return runs


@pytest.mark.parametrize("name", list(CASES))
def test_new_skeleton_equals_parent_skeleton(bev, name):
    """Planner's choice (0 vs 10), forced 128-pixel tiles (5 vs 15: the table wherever it fits) and the table with
    per-lane stores (20 / 25): bit-equal through the NCHW drop-in and the channels-last entry, ReLU on / off (the drop-in
    has none), bias / none.  The 3 x 3 cases must hold whole footprints outside the image and partly cut ones."""
    if CASES[name][5] == 3:
        whole, part = _outside_counts(name)
        assert whole > 0 and part > 0, (whole, part)
    for entry, fn in _runs(bev, name).items():
        for relu in ((False,) if entry == "nchw" else (False, True)):
            for wb in (True, False):
                for new, parent in PAIRS:
                    with variant(parent):
                        want = fn(relu, wb)
                    with variant(new):
                        got = fn(relu, wb)
                    assert got.shape == want.shape and got.stride() == want.stride()
                    assert torch.isfinite(want).all() and want.abs().max() > 0
                    assert torch.equal(got, want), (entry, relu, wb, new, parent, _mismatch(got.cpu(), want.cpu()))


def test_split_k_tail_runs_with_the_table(bev):
    """B = 1, Cin = Cout = 64, (CUs + 10) x 127 pixels: a round of one 128-pixel block per CU and a few tiles left over,
    which plan_tail splits along K -- tail blocks build only their own taps' records, the finish kernel stores.
    Bit-equal to the parent skeleton with the same tail, ReLU and bias, raw offset-convolution layout."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Hn, Wn, C = cus + 10, 127, 64
    tiles = (Hn * Wn + 127) // 128
    left = tiles % cus
    if not (tiles > cus and 0 < left and 2 * left <= cus and 3 * left <= cus):
        pytest.skip(f"{tiles} tiles on {cus} CUs leave {left}: no split-K tail at this shape")
    x, off, _, w, b = (t.half() for t in make(1, C, C, Hn, Wn, 3, 1, 1, 1, 1, 1, seed=13, off_std=OFF_STD))
    om = torch.randn(1, 28, Hn, Wn, generator=torch.Generator().manual_seed(14)) * 1.5
    om[:, :18] = off
    xc, wc, bc, omc = _cl(x), w.cuda(), b.cuda(), _cl(om.half())
    call = lambda: bev.modulated_deformable_conv2d_nhwc(xc, None, None, wc, bc, 1, 1, 1, 1, 1, relu=True, offset_mask_nhwc=omc)
    with variant(10):
        want = call()
    with variant(14):
        no_tail = call()
    got = call()
    assert torch.equal(got, want), _mismatch(got.cpu(), want.cpu())
    assert not torch.equal(want, no_tail)     # the tail's fp32 summation order differs: it did run
    with variant(20):
        assert torch.equal(call(), want)


@pytest.mark.parametrize("entry", ["nchw", "nhwc-om"])
def test_new_skeleton_vs_float64_reference(bev, entry):
    """One case per entry (two images, stride 2, two k-chunks, 128-pixel tiles forced so that the table runs) against
    dcn_ref under the project's fp16 bound."""
    name = "stride2-two-images"
    B, Cin, Cout, H, W, K, s, p, d, G, DG = CASES[name]
    x, off, mask, w, b, om = _inputs(name)
    with variant(5):
        got = _runs(bev, name)[entry](entry != "nchw", True)
    if entry == "nchw":
        want = U.dcn_ref(x, off, mask, w, b, s, p, d, G, DG)
    else:
        om_off, om_mask = U.unpack_offset_mask(om)
        want = U.dcn_ref(x, om_off, om_mask, w, b, s, p, d, G, DG, relu=True)
    _fp16_bound(got, want)


def test_new_skeleton_under_graph_capture(bev):
    """The frame launches the call from a captured HIP graph: capture and two replays give the eager parent's bits."""
    name = "two-tiles"
    fn = _runs(bev, name)["nhwc-om"]
    with variant(15):
        want = fn(True, True).clone()
    with variant(5):
        fn(True, True)                      # packs the weights and sizes the workspace outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = fn(True, True)
    for _ in range(2):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want), _mismatch(got.cpu(), want.cpu())
