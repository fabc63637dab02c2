"""DCNv2 operator tests against the float64 reference of util_dcn.py: the channels-last entry the model's frame
calls (modulated_deformable_conv2d_nhwc, planar offsets or the raw offset-convolution output, fused sigmoid / ReLU),
the plugin entry and the INT8 entry.

Lattice inputs (util_dcn.lattice): taps sit exactly on -1, 0, H - 1, H, half a pixel beside them and far outside, and
all values are chosen so that a correct kernel rounds nowhere before its final store (test_dcn_reference_cpu.py
shows that premise on the reference alone).  Every lattice comparison is therefore torch.equal against
dcn_ref rounded to nearest-even in the output type -- no tolerance."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import util_dcn as U
from test_mdconv_gpu import make

pytestmark = pytest.mark.gpu

B, H, W = U.LATTICE_B, U.LATTICE_H, U.LATTICE_W
CASES = [(cin, cout, geom, 1, 1) for (cin, cout) in U.LATTICE_CHANNELS for geom in U.LATTICE_GEOM] + [(128, 8, (1, 1, 1), 2, 2)]
IDS = [f"cin{c}-cout{o}-s{g[0]}p{g[1]}d{g[2]}-g{gr}dg{dg}" for c, o, g, gr, dg in CASES]


@pytest.fixture(scope="module")
def bev():
    import bevformer_tensorrt_amd as b
    return b


@contextlib.contextmanager
def variant(v):
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    lib.bevops_mdconv_set_variant(v)
    try:
        yield
    finally:
        lib.bevops_mdconv_set_variant(0)


@functools.lru_cache(maxsize=None)
def _lattice(cin, cout, geom, groups, dg):
    return U.lattice(B, cin, cout, H, W, *geom, groups, dg)


@functools.lru_cache(maxsize=None)
def _expected(cin, cout, geom, groups, dg, kind, with_bias, relu):
    """dcn_ref of the lattice case, float64 (computed once, shared, never modified).  kind: 'planar', 'om32', 'om28'."""
    lat = _lattice(cin, cout, geom, groups, dg)
    if kind == "planar":
        off, mask = lat["offset"], lat["mask"]
    else:   # the kernel's mask is the sigmoid ROUNDED TO fp16 (what the fp16 block's mask tensor holds): exactly 0, 1/2, 1 here
        off, mask = U.unpack_offset_mask(lat[kind].half())
        mask = mask.half().double()
        assert set(mask.unique().tolist()) == {0.0, 0.5, 1.0}
    return U.dcn_ref(lat["x"], off, mask, lat["weight"], lat["bias"] if with_bias else None, *geom, groups, dg, relu=relu)


def _cl(t):
    return t.half().cuda().contiguous(memory_format=torch.channels_last)


def _mismatch(got, want):
    bad = got != want
    return f"{int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[:4].tolist()}"


@pytest.mark.parametrize("cin,cout,geom,groups,dg", CASES, ids=IDS)
def test_lattice_channels_last_entry_is_exact(bev, cin, cout, geom, groups, dg):
    """(a) modulated_deformable_conv2d_nhwc with planar offset / mask and with offset_mask_nhwc at OC = 32 and 28
    (junk in the padding channels), ReLU off / on, bias / none, under variants 0, 4 (no split-K tail), 5 (128-pixel
    tiles forced), 7 and 13 (other wave orders): bit-equal to the expectation, channels-last contiguous; an
    NCHW-contiguous input gives the same bits.  The groups = deform_groups = 2 case has planar offsets only."""
    lat = _lattice(cin, cout, geom, groups, dg)
    s, p, d = geom
    x, w = _cl(lat["x"]), lat["weight"].half().cuda()
    ops = {"planar": dict(offset=lat["offset"].half().cuda(), mask=lat["mask"].half().cuda())}
    if dg == 1:
        ops["om32"] = dict(offset=None, mask=None, offset_mask_nhwc=_cl(lat["om32"]))
        ops["om28"] = dict(offset=None, mask=None, offset_mask_nhwc=_cl(lat["om28"]))
    for kind, kw in ops.items():
        for with_bias in (True, False):
            bias = lat["bias"].half().cuda() if with_bias else None
            for relu in (False, True):
                want = U.expect(_expected(cin, cout, geom, groups, dg, kind, with_bias, relu), torch.float16)
                for v in (0, 4, 5, 7, 13):
                    with variant(v):
                        got = bev.modulated_deformable_conv2d_nhwc(x, kw["offset"], kw["mask"], w, bias, s, p, d, groups, dg,
                                                                   relu=relu, offset_mask_nhwc=kw.get("offset_mask_nhwc"))
                    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
                    assert torch.equal(got.cpu(), want), (kind, with_bias, relu, v, _mismatch(got.cpu(), want))
    x_nchw = lat["x"].half().cuda()
    assert x_nchw.is_contiguous() and not x_nchw.is_contiguous(memory_format=torch.channels_last)
    got = bev.modulated_deformable_conv2d_nhwc(x_nchw, ops["planar"]["offset"], ops["planar"]["mask"], w, None, s, p, d,
                                               groups, dg)
    assert torch.equal(got.cpu(), U.expect(_expected(cin, cout, geom, groups, dg, "planar", False, False), torch.float16))


@pytest.mark.parametrize("cin,cout,geom,groups,dg", CASES + [(6, 10, (1, 1, 1), 1, 3)], ids=IDS + ["cin6-ragged-k"])
def test_lattice_plugin_entry_is_exact(bev, cin, cout, geom, groups, dg):
    """(b) The same planar inputs through modulated_deformable_conv2d: fp16 under variants 0 (LDS-DMA kernel), 1
    (im2col + GEMM), 2 / 3 (register-staged kernel, 256 / 512 threads), 5 (128-pixel tiles), and fp32; Cin = 6 is
    outside the fused domain and takes the scalar im2col and the ragged-K GEMM.  Bit-equal in their type."""
    lat = _lattice(cin, cout, geom, groups, dg)
    s, p, d = geom
    for with_bias in (True, False):
        want64 = _expected(cin, cout, geom, groups, dg, "planar", with_bias, False)
        for dtype, variants in ((torch.float16, (0, 1, 2, 3, 5)), (torch.float32, (0,))):
            x, off, mask, w = (lat[k].to(dtype).cuda() for k in ("x", "offset", "mask", "weight"))
            bias = lat["bias"].to(dtype).cuda() if with_bias else None
            want = U.expect(want64, dtype)
            for v in variants:
                with variant(v):
                    got = bev.modulated_deformable_conv2d(x, off, mask, w, bias, s, p, d, groups, dg)
                assert got.dtype == dtype and torch.equal(got.cpu(), want), (dtype, with_bias, v, _mismatch(got.cpu(), want))


@pytest.mark.parametrize("cin,cout", [(64, 8), (128, 260)])   # (the INT8 plugin takes Cout / groups % 4 == 0 only, as the reference's does)
@pytest.mark.parametrize("geom", U.LATTICE_GEOM, ids=lambda g: f"s{g[0]}p{g[1]}d{g[2]}")
def test_lattice_int8_matches_the_int8_oracle(bev, oracle_mod, cin, cout, geom):
    """(c) The lattice's tap targets as int8 offsets (scale 1/2) through modulated_deformable_conv2d_int8 under
    variants 0, 6 (im2col + GEMM), 8 (fused kernel) and 9 (LDS-DMA kernel where its domain allows) against the C
    oracle, under the criterion of test_mdconv_int8_vs_oracle: at most 1 LSB on at most 1 % of the outputs."""
    lat = _lattice(cin, cout, geom, 1, 1)
    q = U.lattice_int8(lat)
    s, p, d = geom
    s_out = float(_expected(cin, cout, geom, 1, 1, "planar", True, False).abs().max()) / 127.0
    want = oracle_mod.mdconv_s8(q["x"].numpy(), q["s_x"], q["offset"].numpy(), q["s_o"], q["mask"].numpy(), q["s_m"],
                                q["weight"].numpy(), q["s_w"], q["bias"].numpy(), s_out, (s,) * 2, (p,) * 2, (d,) * 2, 1, 1)
    want = want.astype(np.int32)
    assert np.abs(want).max() > 32
    for v in (0, 6, 8, 9):
        with variant(v):
            got = bev.modulated_deformable_conv2d_int8(q["x"].cuda(), q["offset"].cuda(), q["mask"].cuda(), q["weight"].cuda(),
                                                       q["bias"].cuda(), q["s_x"], q["s_o"], q["s_m"], q["s_w"], s_out,
                                                       s, p, d, 1, 1)
        diff = np.abs(got.cpu().numpy().astype(np.int32) - want)
        assert diff.max() <= 1 and (diff > 0).mean() <= 0.01, (v, diff.max(), (diff > 0).mean())


def _random_om(off, Bn, Ho, Wo, gen):
    om = torch.zeros(Bn, 32, Ho, Wo)
    om[:, :18] = off
    om[:, 18:27] = torch.randn(Bn, 9, Ho, Wo, generator=gen) * 1.5
    return om.half()


def _fp16_bound(got, want64):
    """The project's fp16 criterion (test_mdconv_gpu.test_mdconv_vs_oracle): max <= 1e-2 x scale, mean <= 0.05."""
    err = (got.double().cpu() - want64).abs()
    scale = max(1.0, want64.abs().max().item())
    print(f"max err {err.max().item():.4g} (bound {1e-2 * scale:.4g}), mean err {err.mean().item():.4g} (bound 0.05)")
    assert err.max().item() <= 1e-2 * scale and err.mean().item() <= 0.05, (err.max().item(), err.mean().item(), scale)
    return scale


@pytest.mark.parametrize("shape", [(2, 64, 64, 17, 19, 1), (1, 256, 256, 20, 28, 1), (2, 128, 192, 33, 47, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_random_channels_last_entry_vs_reference(bev, shape):
    """(d) Random values, offsets of std 2.5 pixels.  offset_mask_nhwc (OC = 32, as conv_offset_nhwc hands it over)
    with ReLU on and off, and planar operands, against dcn_ref under the fp16 bound; with planar offsets and no ReLU
    the channels-last entry and the plugin entry run the same kernel in the same summation order: the same bits."""
    Bn, Cin, Cout, Hn, Wn, stride = shape
    x, off, mask, w, b = (t.half() for t in make(Bn, Cin, Cout, Hn, Wn, 3, stride, 1, 1, 1, 1, seed=3, off_std=2.5))
    Ho, Wo = U.out_size(Hn, stride, 1, 1), U.out_size(Wn, stride, 1, 1)
    om = _random_om(off, Bn, Ho, Wo, torch.Generator().manual_seed(4))
    xc, wc, bc = _cl(x), w.cuda(), b.cuda()
    om_off, om_mask = U.unpack_offset_mask(om)
    for relu in (False, True):
        got = bev.modulated_deformable_conv2d_nhwc(xc, None, None, wc, bc, stride, 1, 1, 1, 1, relu=relu, offset_mask_nhwc=_cl(om))
        assert got.is_contiguous(memory_format=torch.channels_last)
        _fp16_bound(got, U.dcn_ref(x, om_off, om_mask, w, b, stride, 1, 1, 1, 1, relu=relu))
        if relu:
            assert (got >= 0).all()
    got = bev.modulated_deformable_conv2d_nhwc(xc, off.cuda(), mask.cuda(), wc, bc, stride, 1, 1, 1, 1)
    _fp16_bound(got, U.dcn_ref(x, off, mask, w, b, stride, 1, 1, 1, 1))
    plugin = bev.modulated_deformable_conv2d(x.cuda(), off.cuda(), mask.cuda(), wc, bc, stride, 1, 1, 1, 1)
    assert torch.equal(got.contiguous(), plugin), _mismatch(got.contiguous(), plugin)


def test_split_k_tail_with_the_fused_epilogue(bev):
    """(e) B = 1, Cin = Cout = 64, 184 x 184 = 265 tiles of 128 pixels.  THE SHAPE ASSUMES 256 CUs with one resident
    1024-thread block each: 256 tiles fill a round, the 9 left over are split 9 ways along K and summed by the finish
    kernel, which then applies bias and ReLU and stores channels-last (asserted below from the device's CU count, so a
    device on which the tail is not taken fails here instead of passing without it).  offset_mask_nhwc, ReLU, bias:
    within the fp16 bound of dcn_ref, within 4e-3 x scale of variant 4 (the same kernel without the tail: only the
    fp32 summation order differs -- the figure of test_lds_dma_kernel_and_split_k_tail_match_register_staged_kernel),
    bit-equal on a second call, no negative output."""
    Bn, C, Hn, Wn = 1, 64, 184, 184
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (Bn * Hn * Wn + 127) // 128
    left = tiles % cus
    assert tiles > cus and 0 < left and 2 * left <= cus and 9 * left <= cus, \
        f"{tiles} tiles on {cus} CUs leave {left}: no 9-way split-K tail at this shape (it assumes 256 CUs)"
    x, off, _, w, b = (t.half() for t in make(Bn, C, C, Hn, Wn, 3, 1, 1, 1, 1, 1, seed=5, off_std=2.5))
    om = _random_om(off, Bn, Hn, Wn, torch.Generator().manual_seed(6))
    xc, wc, bc, omc = _cl(x), w.cuda(), b.cuda(), _cl(om)
    call = lambda: bev.modulated_deformable_conv2d_nhwc(xc, None, None, wc, bc, 1, 1, 1, 1, 1, relu=True, offset_mask_nhwc=omc)
    got = call()
    with variant(4):
        no_tail = call()
    om_off, om_mask = U.unpack_offset_mask(om)
    scale = _fp16_bound(got, U.dcn_ref(x, om_off, om_mask, w, b, 1, 1, 1, 1, 1, relu=True))
    d = (got.float() - no_tail.float()).abs().max().item()
    print(f"tail vs no tail: max {d:.4g} (bound {4e-3 * scale:.4g})")
    assert d <= 4e-3 * scale
    assert torch.equal(call(), got)
    assert (got >= 0).all() and (got > 0).any()


@pytest.mark.parametrize("zero_offsets", [True, False], ids=["zero-offsets", "lattice-offsets"])
@pytest.mark.parametrize("geom", U.LATTICE_GEOM, ids=lambda g: f"s{g[0]}p{g[1]}d{g[2]}")
def test_non_finite_input_reaches_only_the_outputs_that_sample_it(bev, geom, zero_offsets):
    """(f) x[0, :, 0, 0] = +inf on the lattice inputs (Cin = 128: two K chunks) with zero offsets -- and, beyond what
    the definition needs, with the lattice's own offsets.  A corner outside the image is skipped, never multiplied by
    its zero weight: the non-finite outputs are exactly those dcn_ref has (an in-image corner on pixel (0, 0) of
    image 0), every other output is bit-equal to the expectation.  Plugin entry under variants 0, 2, 3, 5;
    channels-last entry under 0 and 5 (it has no build under 2 and 3: test_argument_checking)."""
    cin, cout = 128, 10
    lat = _lattice(cin, cout, geom, 1, 1)
    s, p, d = geom
    x = lat["x"].clone()
    x[0, :, 0, 0] = float("inf")
    off = torch.zeros_like(lat["offset"]) if zero_offsets else lat["offset"]
    want64 = U.dcn_ref(x, off, lat["mask"], lat["weight"], lat["bias"], s, p, d, 1, 1)
    bad = ~torch.isfinite(want64)
    assert bad[0].any() and not bad[1].any() and not bad.all(dim=1)[0].all()
    assert (bad.any(dim=1) == bad.all(dim=1)).all()        # a pixel that samples the inf loses all its channels
    want = U.expect(want64, torch.float16)
    xg, og, mg, wg, bg = (t.half().cuda() for t in (x, off, lat["mask"], lat["weight"], lat["bias"]))
    runs = [("plugin", v, lambda: bev.modulated_deformable_conv2d(xg, og, mg, wg, bg, s, p, d, 1, 1)) for v in (0, 2, 3, 5)]
    runs += [("nhwc", v, lambda: bev.modulated_deformable_conv2d_nhwc(_cl(x), og, mg, wg, bg, s, p, d, 1, 1)) for v in (0, 5)]
    for entry, v, fn in runs:
        with variant(v):
            got = fn().cpu()
        got_bad = ~torch.isfinite(got)
        assert torch.equal(got_bad, bad), (entry, v, int(got_bad.sum()), int(bad.sum()), (got_bad & ~bad).nonzero()[:4].tolist())
        assert torch.equal(got[~bad], want[~bad]), (entry, v)


def test_argument_checking(bev):
    """(g) What the channels-last entry refuses, each with its status; B = 0 returns an empty channels-last tensor."""
    from bevformer_tensorrt_amd.utils import lib as L
    lat = _lattice(64, 8, (1, 1, 1), 1, 1)
    x, w, off, mask = _cl(lat["x"]), lat["weight"].half().cuda(), lat["offset"].half().cuda(), lat["mask"].half().cuda()

    def status(fn):
        with pytest.raises(L.BevopsError) as e:
            fn()
        return e.value.status

    nhwc = bev.modulated_deformable_conv2d_nhwc
    for oc in (29, 26):      # odd; fewer than 3 KK channels
        om = _cl(torch.zeros(B, oc, H, W))
        assert status(lambda: nhwc(x, None, None, w, None, 1, 1, 1, 1, 1, offset_mask_nhwc=om)) == L.BAD_PARAM, oc
    x96, w96 = _cl(torch.zeros(B, 96, H, W)), torch.zeros(8, 96, 3, 3).half().cuda()
    assert status(lambda: nhwc(x96, off, mask, w96, None, 1, 1, 1, 1, 1)) == L.NOT_SUPPORTED   # outside the fused domain
    assert status(lambda: nhwc(x, off, mask, w.float(), None, 1, 1, 1, 1, 1)) == L.BAD_PARAM    # fp32 weight
    for v in (1, 2):         # builds without the fused epilogue
        with variant(v):
            assert status(lambda: nhwc(x, off, mask, w, None, 1, 1, 1, 1, 1)) == L.NOT_SUPPORTED, v
    # offset_mask_nhwc is the layout of ONE deform group
    x128, w128 = _cl(torch.zeros(B, 128, H, W)), torch.zeros(8, 64, 3, 3).half().cuda()
    om64 = _cl(torch.zeros(B, 64, H, W))
    assert status(lambda: nhwc(x128, None, None, w128, None, 1, 1, 1, 2, 2, offset_mask_nhwc=om64)) == L.NOT_SUPPORTED
    empty = nhwc(_cl(torch.zeros(0, 64, H, W)), off[:0], mask[:0], w, None, 1, 1, 1, 1, 1)
    assert empty.shape == (0, 8, H, W) and empty.dtype == torch.float16
    assert empty.is_contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
