"""The two INT8 launches of csrc/lss_split_s8.hip on the GPU: exact bytes where the statement is exact in fp32 (dyadic
inputs, power-of-two scales), the interval rule of tests/util_lss_split_s8.py against the float64 statement elsewhere,
with the eps derived in design/bevdet_int8.md.  Every case runs in a guarded arena under both poisons
(tests/util_arena.py): guards intact, inputs unchanged, equal bytes under both."""
import numpy as np
import pytest
import torch

import util_lss_split_s8 as U
from util_arena import Arena, POISONS

pytestmark = pytest.mark.gpu


def _lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------- depth split
def _run_split(x, case, sd, sf, poison, depth_align):
    """One guarded launch -> (depth_q [n * hw, D] as pixel rows, feat_q [n * hw, C]) as numpy int8."""
    n, hw, D, C, stride, doff, foff = case
    arena = Arena(8 << 20, poison)
    xd = arena.place(x, 16, "x")
    depth = arena.empty((n, D, hw), torch.int8, depth_align, "depth_q")
    feat = arena.empty((n * hw, C), torch.int8, 16, "feat_q")
    st = _lib().bevops_lss_depth_split_s8(xd.data_ptr(), depth.data_ptr(), feat.data_ptr(), n, hw, stride, doff, D, foff,
                                          C, sd, sf, _stream())
    assert st == 0
    arena.check()
    assert torch.equal(xd.view(torch.int16).cpu(), x.view(torch.int16))           # the input, pad columns included
    return depth.permute(0, 2, 1).reshape(n * hw, D).cpu().numpy(), feat.cpu().numpy()


def _split_everywhere(x, case, sd, sf):
    """Both poisons, the planes on a 16-byte boundary and on an odd address (dword and byte stores): equal bytes."""
    runs = [_run_split(x, case, sd, sf, poison, align) for poison in POISONS for align in (16, 1)]
    for d, f in runs[1:]:
        assert np.array_equal(d, runs[0][0]) and np.array_equal(f, runs[0][1])
    return runs[0]


EXACT_SPLIT_CASES = [  # n, hw, D, C, row_stride, depth_offset, feat_offset
    (1, 1, 1, 16, 24, 16, 0),
    (2, 65, 59, 64, 128, 64, 0),            # BEVDet's layout across a tile edge
    (1, 63, 4, 16, 24, 0, 8),
    (1, 64, 256, 16, 272, 0, 256),
    (3, 129, 7, 32, 40, 32, 0),
]
_ids = lambda c: "x".join(map(str, c))


@pytest.mark.parametrize("case", EXACT_SPLIT_CASES, ids=_ids)
def test_depth_split_exact_bytes(case):
    """Probabilities exactly 0 or 1 / k, power-of-two scales: 1 / 128 saturates k = 1 (128 -> 127), 1 / 4 puts k = 8 on
    the tie 0.5 -> 0 (to even); the -60000 logits are zeros.  Features on sixteenths with scale 1 / 8: ties at every odd
    sixteenth, both saturations (|x| up to 20 -> 160)."""
    n, hw, D, C, stride, doff, foff = case
    x, k = U.exact_rows(n * hw, D, C, stride, doff, foff, seed=hw + D)
    xn = x.numpy()
    logits, feats = xn[:, doff:doff + D].astype(np.float64), xn[:, foff:foff + C].astype(np.float64)
    top = logits == logits.max(axis=1, keepdims=True)
    want_f = np.clip(np.rint(feats * 8.0), -127, 127)
    assert (want_f == 127).any() and (want_f == -127).any() and (np.abs(feats * 8.0 % 1.0) == 0.5).any()
    for sd in (1 / 128, 1 / 64, 1 / 4):
        want_d = np.where(top, np.clip(np.rint((1.0 / sd) / k[:, None]), -127, 127), 0.0)
        got_d, got_f = _split_everywhere(x, case, sd, 1 / 8)
        assert np.array_equal(got_d, want_d.astype(np.int8)), (sd, int((got_d != want_d).sum()))
        assert np.array_equal(got_f, want_f.astype(np.int8))
    if D >= 8:
        assert set(np.unique(np.where(top, np.rint(4.0 / k[:, None]), -1))) >= {0.0, 1.0, 2.0, 4.0}    # the tie is there


GENERAL_SPLIT_CASES = [(2, 65, 59, 64, 128, 64, 0), (1, 130, 256, 16, 272, 0, 256), (3, 129, 7, 32, 40, 32, 0)]


@pytest.mark.parametrize("scales", [(1 / 127, 0.03), (0.0031, 0.011)], ids=["127th", "0.0031"])
@pytest.mark.parametrize("case", GENERAL_SPLIT_CASES, ids=_ids)
def test_depth_split_general_scales(case, scales):
    n, hw, D, C, stride, doff, foff = case
    sd, sf = scales
    x = U.gaussian_rows(n * hw, D, C, stride, doff, foff, seed=D + hw)
    xn = x.numpy()
    logits = xn[:, doff:doff + D]
    t = U.depth_statement(logits, sd)
    eps = U.depth_eps(logits, D)
    got_d, got_f = _split_everywhere(x, case, sd, sf)
    ok = U.interval_ok(got_d, t, eps)
    off = int((got_d != U.saturate(t)).sum())
    print(f"depth split {case} scale {sd:.4g}: eps {eps:.3e}, near-tie share {U.near_tie_share(t, eps):.2e}, "
          f"{off} of {t.size} bytes differ from the rounded statement, {int((~ok).sum())} outside the interval")
    assert ok.all()
    # the features: one product in fp32, then rne -- the float64 product rounded to fp32 is that product
    tf = U.feat_statement(xn[:, foff:foff + C], sf).astype(np.float32).astype(np.float64)
    assert np.array_equal(got_f, U.saturate(tf).astype(np.int8))
    # the wrapper returns the same bytes in the shapes the pooling takes
    from bevformer_tensorrt_amd import functions as fn
    d2, f2 = fn.lss_depth_split_q(x.cuda(), n, D, C, doff, foff, sd, sf)
    assert d2.shape == (n, D, hw) and f2.shape == (n, hw, C) and d2.dtype == f2.dtype == torch.int8
    assert np.array_equal(d2.permute(0, 2, 1).reshape(n * hw, D).cpu().numpy(), got_d)
    assert np.array_equal(f2.view(n * hw, C).cpu().numpy(), got_f)


def test_depth_split_transposition_is_exact():
    """A distinct maximum bin per pixel lands in the right plane and column, and nowhere else."""
    case = n, hw, D, C, stride, doff, foff = (2, 65, 59, 64, 128, 64, 0)
    rows = n * hw
    x = torch.zeros(rows, stride, dtype=torch.float16)
    x[:, doff:doff + D] = -60000.0
    bins = (np.arange(rows) * 7 + np.arange(rows) // hw) % D
    x[torch.arange(rows), doff + torch.from_numpy(bins)] = 2.0
    got_d, _ = _split_everywhere(x, case, 1 / 64, 1.0)
    want = np.zeros((rows, D), dtype=np.int8)
    want[np.arange(rows), bins] = 64
    assert np.array_equal(got_d, want)


def test_depth_split_contains_non_finite_values():
    case = n, hw, D, C, stride, doff, foff = (2, 65, 59, 64, 128, 64, 0)
    sd, sf = 1 / 127, 0.03
    clean = U.gaussian_rows(n * hw, D, C, stride, doff, foff, seed=11)
    x = clean.clone()
    inf, nan = float("inf"), float("nan")
    x[3, doff + 5] = nan                     # a NaN logit, a +inf logit, a row of -inf: the pixel's D bytes are -127
    x[64, doff + 58] = inf
    x[70, doff:doff + D] = -inf
    x[100, doff + 7] = -inf                  # one -inf logit is a probability of 0: the pixel stays good
    x[5, foff + 1], x[5, foff + 2], x[6, foff + 63] = nan, inf, -inf
    base_d, base_f = _split_everywhere(clean, case, sd, sf)
    got_d, got_f = _split_everywhere(x, case, sd, sf)
    spoiled = np.zeros(n * hw, dtype=bool)
    spoiled[[3, 64, 70]] = True
    assert (got_d[spoiled] == -127).all()
    keep = ~spoiled
    keep[100] = False
    assert np.array_equal(got_d[keep], base_d[keep])                               # nothing else moved
    assert got_d[100, 7] == 0
    row = x.numpy()[100:101, doff:doff + D]
    assert U.interval_ok(got_d[100], U.depth_statement(row, sd)[0], U.depth_eps(np.delete(row, 7, axis=1), D)).all()
    assert (got_f[5, 1], got_f[5, 2], got_f[6, 63]) == (-127, 127, -127)
    same = np.ones_like(got_f, dtype=bool)
    same[5, 1] = same[5, 2] = same[6, 63] = False
    assert np.array_equal(got_f[same], base_f[same])


def test_depth_split_replays_from_a_graph_to_the_same_bytes():
    from bevformer_tensorrt_amd import functions as fn
    n, hw, D, C, stride, doff, foff = (2, 65, 59, 64, 128, 64, 0)
    x = U.gaussian_rows(n * hw, D, C, stride, doff, foff, seed=3).cuda()
    eager = fn.lss_depth_split_q(x, n, D, C, doff, foff, 0.0031, 0.011)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn.lss_depth_split_q(x, n, D, C, doff, foff, 0.0031, 0.011)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = fn.lss_depth_split_q(x, n, D, C, doff, foff, 0.0031, 0.011)
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])


# ------------------------------------------------------------------------------------------------------ up-sampler
def _run_up(b, size, C, sb, so, poison, pad):
    """One guarded launch of b int8 [n, hb, wb, C] (numpy); with `pad` both slices sit at channel 16 of wider buffers.
    Every byte outside the output slice is compared with the poison.  -> out [n, h, w, C] numpy int8."""
    n, hb, wb, _ = b.shape
    h, w = size
    bp, op, at = (C + 32, C + 48, 16) if pad else (C, C, 0)
    arena = Arena(8 << 20, poison)
    bbuf = arena.empty((n, hb, wb, bp), torch.int8, 16, "b")
    bbuf[..., at:at + C] = torch.from_numpy(b).cuda()
    b0 = bbuf.clone()
    obuf = arena.empty((n, h, w, op), torch.int8, 16, "out")
    st = _lib().bevops_upsample_bilinear_s8(bbuf[..., at:].data_ptr(), bp, sb, obuf[..., at:].data_ptr(), op, so, n, h, w,
                                            hb, wb, C, _stream())
    assert st == 0
    arena.check()
    assert torch.equal(bbuf, b0)
    outside = torch.ones(op, dtype=torch.bool, device="cuda")
    outside[at:at + C] = False
    assert bool((obuf[..., outside].view(torch.uint8) == poison).all())
    return obuf[..., at:at + C].cpu().numpy()


def _up_everywhere(b, size, C, sb, so):
    runs = [_run_up(b, size, C, sb, so, poison, pad) for poison in POISONS for pad in (True, False)]
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    return runs[0]


DYADIC = [((2, 2), (3, 3)), ((3, 2), (5, 3)), ((1, 1), (4, 4)), ((4, 4), (4, 4)), ((5, 5), (1, 1)), ((2, 3), (1, 5))]


@pytest.mark.parametrize("C", [16, 48])
@pytest.mark.parametrize("geom", DYADIC, ids=lambda g: f"{g[0][0]}x{g[0][1]}to{g[1][0]}x{g[1][1]}")
def test_upsample_exact_bytes_on_dyadic_geometry(geom, C):
    """Weights in quarters, so the fp32 arithmetic is exact and the statement's rounding is the only admissible byte.
    r = 2 saturates, r = 1/2 puts the odd values on ties; r is passed as scale_b = r, scale_out = 1."""
    (hb, wb), (h, w) = geom
    b = np.random.default_rng(hb * 10 + w).integers(-128, 128, size=(2, hb, wb, C)).astype(np.int8)
    b[0, 0, 0, :4] = (127, -128, 1, -1)
    seen_tie = seen_sat = False
    for r in (1.0, 2.0, 0.5):
        t = U.upsample_statement(b, h, w, r)
        assert np.array_equal(t * 8, np.rint(t * 8))                                 # on the lattice of eighths: exact
        seen_tie |= bool((np.abs(t % 1.0) == 0.5).any())
        seen_sat |= bool((np.abs(t) > 127).any())
        got = _up_everywhere(b, (h, w), C, r, 1.0)
        assert np.array_equal(got, U.saturate(t).astype(np.int8)), r
        if r == 1.0 and (hb, wb) == (h, w):
            assert np.array_equal(got, np.maximum(b, -127))                          # the input bytes (the clamp aside)
    assert seen_tie and seen_sat


GENERAL_GEOMETRY = [(16, 64), (64, 128), (5, 7), (7, 5)]


@pytest.mark.parametrize("src,dst", GENERAL_GEOMETRY, ids=lambda v: str(v))
def test_upsample_general_geometry(src, dst):
    """The model's two calls and two odd ones with r = 0.05 / 0.037, on non-negative inputs (behind a ReLU, as in the
    model; the relative interval rule needs corners of one sign)."""
    b = np.random.default_rng(src).integers(0, 128, size=(1, src, src, 16)).astype(np.int8)
    t = U.upsample_statement(b, dst, dst, U.f32_ratio(0.05, 0.037))
    eps = U.upsample_eps(dst, dst)
    got = _up_everywhere(b, (dst, dst), 16, 0.05, 0.037)
    ok = U.interval_ok(got, t, eps)
    print(f"up-sampler {src} -> {dst}: eps {eps:.3e}, near-tie share {U.near_tie_share(t, eps):.2e}, "
          f"{int((got != U.saturate(t)).sum())} of {t.size} bytes differ from the rounded statement, "
          f"{int((~ok).sum())} outside the interval")
    assert ok.all()
    # the wrapper: the same bytes, as a new tensor and into a slice of a wider buffer
    from bevformer_tensorrt_amd import functions as fn
    bq = torch.from_numpy(b).cuda().permute(0, 3, 1, 2)
    o1 = fn.upsample_bilinear_nhwc_q(bq, 0.05, 0.037, size=(dst, dst))
    assert o1.shape == (1, 16, dst, dst) and o1.dtype == torch.int8
    assert np.array_equal(o1.permute(0, 2, 3, 1).cpu().numpy(), got)
    wide = torch.full((1, dst, dst, 48), 77, dtype=torch.int8, device="cuda").permute(0, 3, 1, 2)
    o2 = fn.upsample_bilinear_nhwc_q(bq, 0.05, 0.037, out=wide[:, 16:32])
    assert o2.data_ptr() == wide[:, 16:32].data_ptr()
    assert np.array_equal(wide[:, 16:32].permute(0, 2, 3, 1).cpu().numpy(), got)
    assert bool((wide[:, :16] == 77).all()) and bool((wide[:, 32:] == 77).all())


def test_upsample_replays_from_a_graph_to_the_same_bytes():
    from bevformer_tensorrt_amd import functions as fn
    b = torch.from_numpy(np.random.default_rng(9).integers(0, 128, size=(2, 16, 16, 32)).astype(np.int8)).cuda()
    bq = b.permute(0, 3, 1, 2)
    wide = torch.zeros((2, 64, 64, 64), dtype=torch.int8, device="cuda").permute(0, 3, 1, 2)
    eager = fn.upsample_bilinear_nhwc_q(bq, 0.05, 0.037, scale_factor=4).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn.upsample_bilinear_nhwc_q(bq, 0.05, 0.037, out=wide[:, 32:])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn.upsample_bilinear_nhwc_q(bq, 0.05, 0.037, out=wide[:, 32:])
    wide.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 32:], eager) and not wide[:, :32].any()
