"""bevops_deconv4x4s2_f16 (csrc/deconv.hip) through the C ABI in the guarded arena of tests/util_arena.py: every output
bit against a float64 prediction on operands that leave the kernel no rounding but the final one (the F16 lattice of
tests/util_exact_dense.py: integers in [-8, 8] * 2^-4, bias integers * 2^-6; a sum has at most 4 * 512 products of at most
64 units of 2^-8 = 2^17 units, far below 2^24, so every fp32 partial sum is exact in any order), which tap lands where,
what a non-finite input reaches, Gaussian operands at the three layer shapes of the CenterNet neck within the bound of
fp32 accumulation + one fp16 rounding, and the Python wrapper."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 12 << 20


def _ref64(x, w, bias):
    """float64 conv_transpose2d of x [B, H, W, Cin] with w [Cin, Cout, 4, 4] (stride 2, padding 1) -> [B, 2H, 2W, Cout]."""
    y = F.conv_transpose2d(torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2),
                           torch.from_numpy(np.asarray(w, dtype=np.float64)), None, stride=2, padding=1)
    y = y.permute(0, 2, 3, 1).numpy()
    return y if bias is None else y + np.asarray(bias, dtype=np.float64)


def c_call(arena, x, w, bias, relu, packed=None):
    """One call of the entry with every operand carved from `arena` at 16 bytes; the weight through the C pack.
    -> (out [B, 2H, 2W, Cout] device tensor, packed weight device tensor)."""
    from bevformer_tensorrt_amd.utils import lib as L
    h = L.load_library()
    st = L.current_stream_ptr(torch.device("cuda"))
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    xd = arena.place(torch.from_numpy(np.array(x)), 16, "x")
    if packed is None:
        wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
        nbytes = h.bevops_deconv4x4s2_packed_weight_size(L.F16, Cin, Cout)
        assert nbytes == 16 * Cin * Cout * 2
        packed = arena.empty((4, Cout, 2, 2, Cin), torch.float16, 16, "packed")
        assert h.bevops_deconv4x4s2_pack_weight(L.F16, wd.data_ptr(), packed.data_ptr(), Cin, Cout, st) == L.SUCCESS
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias)), 2, "bias")
    out = arena.empty((B, 2 * H, 2 * W, Cout), torch.float16, 16, "out")
    rc = h.bevops_deconv4x4s2_f16(L.F16, xd.data_ptr(), packed.data_ptr(), None if bd is None else bd.data_ptr(),
                                  out.data_ptr(), B, H, W, Cin, Cout, 4, 2, 1, int(relu), st)
    assert rc == L.SUCCESS
    arena.check()
    return out, packed


def run_both_poisons(x, w, bias, relu):
    """The call under both poisons with intact guards; the two results must be equal bit for bit (a kernel that read
    bytes it was not given would differ, or turn 0xFF into NaN).  -> int16 bit patterns [B, 2H, 2W, Cout]."""
    got = []
    for poison in POISONS:
        out, _ = c_call(Arena(CAPACITY, poison), x, w, bias, relu)
        got.append(out.cpu().numpy().view(np.int16))
    assert np.array_equal(got[0], got[1]), "results differ between the two poisons"
    return got[0]


# ---------------------------------------------------------------------------------------------- tolerance 0
CASES = ((1, 1, 1, 32, 8), (1, 3, 5, 64, 64), (2, 7, 9, 128, 128), (1, 12, 11, 256, 256), (1, 5, 4, 64, 136),
         (3, 2, 2, 512, 72))


@functools.lru_cache(maxsize=None)
def lattice_case(case):
    B, H, W, Cin, Cout = case
    r = X._rng("deconv", case)
    x, w = X.gen_f16_small(r, (B, H, W, Cin)), X.gen_f16_small(r, (Cin, Cout, 4, 4))
    bias = X.gen_bias(r, Cout, X.F16)
    worst = _ref64(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), None).max()
    assert worst * 2.0 ** 8 < 2.0 ** 24
    acc = X.f32_exact(_ref64(x, w, None), "sums")
    for a in (x, w, bias, acc):
        a.setflags(write=False)
    return x, w, bias, acc


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(case, with_bias, relu):
    x, w, bias, acc = lattice_case(case)
    v = X.f32_exact(acc + bias.astype(np.float64), "+ bias") if with_bias else acc
    want = (np.maximum(v, 0.0) if relu else v).astype(np.float32).astype(np.float16)     # the ONE rounding
    got = run_both_poisons(x, w, bias if with_bias else None, relu)
    bad = np.argwhere(got != want.view(np.int16))
    assert len(bad) == 0, (f"{len(bad)} of {want.size} outputs differ, first at {tuple(bad[0])}: got "
                           f"{got.view(np.float16)[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
    assert want.any() and (not relu or (want == 0).any())


# ---------------------------------------------------------------------------------------------- which tap lands where
@pytest.mark.parametrize("y0,x0", [(0, 0), (4, 5), (0, 3), (2, 0), (2, 3)],
                         ids=["corner", "far-corner", "edge-top", "edge-left", "interior"])
def test_one_hot_names_its_tap(y0, x0):
    """x = 1 at one pixel and channel, w[ci, co, ky, kx] = 2^(4 ky + kx - 8): output pixel (oy, ox) must hold the weight
    of tap (ky, kx) = (oy - 2 y0 + 1, ox - 2 x0 + 1) when that is a tap, and zero otherwise."""
    B, H, W, Cin, Cout, c0 = 2, 5, 6, 32, 8, 5
    x = np.zeros((B, H, W, Cin), np.float16)
    x[1, y0, x0, c0] = 1.0
    taps = 2.0 ** (4.0 * np.arange(4)[:, None] + np.arange(4)[None, :] - 8.0)
    w = np.broadcast_to(taps, (Cin, Cout, 4, 4)).astype(np.float16)
    want = np.zeros((B, 2 * H, 2 * W, Cout), np.float16)
    for oy in range(2 * H):
        for ox in range(2 * W):
            ky, kx = oy - 2 * y0 + 1, ox - 2 * x0 + 1
            if 0 <= ky < 4 and 0 <= kx < 4:
                want[1, oy, ox, :] = taps[ky, kx]
    got = run_both_poisons(x, w, None, False).view(np.float16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert np.array_equal(want, _ref64(x, w, None).astype(np.float16))      # (the statement above is conv_transpose2d)


# ---------------------------------------------------------------------------------------------- non-finite containment
def test_an_infinite_input_reaches_its_sixteen_output_pixels_only():
    case = (2, 7, 9, 128, 128)
    B, H, W, Cin, Cout = case
    x, w, bias, _ = lattice_case(case)
    clean = run_both_poisons(x, w, bias, False)
    b0, y0, x0 = 1, 3, 4
    xi = x.copy()
    xi[b0, y0, x0, 17] = np.inf
    got = run_both_poisons(xi, w, bias, False)
    reached = np.zeros((B, 2 * H, 2 * W), bool)
    reached[b0, 2 * y0 - 1:2 * y0 + 3, 2 * x0 - 1:2 * x0 + 3] = True
    assert reached.sum() == 16
    finite = np.isfinite(got.view(np.float16))
    assert not finite[reached].any(), "an output whose window holds the infinite input is finite"
    assert finite[~reached].all()
    assert np.array_equal(got[~reached], clean[~reached])


# ---------------------------------------------------------------------------------------------- Gaussian operands
@pytest.mark.parametrize("C", [256, 128, 64])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_gaussian_operands_within_the_fp32_accumulation_bound(C, relu):
    """The three layers of CTResNetNeck (C -> C), spatially small: 16 x 13 = 208 input pixels = two row tiles.
    |got - exact| <= (K + 1) 2^-24 (sum |x w| + |bias|) + 2^-11 |exact| + 2^-25: fp32 accumulation of exact fp16
    products in any order (each of the K additions rounds at most 2^-24 relative to a partial sum bounded by sum |x w|
    + |bias|) plus one fp16 rounding (half an ulp: 2^-11 relative; 2^-25 for the subnormal range)."""
    r = X._rng("deconv gaussian", C)
    B, H, W = 1, 16, 13
    x = r.standard_normal((B, H, W, C)).astype(np.float16)
    w = (r.standard_normal((C, C, 4, 4)) / np.sqrt(4 * C)).astype(np.float16)
    bias = (0.5 * r.standard_normal(C)).astype(np.float16)
    exact = _ref64(x, w, bias)
    mag = _ref64(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64)), None) + np.abs(bias.astype(np.float64))
    if relu:
        exact = np.maximum(exact, 0.0)
    K = 4 * C
    bound = (K + 1) * 2.0 ** -24 * mag + 2.0 ** -11 * np.abs(exact) + 2.0 ** -25
    got = run_both_poisons(x, w, bias, relu).view(np.float16).astype(np.float64)
    err = np.abs(got - exact)
    print(f"C = {C} relu = {relu}: max |err| {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), f"{int((err > bound).sum())} outputs beyond the bound, worst ratio {np.max(err / bound):.3f}"


# ---------------------------------------------------------------------------------------------- the Python side
def test_c_pack_equals_python_pack_and_wrapper_equals_c_call():
    import bevformer_tensorrt_amd as bev
    case = (1, 5, 4, 64, 136)
    B, H, W, Cin, Cout = case
    x, w, bias, _ = lattice_case(case)
    out, packed = c_call(Arena(CAPACITY, 0x55), x, w, bias, True)
    wd, xd = torch.from_numpy(w.copy()).cuda(), torch.from_numpy(x.copy()).cuda().permute(0, 3, 1, 2)
    assert torch.equal(bev.pack_deconv4x4s2(wd), packed)
    assert xd.is_contiguous(memory_format=torch.channels_last)
    y1 = bev.conv_transpose2d_nhwc(xd, wd, torch.from_numpy(bias.copy()).cuda(), relu=True)
    y2 = bev.conv_transpose2d_nhwc(xd, wd, torch.from_numpy(bias.copy()).cuda(), relu=True)
    assert y1.shape == (B, Cout, 2 * H, 2 * W) and y1.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y1.permute(0, 2, 3, 1), out) and torch.equal(y1, y2)
    assert bev.conv_transpose2d_nhwc(xd[:0], wd).shape == (0, Cout, 2 * H, 2 * W)


def test_wrapper_repacks_a_changed_weight_and_never_under_capture():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import deconv as D
    r = X._rng("deconv repack")
    x = torch.from_numpy(X.gen_f16_small(r, (1, 3, 3, 32))).cuda().permute(0, 3, 1, 2)
    w = torch.from_numpy(X.gen_f16_small(r, (32, 8, 4, 4))).cuda()
    y0 = bev.conv_transpose2d_nhwc(x, w)
    p0 = D.deconv_packed_weight(w, build=False)
    assert p0 is not None and D.deconv_packed_weight(w) is p0
    w.mul_(2.0)
    assert D.deconv_packed_weight(w, build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="capturing"):
            bev.conv_transpose2d_nhwc(x, w)                          # raises before it packs or launches anything
    del graph
    assert D.deconv_packed_weight(w, build=False) is None
    assert torch.equal(bev.conv_transpose2d_nhwc(x, w), 2.0 * y0)
    assert D.deconv_packed_weight(w, build=False) is not p0
