"""tile_gemm_kernel (csrc/tile_gemm.hip) at its tile edges, bit for bit: every output of every case must equal the float64
reference of tests/util_exact_dense.py, whose operands (power-of-two scales, dyadic grids) leave the kernel no rounding
but the final one -- see that module's docstring for the bit budget and test_dense_exact_cpu.py for the proof that the
cases stay inside it, exercise ties / inexact values / saturation, and reach all 22 instantiations.  No tolerance
anywhere: "int32 sums (exact)", "ONE rounding to fp16", q = clamp(rne(...)) and "an output row depends on its own
operands only" are asserted as stated.  Also here: the stand-alone quantise / de-quantise passes and the int8 stem
pooling on the same kind of operands."""
import contextlib

import numpy as np
import pytest
import torch

import util_exact_dense as X

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scale_w(o):
    return o["s_w"] if np.isscalar(o["s_w"]) else _dev(o["s_w"])


def _ptr(t):
    return None if t is None else t.data_ptr()


@contextlib.contextmanager
def _tiled_only():
    """The tiled kernel whatever the shape (linear_int8_chain would hand N % 256 == 0, K % 128 == 0 to tsgemm_s8)."""
    from bevformer_tensorrt_amd.functions import int8_chain as C
    prev = C._TS_S8["enabled"]
    C._TS_S8["enabled"] = False
    try:
        yield C
    finally:
        C._TS_S8["enabled"] = prev


def _out_dtype(c):
    return torch.int8 if c["out"] == "int8" else torch.float16


def _nchw(t, B, H, W):
    """[B * H * W, C] or [B, H, W, C] rows -> the NCHW-shaped channels-last view the wrappers take."""
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def run_dense(c, o, a=None, mode=None):
    """The case through the Python wrappers; `a` / `mode` override the activation (F16Q's integers on the S8 path)."""
    import bevformer_tensorrt_amd as bev
    mode = mode or c["mode"]
    a = _dev(o["a"] if a is None else a)
    w, bias, res = _dev(o["w"]), _dev(o["bias"]), _dev(o["res"])
    if mode == X.F16:
        return bev.tile_gemm(a, w, bias, res, c["relu"])
    if c["res"] == "int8" or c["relu"]:            # bevops_linear_int8_chain (int8 or fp16 activation)
        with _tiled_only() as C:
            return C.linear_int8_chain(a, o["s_a"], w, _scale_w(o), bias, res, o["s_res"], c["relu"], _out_dtype(c),
                                       o["s_out"])
    return bev.linear_int8(a, o["s_a"], w, _scale_w(o), bias, res, c["relu"], _out_dtype(c), o["s_out"])


def run_conv(c, o, a=None, mode=None):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import int8_chain as C
    from bevformer_tensorrt_amd.utils import lib as L
    mode = mode or c["mode"]
    B, H, W, ks, stride = c["B"], c["H"], c["W"], c["ks"], c["stride"]
    ho, wo = X.conv_out_hw(H, W, ks, stride)
    x = _nchw(_dev(o["a"] if a is None else a), B, H, W)
    w, bias = _dev(o["w"]), _dev(o["bias"])
    res = None if o["res"] is None else _nchw(_dev(o["res"]), B, ho, wo)
    if mode == X.F16:
        out = bev.conv_nhwc(x, w.permute(0, 3, 1, 2), bias, c["relu"], res, stride)
    elif mode == X.F16Q:
        out = bev.conv_int8_nhwc(x, o["s_a"], w, _scale_w(o), bias, c["relu"], res, stride)
    elif res is None:
        out = C.conv_int8_chain_nhwc(x, o["s_a"], w, _scale_w(o), bias, c["relu"], stride, _out_dtype(c), o["s_out"])
    else:                                           # the wrapper has no identity argument: the C ABI
        sw = _scale_w(o)
        out = torch.empty((B, c["Cout"], ho, wo), dtype=_out_dtype(c), device="cuda", memory_format=torch.channels_last)
        st = L.load_library().bevops_conv_tile_int8(
            x.data_ptr(), o["s_a"], w.data_ptr(), _ptr(sw) if torch.is_tensor(sw) else None,
            1.0 if torch.is_tensor(sw) else sw, _ptr(bias), res.data_ptr(), L.I8 if c["out"] == "int8" else L.F16,
            out.data_ptr(), o["s_out"], B, H, W, c["Cin"], c["Cout"], ks, stride, int(c["relu"]),
            L.current_stream_ptr(x.device))
        assert st == L.SUCCESS
    assert out.shape == (B, c["Cout"], ho, wo) and out.is_contiguous(memory_format=torch.channels_last)
    return out.permute(0, 2, 3, 1).reshape(c["M"], c["N"])


def _equal(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        m, n = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} outputs differ, first at [{m}, {n}]: got {got[m, n]!r}, "
                             f"want {want[m, n]!r}; rows {sorted(set(bad[:, 0]))[:8]}, columns {sorted(set(bad[:, 1]))[:8]}")


@pytest.mark.parametrize("c", X.gemm_cases(), ids=lambda c: c["id"])
def test_dense_bits(c):
    import bevformer_tensorrt_amd as bev
    o = X.make_ops(c)
    want = X.reference(c, o)
    assert X.case_instance(c) in X.ALL_TILE_INSTANCES
    _equal(run_dense(c, o), want, c["id"])
    if c["mode"] == X.F16Q:
        # the quantiser inside the operand load is the reference quantiser on the tie grid: the S8 path fed the
        # reference's integers gives the same bits, and bevops_quantize_rows gives those integers
        q = X.ref_quantize(o["a"], o["s_a"])
        assert q.max() == 127 and q.min() == -127
        _equal(run_dense(c, o, a=q, mode=X.S8), want, c["id"] + " on the S8 path")
        _equal(bev.quantize_rows(_dev(o["a"]), o["s_a"]), q, "quantize_rows")


@pytest.mark.parametrize("c", X.conv_cases(), ids=lambda c: c["id"])
def test_conv_bits(c):
    o = X.make_ops(c)
    want = X.reference(c, o)
    assert X.case_instance(c) in X.ALL_TILE_INSTANCES
    _equal(run_conv(c, o), want, c["id"])
    if c["mode"] == X.F16Q:
        _equal(run_conv(c, o, a=X.ref_quantize(o["a"], o["s_a"]), mode=X.S8), want, c["id"] + " on the S8 path")


@pytest.mark.parametrize("c", X.saturated_cases(), ids=lambda c: c["id"])
def test_saturated_accumulators(c):
    """|acc| up to 33 032 192 > 2^24: the sums are int32, (float)acc rounds to nearest even, the rest is exact."""
    o = X.make_ops(c)
    _equal(run_dense(c, o), X.reference(c, o), c["id"])


def test_unsupported_k_leaves_the_output_alone():
    """K % 16 != 0 (int8 flavours), K % 8 != 0 (fp16), channel counts a k-step would straddle, and an int8 identity on
    anything but the plain S8 GEMM: NOT_SUPPORTED, and not one byte of the (NaN-filled) output is written."""
    from bevformer_tensorrt_amd.utils import lib as L
    h = L.load_library()
    st = L.current_stream_ptr(torch.device("cuda"))
    M, N = 40, 24
    a8 = torch.ones(M * 64, dtype=torch.int8, device="cuda")
    a16 = torch.ones(M * 64, dtype=torch.float16, device="cuda")
    w8 = torch.ones(N * 9 * 64, dtype=torch.int8, device="cuda")
    w16 = torch.ones(N * 9 * 64, dtype=torch.float16, device="cuda")
    r8 = torch.ones(M * N, dtype=torch.int8, device="cuda")
    out = torch.full((M * N,), float("nan"), dtype=torch.float16, device="cuda")
    ap, hp, wp, vp, op = a8.data_ptr(), a16.data_ptr(), w8.data_ptr(), w16.data_ptr(), out.data_ptr()
    calls = {
        "linear_int8 K=24": h.bevops_linear_int8(ap, 0.5, wp, None, 0.5, None, None, L.F16, op, 1.0, M, N, 24, 0, st),
        "linear_int8 K=8, int8 out": h.bevops_linear_int8(ap, 0.5, wp, None, 0.5, None, None, L.I8, op, 1.0, M, N, 8, 0, st),
        "linear_int8_fused K=40": h.bevops_linear_int8_fused(hp, 0.5, wp, None, 0.5, None, None, L.F16, op, 1.0, M, N, 40,
                                                             0, st),
        "linear_int8_chain K=56": h.bevops_linear_int8_chain(ap, L.I8, 0.5, wp, None, 0.5, None, None, L.F16, 1.0, L.I8,
                                                             op, 1.0, M, N, 56, 0, st),
        "tile_gemm_f16 K=12": h.bevops_tile_gemm_f16(hp, vp, None, None, op, M, N, 12, 0, st),
        "tile_gemm_f16 K=20": h.bevops_tile_gemm_f16(hp, vp, None, None, op, M, N, 20, 0, st),
        "conv_tile_int8 Cin=32": h.bevops_conv_tile_int8(ap, 0.5, wp, None, 0.5, None, None, L.I8, op, 1.0, 1, 5, 8, 32, N,
                                                         3, 1, 0, st),
        "conv_tile_int8_fused Cin=48": h.bevops_conv_tile_int8_fused(hp, 0.5, wp, None, 0.5, None, None, op, 1, 5, 8, 48,
                                                                     N, 1, 1, 0, st),
        "conv_tile_f16 Cin=16": h.bevops_conv_tile_f16(hp, vp, None, None, op, 1, 5, 8, 16, N, 3, 1, 0, st),
        "conv_tile_f16 5 x 5": h.bevops_conv_tile_f16(hp, vp, None, None, op, 1, 5, 8, 32, N, 5, 1, 0, st),
        "fp16 activation, int8 identity": h.bevops_linear_int8_chain(hp, L.F16, 0.5, wp, None, 0.5, None, r8.data_ptr(),
                                                                     L.I8, 0.5, L.F16, op, 1.0, M, N, 64, 0, st),
    }
    torch.cuda.synchronize()
    assert {k: v for k, v in calls.items() if v != L.NOT_SUPPORTED} == {}
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------ the stand-alone quantise / de-quantise passes
@pytest.mark.parametrize("count", [8, 24, 40, 2056, 4104])       # one vector; odd vector counts; 257 and 513 vectors
def test_quantize_and_dequantize_rows_on_the_tie_grid(count):
    import bevformer_tensorrt_amd as bev
    x = X.gen_f16q_acts(X._rng("quantize_rows", count), (count,))
    q = X.ref_quantize(x, X.S_A)
    assert (np.abs(x.astype(np.float64) / X.S_A % 1.0) == 0.5).any()
    _equal(bev.quantize_rows(_dev(x), X.S_A), q, "quantize_rows")
    q8 = X.gen_int8(X._rng("dequantize_rows", count), (count,), 127, plant128=True)
    for s in (2.0 ** -5, 2.0 ** 3, 2.0 ** -26):     # 2^-26: q / 4 fp16 subnormal steps -- the one rounding, with ties
        _equal(bev.dequantize_rows(_dev(q8), s), X.ref_dequantize(q8, s), f"dequantize_rows * {s}")


def test_quantize_rows_rejects_a_single_element():
    """The passes work on 8-element vectors: a count of 1 is NOT_SUPPORTED and writes nothing."""
    from bevformer_tensorrt_amd.utils import lib as L
    h = L.load_library()
    st = L.current_stream_ptr(torch.device("cuda"))
    x = torch.ones(8, dtype=torch.float16, device="cuda")
    q = torch.full((8,), 77, dtype=torch.int8, device="cuda")
    y = torch.full((8,), float("nan"), dtype=torch.float16, device="cuda")
    assert h.bevops_quantize_rows(L.F16, x.data_ptr(), q.data_ptr(), 1, 0.5, st) == L.NOT_SUPPORTED
    assert h.bevops_dequantize_rows(L.F16, q.data_ptr(), y.data_ptr(), 1, 0.5, st) == L.NOT_SUPPORTED
    torch.cuda.synchronize()
    assert bool((q == 77).all()) and bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------------ the int8 stem pooling
@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (7, 9)])
@pytest.mark.parametrize("C", [8, 64])
def test_stem_pool_int8_bits(H, W, C):
    """bevops_bias_relu_maxpool_nhwc_int8 with dyadic input, bias and scale: max and + bias are exact in fp32,
    v / s_out is a shift with half of the values on a rounding tie, |v / s_out| passes 127."""
    from bevformer_tensorrt_amd.functions import int8_chain as Cn
    r = X._rng("stem_pool", H, W, C)
    B, s_out = 2, 2.0 ** -2
    x = (r.integers(-400, 401, size=(B, H, W, C)) * 2.0 ** -3).astype(np.float16)
    bias = (r.integers(-64, 65, size=C) * 2.0 ** -3).astype(np.float16)
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = np.full((B, H + 2, W + 2, C), -np.inf)
    pad[:, 1:-1, 1:-1] = x
    m = np.full((B, ho, wo, C), -np.inf)
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, pad[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2][:, :ho, :wo])
    v = np.maximum(X.f32_exact(m + bias.astype(np.float64), "+ bias"), 0.0)
    t = X.f32_exact(v / s_out, "* 1 / s_out")
    want = np.clip(np.rint(t), -127, 127).astype(np.int8)
    ties, beyond = X.int8_shares(t)
    assert B * ho * wo * C < 64 or (ties > 0 and beyond > 0)
    for b in (bias, None):
        if b is None:
            want = np.clip(np.rint(np.maximum(m, 0.0) / s_out), -127, 127).astype(np.int8)
        got = Cn.bias_relu_maxpool_nhwc_int8(_nchw(_dev(x), B, H, W), _dev(b), s_out)
        assert got.shape == (B, C, ho, wo) and got.is_contiguous(memory_format=torch.channels_last)
        _equal(got.permute(0, 2, 3, 1).reshape(-1, C), want.reshape(-1, C), f"stem pool {H} x {W} x {C}")
