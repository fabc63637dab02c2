"""CPU-only: the int8 weight pack and the four integer GEMMs of bevops_deconv4x4s2_s8 against F.conv_transpose2d in
float64 (exact on integers), the pre-launch status contract of bevops_deconv4x4s2_s8 and bevops_conv_slice_s8_ex, the
properties the GPU tests' statements must have (tests/util_deconv_s8.py, tests/util_conv_slice_s8_ex.py: the near-tie
interval excuses under 1 % of the outputs; the two identity orders differ on at least 10 %), and the Python wrappers'
argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import util_conv_slice_s8_ex as E
import util_deconv_s8 as D
import util_exact_dense as X

F32, F16, I8 = 0, 1, 2
SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


# ------------------------------------------------------------------------------------------------ pack and integer GEMMs
@pytest.mark.parametrize("case", [(1, 1, 1, 64, 16), (2, 3, 5, 64, 24), (1, 7, 4, 128, 72)], ids=str)
def test_int8_pack_and_four_integer_gemms_equal_conv_transpose2d_exactly(case):
    B, H, W, Cin, Cout = case
    r = X._rng("deconv_s8 cpu", case)
    x, w = X.gen_int8(r, (B, H, W, Cin)), X.gen_int8(r, (Cin, Cout, 4, 4))
    packed = D.pack(w)
    assert packed.shape == (4, Cout, 2, 2, Cin) and packed.dtype == np.int8
    assert sorted(packed.reshape(-1).tolist()) == sorted(w.reshape(-1).tolist())
    got = D.four_gemms_int(x, packed)
    want = D.sums(x, w)
    assert got.dtype == np.int64 and np.array_equal(got, want) and want.any()


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_symbols_resolve_and_wrappers_are_exported(lib):
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_deconv4x4s2_s8", "bevops_conv_slice_s8_ex"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    assert "conv_transpose2d_q_nhwc" in fn.__all__ and "quantize_deconv_weight" in fn.__all__


def _host_block():
    buf = (ctypes.c_char * 8192)()
    return buf, (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced


def test_deconv_s8_status_codes_without_gpu(lib):
    buf, p = _host_block()
    inf, nan = float("inf"), float("nan")

    def fwd(x=p, sa=0.5, w=p + 256, ws=p + 512, sw=1.0, b=p + 768, dt=I8, o=p + 1024, so=0.25, B=1, H=4, W=4, Cin=64,
            Cout=16):
        return lib.bevops_deconv4x4s2_s8(x, sa, w, ws, sw, b, dt, o, so, B, H, W, Cin, Cout, 1, None)

    assert fwd(Cin=32) == NOT_SUPPORTED and fwd(Cin=96) == NOT_SUPPORTED
    assert fwd(Cout=8) == NOT_SUPPORTED and fwd(Cout=24) == NOT_SUPPORTED            # int8 out: Cout % 16
    assert fwd(dt=F16, Cout=12) == NOT_SUPPORTED                                     # fp16 out: Cout % 8
    assert fwd(dt=F32) == NOT_SUPPORTED and fwd(dt=3) == NOT_SUPPORTED
    # B H W Cin, or the packed weight, of 0xFFFFFF00 bytes or more
    assert fwd(B=1, H=32768, W=2048, Cin=64) == NOT_SUPPORTED                        # 2^32 bytes
    assert fwd(B=1, H=1, W=1, Cin=16384, Cout=16384) == NOT_SUPPORTED                # 16 Cin Cout = 2^32 bytes
    assert fwd(x=None) == BAD_PARAM and fwd(w=None) == BAD_PARAM and fwd(o=None) == BAD_PARAM
    assert fwd(x=p + 8) == BAD_PARAM and fwd(w=p + 264) == BAD_PARAM and fwd(o=p + 1028) == BAD_PARAM
    assert fwd(b=p + 770) == BAD_PARAM and fwd(ws=p + 513) == BAD_PARAM
    assert fwd(H=0) == BAD_PARAM and fwd(W=-1) == BAD_PARAM and fwd(B=-1) == BAD_PARAM
    assert fwd(Cin=0) == BAD_PARAM and fwd(Cout=0) == BAD_PARAM
    for bad in (0.0, -1.0, inf, nan):
        assert fwd(sa=bad) == BAD_PARAM and fwd(sw=bad) == BAD_PARAM and fwd(so=bad) == BAD_PARAM
        assert fwd(dt=F16, so=bad, B=0) == SUCCESS                                   # scale_out is not in use with fp16 out
    assert fwd(B=0) == SUCCESS and fwd(B=0, b=None, ws=None) == SUCCESS and fwd(B=0, dt=F16, Cout=8) == SUCCESS
    del buf


def test_deconv_f16_entry_still_refuses_int8(lib):
    buf, p = _host_block()
    assert lib.bevops_deconv4x4s2_f16(I8, p, p + 256, p + 512, p + 768, 1, 4, 4, 64, 16, 4, 2, 1, 0, None) == NOT_SUPPORTED
    assert lib.bevops_deconv4x4s2_packed_weight_size(I8, 64, 16) == 0
    del buf


def test_conv_slice_s8_ex_status_codes_without_gpu(lib):
    buf, p = _host_block()
    inf, nan = float("inf"), float("nan")

    def fwd(x=p, xp=64, sa=0.5, w=p + 256, ws=p + 512, sw=1.0, b=p + 768, r=p + 1024, rp=16, sr=0.5, dt=I8, o=p + 1280,
            op=16, so=0.25, B=1, H=4, W=4, Cin=64, Cout=16, k=3, s=1, act=1, first=1):
        return lib.bevops_conv_slice_s8_ex(x, xp, sa, w, ws, sw, b, r, rp, sr, dt, o, op, so, B, H, W, Cin, Cout, k, s, act,
                                           first, None)

    # the identity in front of the activation: of an identity only, and not of SiLU
    assert fwd(act=2) == NOT_SUPPORTED and fwd(r=None) == NOT_SUPPORTED
    assert fwd(B=0) == SUCCESS and fwd(B=0, act=0) == SUCCESS and fwd(B=0, dt=F16, Cout=8, op=8) == SUCCESS
    for first in (0, 1):      # everything else as bevops_conv_slice_s8 answers it
        f = lambda **kw: fwd(first=first, **kw)
        assert f(Cin=48, xp=48) == NOT_SUPPORTED and f(Cout=8, op=16) == NOT_SUPPORTED
        assert f(dt=F16, Cout=12, op=16, rp=16) == NOT_SUPPORTED
        assert f(k=5) == NOT_SUPPORTED and f(s=3) == NOT_SUPPORTED and f(act=3) == NOT_SUPPORTED and f(dt=F32) == NOT_SUPPORTED
        assert f(B=1, H=32768, W=2048, Cin=64) == NOT_SUPPORTED
        assert f(x=None) == BAD_PARAM and f(w=None) == BAD_PARAM and f(o=None) == BAD_PARAM
        assert f(x=p + 8) == BAD_PARAM and f(w=p + 264) == BAD_PARAM and f(o=p + 1284) == BAD_PARAM and f(r=p + 1030) == BAD_PARAM
        assert f(b=p + 770) == BAD_PARAM and f(ws=p + 513) == BAD_PARAM
        assert f(xp=32) == BAD_PARAM and f(op=8) == BAD_PARAM and f(rp=8) == BAD_PARAM and f(xp=72) == BAD_PARAM
        assert f(H=0) == BAD_PARAM and f(B=-1) == BAD_PARAM and f(Cin=0) == BAD_PARAM and f(k=0) == BAD_PARAM
        for bad in (0.0, -1.0, inf, nan):
            assert f(sa=bad) == BAD_PARAM and f(sw=bad) == BAD_PARAM and f(sr=bad) == BAD_PARAM and f(so=bad) == BAD_PARAM
    assert fwd(first=0, B=0, act=2) == SUCCESS and fwd(first=0, B=0, r=None) == SUCCESS
    # bevops_conv_slice_s8 answers as _ex with res_first = 0
    assert lib.bevops_conv_slice_s8(p, 64, 0.5, p + 256, None, 1.0, None, None, 0, 1.0, I8, p + 1280, 16, 0.25, 0, 4, 4, 64,
                                    16, 3, 1, 2, None) == SUCCESS
    del buf


# ------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("case", D.GENERAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_near_tie_interval_excuses_under_one_percent(case, relu):
    scale_out, t, delta, lo, hi, y_lo, y_hi = D.general_statement(case, relu)
    share = float((lo != hi).mean())
    print(f"delta max {delta.max():.2e} steps, {share:.4%} of the outputs within delta of a half-integer")
    assert delta.max() < 0.01 and share < 0.01
    assert (np.abs(t) > 127.5).any() and int(np.abs(hi.astype(int) - lo).max()) <= 1
    lo16, hi16 = y_lo.astype(np.float16), y_hi.astype(np.float16)
    assert float((lo16 != hi16).mean()) < 0.01


@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("act", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("case", E.CASES, ids=lambda c: "x".join(map(str, c)))
def test_the_two_identity_orders_differ_on_a_tenth_of_the_outputs(case, act, out):
    first, behind, _ = E.statements(case, act, out)
    share = E.differing_share(first, behind)
    print(f"{share:.2%} of the outputs differ between the two orders")
    assert share >= 0.10 if act == 1 else share == 0.0      # (without an activation the two orders are one sum)


@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_statements_hold_fp32_numbers_on_both_sides_of_the_clamp(shape):
    for per_channel in (False, True):
        for with_bias in (False, True):
            for relu in (False, True):
                want, s_out, t = D.lattice_statement(shape, "int8", per_channel, with_bias, relu)
                x, w, ws, scale_w, bias, acc = D.lattice_case(shape, "int8", per_channel)
                same = D.exact_output(acc, D.S_A, scale_w, ws, bias if with_bias else None, int(relu), None, 1.0, s_out, "int8")
                assert np.array_equal(same, want)
                if want.size >= 1000:
                    ties, beyond = X.int8_shares(t)
                    assert ties > 0 and beyond > 0 and (want == 127).any() and ((want == -127).any() or relu)
                D.lattice_statement(shape, "fp16", per_channel, with_bias, relu)


# ------------------------------------------------------------------------------------------------ the Python side
def test_wrappers_check_their_arguments_before_any_device_call():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import deconv as DC
    x = torch.zeros(1, 64, 2, 2, dtype=torch.int8).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        DC.conv_transpose2d_q_nhwc(x, 0.1, torch.zeros(64, 16, 4, 4, dtype=torch.int8), None, None, True, 0.1)   # host tensor
    w = torch.randn(8, 6, 4, 4)
    q, s, b = DC.quantize_deconv_weight(w)
    assert q.dtype == torch.int8 and q.shape == w.shape and s.shape == (6,) and b.shape == (6,) and not b.any()
    assert int(q.abs().amax()) == 127 and torch.equal(q.abs().amax(dim=(0, 2, 3)), torch.full((6,), 127, dtype=torch.int8))
    assert float((q.float() * s[None, :, None, None] - w).abs().max()) <= float(s.max()) / 2 * (1 + 1e-6)
    assert "conv_transpose2d_q_nhwc" not in bev.TRT_FUNCTIONS
