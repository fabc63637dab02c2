"""CPU-only: the pre-launch status contract of bevops_se_gate2_nhwc_s8 and bevops_global_avgpool_nhwc_s8
(csrc/lss_depthnet_s8.hip) in the order include/bevops.h states, the numpy statements of
tests/util_lss_depthnet_s8.py on hand-made values (ties, saturation, NaN), and the wrappers' own refusals."""
import ctypes

import numpy as np
import pytest
import torch

import util_lss_depthnet_s8 as U

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_symbols_resolve_and_are_not_registry_functions(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_se_gate2_nhwc_s8", "bevops_global_avgpool_nhwc_s8"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    for name in ("se_gate2_nhwc_q", "global_avgpool_nhwc_q"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS


def test_se_gate2_s8_status_codes(lib, p):
    p = p[0]

    def call(x=p, xp=16, sx=0.5, g=p + 256, a=p + 512, ap=16, sa=0.25, b=p + 768, bp=16, sb=0.125, n=1, hw=4, c=16):
        return lib.bevops_se_gate2_nhwc_s8(x, xp, sx, g, a, ap, sa, b, bp, sb, n, hw, c, None)

    assert call(x=None) == BAD_PARAM and call(g=None) == BAD_PARAM and call(a=None) == BAD_PARAM and call(b=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(hw=0) == BAD_PARAM and call(c=0) == BAD_PARAM
    assert call(xp=0) == BAD_PARAM and call(ap=8) == BAD_PARAM and call(bp=24) == BAD_PARAM and call(xp=40, c=32) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(g=p + 260) == BAD_PARAM and call(a=p + 514) == BAD_PARAM
    assert call(b=p + 776) == BAD_PARAM
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(sx=bad) == BAD_PARAM and call(sa=bad) == BAD_PARAM and call(sb=bad) == BAD_PARAM
        assert call(sb=bad, n=0) == BAD_PARAM
    assert call(c=24, xp=32, ap=32, bp=32) == NOT_SUPPORTED and call(c=8) == NOT_SUPPORTED
    assert call(c=24, xp=32, ap=32, bp=32, n=0) == NOT_SUPPORTED
    assert call(c=24, xp=32, ap=32, bp=32, sx=0.0) == BAD_PARAM               # BAD_PARAM in front of the domain checks
    assert call(n=0) == SUCCESS and call(n=0, xp=80, ap=32, bp=16) == SUCCESS and call(n=0, c=256, xp=256, ap=256, bp=512) == SUCCESS


def test_global_avgpool_s8_status_codes(lib, p):
    p = p[0]

    def call(x=p, xp=16, sx=0.5, o=p + 512, op=16, n=1, hw=4, c=16):
        return lib.bevops_global_avgpool_nhwc_s8(x, xp, sx, o, op, n, hw, c, None)

    assert call(x=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(hw=0) == BAD_PARAM and call(c=0) == BAD_PARAM
    assert call(xp=8) == BAD_PARAM and call(xp=24) == BAD_PARAM and call(op=8) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(o=p + 513) == BAD_PARAM
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(sx=bad) == BAD_PARAM and call(sx=bad, n=0) == BAD_PARAM
    assert call(c=24, xp=32, op=24) == NOT_SUPPORTED and call(c=24, xp=32, op=24, n=0) == NOT_SUPPORTED
    # hw > 2^24: the int32 sum could overflow
    assert call(hw=(1 << 24) + 1, n=0) == NOT_SUPPORTED and call(hw=(1 << 24) + 1) == NOT_SUPPORTED
    assert call(hw=1 << 24, n=0) == SUCCESS and 127 * (1 << 24) < 2 ** 31
    assert call(n=0) == SUCCESS and call(n=0, op=17, o=p + 514) == SUCCESS


def test_gate_statement_on_hand_made_values():
    x, sx, g, sa, sb, want_a, want_b = U.handmade_gate_case()
    assert np.array_equal(U.gate_statement(x, sx, g[0], sa), want_a)
    assert np.array_equal(U.gate_statement(x, sx, g[1], sb), want_b)
    assert (want_a == 127).any() and (want_a == -127).any() and (want_b == -127).any() and (want_b == 127).any()
    # every step is its own fp32 rounding: a float64 evaluation of a general case differs from the statement somewhere
    r = np.random.default_rng(5)
    xq = r.integers(-127, 128, (2, 300, 16)).astype(np.int8)
    gg = r.uniform(0.05, 1.0, (2, 16)).astype(np.float32)
    s_x, s_o = np.float32(0.0371), np.float32(0.0123)
    got = U.gate_statement(xq, s_x, gg, s_o)
    loose = np.clip(np.rint(xq.astype(np.float64) * float(s_x) * gg.astype(np.float64)[:, None, :] / float(s_o)), -127, 127)
    assert np.abs(got - loose).max() <= 1 and (got == 127).any() and (got == -127).any()


def test_pool_statement_on_hand_made_values():
    x, sx, want = U.handmade_pool_case()
    got = U.pool_statement(x, sx)
    assert got.dtype == np.float16 and np.array_equal(got.view(np.int16), want.view(np.int16))
    assert np.isposinf(U.pool_statement(x, 1024.0)[0, 4]) and np.isneginf(U.pool_statement(x, 1024.0)[0, 5])   # binary16 overflow
    # the integer sum does not depend on the order of the pixels
    perm = np.random.default_rng(0).permutation(32)
    assert np.array_equal(U.pool_statement(x[:, perm], sx).view(np.int16), want.view(np.int16))
    # (float)sum is a rounding to nearest even above 2^24, in numpy as on the device
    assert np.int64(2 ** 24 + 1).astype(np.float32) == np.float32(2 ** 24)
    assert np.int64(2 ** 24 + 3).astype(np.float32) == np.float32(2 ** 24 + 4)


def test_wrappers_refuse_what_is_outside_their_domain_without_a_device():
    import bevformer_tensorrt_amd as bev
    with pytest.raises(ValueError):
        bev.se_gate2_nhwc_q(torch.zeros((1, 16, 2, 2), dtype=torch.int8), 0.5, torch.zeros((2, 1, 16)), 0.5, 0.5)
    with pytest.raises(ValueError):
        bev.global_avgpool_nhwc_q(torch.zeros((1, 16, 2, 2), dtype=torch.int8), 0.5)
