"""CPU-only: the pre-launch status contract of bevops_lss_depth_split_s8 and bevops_upsample_bilinear_s8
(csrc/lss_split_s8.hip), the argument checks of their Python wrappers, the float64 statements' own properties, and the
near-tie condition of the GPU tests' general-scale cases, computed from the statement alone."""
import ctypes

import numpy as np
import pytest
import torch

import util_lss_split_s8 as U

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 16384)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_symbols_resolve_and_are_exported(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_lss_depth_split_s8", "bevops_upsample_bilinear_s8"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    for name in ("lss_depth_split_q", "upsample_bilinear_nhwc_q"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS


def test_depth_split_s8_status_codes_without_gpu(lib, p):
    p = p[0]
    inf, nan = float("inf"), float("nan")

    def call(x=p, d=p + 4096, f=p + 8192, n=2, hw=15, stride=32, doff=16, D=5, foff=0, C=16, sd=1 / 127, sf=0.03):
        return lib.bevops_lss_depth_split_s8(x, d, f, n, hw, stride, doff, D, foff, C, sd, sf, None)

    assert call(D=0) == NOT_SUPPORTED and call(D=257, stride=512, doff=0, foff=264) == NOT_SUPPORTED
    assert call(x=None) == BAD_PARAM and call(d=None) == BAD_PARAM and call(f=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(hw=-1) == BAD_PARAM
    assert call(C=8) == BAD_PARAM and call(C=24, stride=48, doff=24) == BAD_PARAM and call(C=0) == BAD_PARAM   # C % 16
    assert call(foff=4) == BAD_PARAM and call(foff=-8) == BAD_PARAM and call(doff=-1) == BAD_PARAM
    assert call(stride=28) == BAD_PARAM and call(stride=0) == BAD_PARAM
    assert call(doff=28) == BAD_PARAM and call(foff=24) == BAD_PARAM                  # a range leaves the row
    assert call(doff=12) == BAD_PARAM and call(doff=0, D=1) == BAD_PARAM              # overlapping ranges
    assert call(x=p + 8) == BAD_PARAM and call(f=p + 8200) == BAD_PARAM               # 16-byte alignment
    for bad in (0.0, -1.0, inf, nan):
        assert call(sd=bad) == BAD_PARAM and call(sf=bad) == BAD_PARAM
        assert call(n=0, sd=bad) == BAD_PARAM                                         # checked in front of the early return
    # nothing to do: SUCCESS without a launch (there is no GPU here); depth_q may sit at any address
    assert call(n=0) == SUCCESS and call(hw=0) == SUCCESS and call(n=0, d=p + 4097) == SUCCESS
    assert call(n=0, D=256, stride=272, doff=0, foff=256) == SUCCESS and call(n=0, D=1, doff=16) == SUCCESS
    assert call(n=0, D=59, C=64, stride=128, doff=64) == SUCCESS                      # BEVDet's layout
    assert call(n=0, doff=0, foff=8, stride=24) == SUCCESS                            # features behind the depth columns


def test_upsample_bilinear_s8_status_codes_without_gpu(lib, p):
    p = p[0]
    inf, nan = float("inf"), float("nan")

    def call(b=p, bp=16, sb=0.05, o=p + 8192, op=16, so=0.037, n=1, h=4, w=4, hb=2, wb=2, C=16):
        return lib.bevops_upsample_bilinear_s8(b, bp, sb, o, op, so, n, h, w, hb, wb, C, None)

    assert call(b=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(h=0) == BAD_PARAM and call(w=0) == BAD_PARAM
    assert call(hb=0) == BAD_PARAM and call(wb=-1) == BAD_PARAM and call(C=0) == BAD_PARAM
    assert call(C=8) == BAD_PARAM and call(C=24, bp=32, op=32) == BAD_PARAM                             # C % 16
    assert call(bp=0) == BAD_PARAM and call(op=0) == BAD_PARAM and call(C=32, bp=16, op=32) == BAD_PARAM   # pitch < C
    assert call(bp=24) == BAD_PARAM and call(op=40) == BAD_PARAM                                        # pitch % 16
    assert call(b=p + 8) == BAD_PARAM and call(o=p + 8196) == BAD_PARAM                                 # 16-byte alignment
    for bad in (0.0, -1.0, inf, nan):
        assert call(sb=bad) == BAD_PARAM and call(so=bad) == BAD_PARAM
    # b must not overlap out: the same bytes, a shifted range, slices of one buffer that share channels
    assert call(o=p) == BAD_PARAM and call(o=p + 16) == BAD_PARAM
    assert call(h=2, w=2, bp=64, op=64, C=32, o=p + 16) == BAD_PARAM
    assert call(h=2, w=2, bp=64, op=48, C=16, o=p + 32) == BAD_PARAM           # ranges meet, pitches differ
    # the source position is a 32-bit fraction; pixel counts stay below 2^31
    assert call(h=65536, hb=32768) == NOT_SUPPORTED and call(w=65536, wb=32768) == NOT_SUPPORTED
    assert call(n=4, h=32768, w=32768, hb=1, wb=1) == NOT_SUPPORTED
    # nothing to do: SUCCESS without a launch (there is no GPU here)
    assert call(n=0) == SUCCESS and call(n=0, bp=48, op=640, C=16) == SUCCESS
    assert call(n=0, h=1, w=1, hb=5, wb=5) == SUCCESS and call(n=0, hb=1, wb=1) == SUCCESS


def test_wrapper_argument_checks():
    from bevformer_tensorrt_amd import functions as fn
    x = torch.zeros(30, 32, dtype=torch.float16)
    ok = dict(n=2, D=5, C=16, depth_offset=16, feat_offset=0, scale_depth=1 / 127, scale_feat=0.03)
    split = lambda x=x, **kw: fn.lss_depth_split_q(x, **{**ok, **kw})
    with pytest.raises(TypeError):
        split(x.float())
    with pytest.raises(TypeError):
        split(x.numpy())
    with pytest.raises(TypeError):
        split(scale_depth="1")
    for kw in (dict(n=4), dict(D=0), dict(D=257), dict(C=8), dict(feat_offset=4, depth_offset=24), dict(depth_offset=28),
               dict(depth_offset=12), dict(spatial=(4, 4)), dict(scale_depth=0.0), dict(scale_feat=float("inf")),
               dict(scale_feat=float("nan")), dict(scale_depth=-1.0), dict(scale_depth=1e-60)):
        with pytest.raises(ValueError):
            split(**kw)
    with pytest.raises(ValueError):
        split(x.t())
    with pytest.raises(ValueError):
        split(torch.zeros(30, 28, dtype=torch.float16))
    with pytest.raises(TypeError, match="GPU"):
        split()                                                     # the device check comes last

    b = torch.zeros(1, 2, 2, 32, dtype=torch.int8).permute(0, 3, 1, 2)
    up = lambda b=b, sb=0.05, so=0.037, **kw: fn.upsample_bilinear_nhwc_q(b, sb, so, **kw)
    with pytest.raises(TypeError):
        up(b.half(), size=(4, 4))
    with pytest.raises(TypeError):
        up(None, size=(4, 4))
    with pytest.raises(TypeError):
        up(size=(4, 4), out=torch.zeros(1, 4, 4, 32, dtype=torch.float16).permute(0, 3, 1, 2))
    with pytest.raises(TypeError):
        up(sb=None, size=(4, 4))
    for kw in (dict(), dict(scale_factor=1.5), dict(scale_factor=0), dict(size=(0, 4)), dict(sb=0.0, size=(4, 4)),
               dict(so=float("nan"), size=(4, 4)),
               dict(size=(3, 3), out=torch.zeros(1, 4, 4, 32, dtype=torch.int8).permute(0, 3, 1, 2)),
               dict(out=torch.zeros(1, 4, 4, 16, dtype=torch.int8).permute(0, 3, 1, 2)),
               dict(out=torch.zeros(2, 4, 4, 32, dtype=torch.int8).permute(0, 3, 1, 2)),
               dict(out=torch.zeros(1, 32, 4, 4, dtype=torch.int8))):                # planar out
        with pytest.raises(ValueError):
            up(**kw)
    with pytest.raises(ValueError):
        up(torch.zeros(1, 32, 2, 2, dtype=torch.int8), size=(4, 4))                  # planar b
    with pytest.raises(ValueError):
        up(torch.zeros(1, 2, 2, 24, dtype=torch.int8).permute(0, 3, 1, 2), size=(4, 4))   # C % 16
    with pytest.raises(ValueError):
        up(torch.zeros(1, 2, 2, 48, dtype=torch.int8).permute(0, 3, 1, 2)[:, 8:24], size=(4, 4))   # slice off a 16-byte boundary
    with pytest.raises(TypeError, match="GPU"):
        up(size=(4, 4))
    with pytest.raises(TypeError, match="GPU"):
        up(b[:, 16:], scale_factor=2)                               # a channel slice passes the layout checks


# ------------------------------------------------------------------------------------- the statements' own properties
def test_depth_statement_rows_sum_to_one():
    x = U.gaussian_rows(130, 59, 64, 128, 64, 0, seed=1).numpy()
    p = U.softmax64(x[:, 64:123].astype(np.float64))
    assert np.abs(p.sum(axis=1) - 1.0).max() <= 1e-14 and p.min() >= 0
    x, k = U.exact_rows(65, 59, 64, 128, 64, 0, seed=2)
    p = U.softmax64(x.numpy()[:, 64:123].astype(np.float64))
    assert np.array_equal(np.sort(p, axis=1)[:, -1], 1.0 / k)       # exactly 0 or 1 / k
    assert np.array_equal((p > 0).sum(axis=1), k)


@pytest.mark.parametrize("size", [1, 2, 5, 64])
def test_axis_statement_identity_and_ends(size):
    i0, i1, lam = U.axis_pos(size, size)                            # an equal-size axis is the identity
    assert np.array_equal(i0, np.arange(size)) and not lam.any()
    for dst in (1, 2, 3, 7, 128):
        i0, i1, lam = U.axis_pos(dst, size)
        assert i0[0] == 0 and lam[0] == 0                           # the first output sits on the first input
        if dst > 1:
            assert lam[-1] == 0 and i0[-1] == size - 1              # the last on the last
        assert (i1 <= size - 1).all() and (lam >= 0).all() and (lam < 1).all()
    b = np.arange(size * size * 16, dtype=np.int64).reshape(1, size, size, 16) % 251 - 125
    assert np.array_equal(U.upsample_statement(b, size, size, 1.0), b.astype(np.float64))


# ---------------------------------------------------------------------------- near ties of the general-scale cases
EPS_TIE = 1e-5


@pytest.mark.parametrize("D", [59, 256])
@pytest.mark.parametrize("scale", [1 / 127, 0.0031])
def test_depth_general_cases_have_few_near_ties(D, scale):
    stride = (D + 16 + 7) // 8 * 8
    x = U.gaussian_rows(130, D, 16, stride, 0, stride - 16, seed=D).numpy()
    share = U.near_tie_share(U.depth_statement(x[:, :D], scale), EPS_TIE)
    print(f"depth split D = {D}, scale {scale:.4g}: near-tie share {share:.2e}")
    assert share <= 0.01
    assert U.depth_eps(x[:, :D], D) <= 2e-5                         # the derived eps is of that size


@pytest.mark.parametrize("src,dst", [(16, 64), (64, 128), (5, 7), (7, 5)])
def test_upsample_general_cases_have_few_near_ties(src, dst):
    b = np.random.default_rng(src).integers(0, 128, size=(1, src, src, 16))
    t = U.upsample_statement(b, dst, dst, U.f32_ratio(0.05, 0.037))
    share = U.near_tie_share(t, EPS_TIE)
    print(f"up-sampler {src} -> {dst}: near-tie share {share:.2e}")
    assert share <= 0.01
    assert U.upsample_eps(dst, dst) <= 2e-5


def test_dyadic_ratio_is_not_an_interval_case():
    """Exact ties: with r = 1/2 on a dyadic geometry a large share of the outputs sits on a half -- those belong to the
    exact cases."""
    b = np.random.default_rng(0).integers(-128, 128, size=(1, 2, 2, 16))
    assert U.near_tie_share(U.upsample_statement(b, 3, 3, 0.5), EPS_TIE) > 0.01
