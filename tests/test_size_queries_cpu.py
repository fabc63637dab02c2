"""CPU-only: the size queries of include/bevops.h against an independent restatement of the layouts their comments
state (csrc/msda_pad.h: one lead entry, (H + 2)(W + 1) entries per level, one trail entry, 128 bytes per entry of the
set read through the caches and 64 per entry of the LDS-staged set), swept over level sets with one-row, one-column
and one-pixel levels, odd widths and the model pyramids, for batch x heads up to 6 x 8.  No planning code of the
library is called to produce an expectation: the arithmetic below is the test's own."""
import ctypes
import itertools

import pytest

F32, F16, I8 = 0, 1, 2
SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3
HEADS_C = 32

LEVEL_SETS = {
    "one_pixel": [[1, 1]],
    "one_row_9": [[1, 9]],
    "one_row_21": [[1, 21]],
    "one_col": [[9, 1]],
    "three_one_row": [[1, 9], [1, 21], [1, 1], [2, 2]],
    "four_one_row": [[1, 40], [1, 20], [1, 10], [1, 5]],
    "one_rows_cols": [[1, 7], [7, 1], [1, 1], [3, 1]],
    "odd_widths": [[7, 9], [5, 3], [3, 1], [1, 1]],
    "ragged": [[12, 17], [6, 9]],
    "lp16": [[10, 12], [5, 6]],
    "tiny_sca": [[15, 25]],
    "small_sca": [[23, 40]],
    "tiny_tsa": [[50, 50]],
    "base_tsa": [[200, 200]],
    "base_sca": [[116, 200], [58, 100], [29, 50], [15, 25]],
    "other_pyramid": [[92, 160], [46, 80], [23, 40], [12, 20]],
}
BATCH_HEADS = [(1, 1), (2, 8), (3, 4), (6, 8)]
QUERIES = [1, 300, 2047, 2048, 2049, 40000]
POINTS = [4, 8]


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    handle = load_library()
    handle.bevops_msda_set_variant(0)
    return handle


def _host(levels):
    flat = [v for hw in levels for v in hw]
    return (ctypes.c_int32 * len(flat))(*flat)


def _cases():
    for (name, levels), (bs, heads), nq, P in itertools.product(LEVEL_SETS.items(), BATCH_HEADS, QUERIES, POINTS):
        if (len(levels) * P) % 4 == 0:
            yield name, levels, bs, heads, nq, P


# ---- the layout of csrc/msda_pad.h, restated -------------------------------------------------------------------------
ENTRY_BIG, ENTRY_STAGED = 128, 64
LDS_LIMIT, LEVEL_TABLE = 160 * 1024, 8 * 32


def _padded(hw):
    return (hw[0] + 2) * (hw[1] + 1)


def _round_up(v, to):
    return (v + to - 1) // to * to


def _first_staged(levels, nq, lds_other):
    """The longest tail of levels whose padded planes (plus lead and trail entry, 64 bytes each) fit in LDS next to
    `lds_other` bytes; nothing is staged below 2048 queries."""
    first = len(levels)
    if nq >= 2048:
        tail = 2
        for l in range(len(levels) - 1, -1, -1):
            tail += _padded(levels[l])
            if tail * ENTRY_STAGED > LDS_LIMIT - LEVEL_TABLE - lds_other:
                break
            first = l
    return first


def _set_bytes(levels, bs, heads, first):
    """(bytes of the cached set, bytes of the staged set) for all batches and heads."""
    big = 2 + sum(_padded(hw) for hw in levels[:first])
    staged = 2 + sum(_padded(hw) for hw in levels[first:]) if first < len(levels) else 0
    return bs * heads * big * ENTRY_BIG, _round_up(bs * heads * staged * ENTRY_STAGED, 128)


# (L P, batches of four points read through the caches) the sampler is built for (include/bevops.h: "the instantiated
# (levels x points, staged levels) combinations"; csrc/msda_hm4.hip lists them with the model call each serves)
HM4_KERNELS = {(32, 4), (32, 8), (32, 6), (8, 0), (8, 2), (4, 1), (4, 0)}


def _hm4_bytes(levels, bs, heads, nq, P, int8):
    """bevops_msda_packed_size: [cached set, to 128][128 bytes for the last entry's pair partner][staged set].  The
    sampler's 512 threads keep 64 mailboxes of (L P + 1) 16-byte records next to the staged planes; the int8 kernel
    for L P == 32 prefers to stage at most 40 KiB when that leaves exactly six batches of four points cached.  A
    batch of min(L P, 4) points never straddles the two sets, and the sampler exists for the HM4_KERNELS combinations
    only (0: outside the family's domain)."""
    L, LP = len(levels), len(levels) * P
    bt = min(LP, 4)
    if int8 and LP == 32:
        first = _first_staged(levels, nq, LDS_LIMIT - LEVEL_TABLE - 40 * 1024)
        if first < L and (first * P) % bt == 0 and first * P // bt == 6:
            g, s = _set_bytes(levels, bs, heads, first)
            return g + 128 + s
    first = _first_staged(levels, nq, 64 * (LP * 16 + 16))
    if (first * P) % bt or (LP, first * P // bt) not in HM4_KERNELS:
        return 0
    g, s = _set_bytes(levels, bs, heads, first)
    return g + 128 + s


def test_restated_layout_is_the_packed_size(lib):
    """bevops_msda_packed_size (fp16 and int8) equals the layout the header states, and is 0 exactly where
    bevops_msda_pack_value and bevops_msda_forward_prepacked answer NOT_SUPPORTED (host-side rejections: those calls
    return before any launch; where the size is non-zero the pair's status 0 is the GPU suite's to show, a call here
    would launch)."""
    buf = (ctypes.c_char * 512)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 128
    one = ctypes.c_float(1.0)
    zero_sized = 0
    for name, levels, bs, heads, nq, P in _cases():
        nk = sum(h * w for h, w in levels)
        sh = _host(levels)
        for dt in (F16, I8):
            want = _hm4_bytes(levels, bs, heads, nq, P, dt == I8)
            got = lib.bevops_msda_packed_size(dt, ctypes.addressof(sh), bs, nk, heads, HEADS_C, len(levels), nq, P)
            assert got == want, (name, dt, bs, heads, nq, P, got, want)
            if got == 0:        # ... and there, and only there, the pair turns the call away on the host (no launch)
                zero_sized += 1
                rdt = F16 if dt == F16 else F32
                assert lib.bevops_msda_pack_value(dt, rdt, p, ctypes.addressof(sh), p, 1 << 40, bs, nk, heads, HEADS_C,
                                                  len(levels), nq, P, None) == NOT_SUPPORTED, (name, dt, bs, heads, nq, P)
                assert lib.bevops_msda_forward_prepacked(dt, p, 1 << 40, ctypes.addressof(sh), p, rdt, p, p, p, bs, nk, heads,
                                                         HEADS_C, len(levels), nq, P, 4 if P % 4 == 0 else 1, one, one, one,
                                                         one, 0, None) == NOT_SUPPORTED, (name, dt, bs, heads, nq, P)
        # 0 outside the domain, like the pack entry's NOT_SUPPORTED (host-side rejection: 48 channels per head)
        assert lib.bevops_msda_packed_size(F16, ctypes.addressof(sh), bs, nk, heads, 48, len(levels), nq, P) == 0
    assert zero_sized > 100      # L P = 16, L P = 32 with every level staged, ...: the sweep does visit the boundary


def test_int8_coarse_query_bounds_the_exact_one(lib):
    """bevops_msda_workspace_size(BEVOPS_I8) is documented as an upper bound of the exact, shape-aware size: a caller
    that lends it must never be turned away from the head-major kernel.  (H + 2)(W + 1) <= 3 H W + 3, with equality
    on one-row levels: three entries of slack per level, not two."""
    lib.bevops_msda_set_variant(17)   # the int8 head-major family wherever it applies, whatever the call's size
    try:
        seen = 0
        for name, levels, bs, heads, nq, P in _cases():
            nk = sum(h * w for h, w in levels)
            L = len(levels)
            sh = _host(levels)
            coarse = lib.bevops_msda_workspace_size(I8, bs, nk, heads, HEADS_C, L, nq, P)
            exact = lib.bevops_msda_workspace_size_shapes(I8, ctypes.addressof(sh), bs, nk, heads, HEADS_C, L, nq, P)
            assert coarse > 0, (name, bs, heads, nq, P)
            assert exact == _hm4_bytes(levels, bs, heads, nq, P, True), (name, bs, heads, nq, P)
            assert coarse >= exact, (name, bs, heads, nq, P, coarse, exact)
            # and the bound is what its comment states: 3 nk + 3 L + 4 entries of 128 bytes per plane, plus 4096
            assert coarse == bs * heads * (3 * nk + 3 * L + 4) * 128 + 4096
            seen += 1
        assert seen > 500
    finally:
        lib.bevops_msda_set_variant(0)


def test_shapes_query_covers_the_coarse_one_fp16(lib):
    """fp16: the shape-aware query is the largest need of every family that may serve the call, so it is at least the
    coarse one and at least the padded planes (hm3 / hm4) the header names.  (For int8 the shape-aware query is the
    exact size and the coarse one its upper bound: the order is the other way round, see the test above.)"""
    for variant in (0, 11, 15, 16, 17, 1000):
        lib.bevops_msda_set_variant(variant)
        try:
            for name, levels, bs, heads, nq, P in _cases():
                nk = sum(h * w for h, w in levels)
                L = len(levels)
                sh = _host(levels)
                coarse = lib.bevops_msda_workspace_size(F16, bs, nk, heads, HEADS_C, L, nq, P)
                shaped = lib.bevops_msda_workspace_size_shapes(F16, ctypes.addressof(sh), bs, nk, heads, HEADS_C, L, nq, P)
                assert shaped >= coarse, (variant, name, bs, heads, nq, P, shaped, coarse)
                if coarse:
                    assert shaped >= _hm4_bytes(levels, bs, heads, nq, P, False), (variant, name, bs, heads, nq, P)
                # without the shapes the query is the coarse one
                assert lib.bevops_msda_workspace_size_shapes(F16, None, bs, nk, heads, HEADS_C, L, nq, P) == coarse
        finally:
            lib.bevops_msda_set_variant(0)


def test_sca_workspace_embeds_planes_and_sampled_rows(lib):
    """bevops_sca_workspace_size = the padded planes of the sampler (lead, levels, trail: 128-byte entries, 64-byte for
    the staged tail; 1024 threads keep 128 mailboxes of min(L P, 8) + 1 16-byte records) to 256 bytes, then the sampled
    rows [cams, nq, heads, 32] fp16 the camera reduce reads."""
    for name, levels, bs, heads, nq, P in _cases():
        nk = sum(h * w for h, w in levels)
        L, LP = len(levels), len(levels) * P
        sh = _host(levels)
        first = _first_staged(levels, nq, 128 * (min(LP, 8) * 16 + 16))
        g, s = _set_bytes(levels, bs, heads, first)
        planes = g + 128 + s
        want = _round_up(planes, 256) + bs * nq * heads * HEADS_C * 2
        got = lib.bevops_sca_workspace_size(F16, ctypes.addressof(sh), bs, nk, heads, HEADS_C, L, nq, P)
        assert got == want, (name, bs, heads, nq, P, got, want)
        assert got >= planes + bs * nq * heads * HEADS_C * 2
        assert lib.bevops_sca_workspace_size(F32, ctypes.addressof(sh), bs, nk, heads, HEADS_C, L, nq, P) == 0
        assert lib.bevops_sca_workspace_size(F16, ctypes.addressof(sh), bs, nk, heads, 48, L, nq, P) == 0
        assert lib.bevops_sca_prepacked_workspace_size(bs, heads, HEADS_C, nq) == bs * nq * heads * HEADS_C * 2


def test_plan_and_small_packed_sizes_match_their_comments(lib):
    for cams, nq in itertools.product((1, 2, 6, 16), (1, 63, 64, 65, 100, 2049, 40000, 65535)):
        # 64 bytes of counts, per camera the list padded to 64 entries of 4 bytes, 1 KiB of builder scratch
        assert lib.bevops_sca_plan_size(cams, nq) == 64 + cams * _round_up(nq, 64) * 4 + cams * 1024
    for cams, nq in ((0, 5), (17, 100), (6, 65536), (6, 0), (-1, 5)):
        assert lib.bevops_sca_plan_size(cams, nq) == 0
    assert lib.bevops_stem_packed_size() == 11 * 2 * 64 * 8 * 2
    assert lib.bevops_linear_workspace_size() > 0


def test_zero_size_where_the_entry_rejects_on_the_host(lib):
    """A query returns 0 for arguments its entry turns away before any device call."""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 128
    sh = _host([[3, 3]])
    f = ctypes.c_float
    # fused SCA: fp32 -> NOT_SUPPORTED and size 0; 48 channels -> size 0 and NOT_SUPPORTED from the sampler's domain check
    assert lib.bevops_sca_workspace_size(F32, ctypes.addressof(sh), 2, 9, 8, 32, 1, 10, 4) == 0
    assert lib.bevops_sca_forward(F32, p, ctypes.addressof(sh), p, p, p, p, p, 2, 9, 8, 32, 1, 10, 4, 1, p, 4096, None) == NOT_SUPPORTED
    assert lib.bevops_sca_workspace_size(F16, ctypes.addressof(sh), 2, 9, 8, 48, 1, 10, 4) == 0
    assert lib.bevops_sca_forward(F16, p, ctypes.addressof(sh), p, p, p, p, p, 2, 9, 8, 48, 1, 10, 4, 1, p, 4096, None) == NOT_SUPPORTED
    # ... and a workspace below the documented 128-byte alignment, or none, is a bad parameter (no kernel to fall back to)
    assert lib.bevops_sca_forward(F16, p, ctypes.addressof(sh), p, p, p, p, p, 2, 9, 8, 32, 1, 10, 4, 1, p + 16, 1 << 30, None) == BAD_PARAM
    assert lib.bevops_sca_forward(F16, p, ctypes.addressof(sh), p, p, p, p, p, 2, 9, 8, 32, 1, 10, 4, 1, p + 64, 1 << 30, None) == BAD_PARAM
    assert lib.bevops_sca_forward(F16, p, ctypes.addressof(sh), p, p, p, p, p, 2, 9, 8, 32, 1, 10, 4, 1, None, 0, None) == BAD_PARAM
    # packed MSDA value: 48 channels per head
    assert lib.bevops_msda_packed_size(F16, ctypes.addressof(sh), 2, 9, 8, 48, 1, 10, 4) == 0
    assert lib.bevops_msda_pack_value(F16, F16, p, ctypes.addressof(sh), p, 4096, 2, 9, 8, 48, 1, 10, 4, None) == NOT_SUPPORTED
    # a packed buffer below the documented 128-byte alignment is outside the domain, not a launch
    assert lib.bevops_msda_pack_value(F16, F16, p, ctypes.addressof(sh), p + 16, 4096, 2, 9, 8, 32, 1, 10, 4, None) == NOT_SUPPORTED
    # visibility plan: too many cameras / queries
    assert lib.bevops_sca_plan_size(17, 100) == 0
    assert lib.bevops_sca_plan_build(F16, p, 17, 100, p, 4096, None) == NOT_SUPPORTED
    assert lib.bevops_sca_plan_size(6, 65536) == 0
    assert lib.bevops_sca_plan_build(F16, p, 6, 65536, p, 4096, None) == NOT_SUPPORTED
    # and a plan that is not 16-byte aligned or too short is a bad parameter
    assert lib.bevops_sca_plan_build(F16, p, 2, 10, p + 8, 4096, None) == BAD_PARAM
    assert lib.bevops_sca_plan_build(F16, p, 2, 10, p, lib.bevops_sca_plan_size(2, 10) - 1, None) == BAD_PARAM
    # MSDA workspace: (L P) % 4 != 0 has no head-major kernel; dims <= 0
    assert lib.bevops_msda_workspace_size(F16, 2, 9, 8, 32, 1, 10, 3) == 0
    assert lib.bevops_msda_workspace_size(F16, 0, 9, 8, 32, 1, 10, 4) == 0
    assert lib.bevops_msda_workspace_size(F32, 2, 9, 8, 32, 1, 10, 4) == 0
    assert lib.bevops_msda_forward_ws(F16, p, p, ctypes.addressof(sh), p, F16, p, p, p, 0, 9, 8, 32, 1, 10, 4, 1,
                                      f(1), f(1), f(1), f(1), 0, p, 4096, None) == BAD_PARAM
    # shapes that do not cover nk
    assert lib.bevops_msda_forward_ws(F16, p, p, ctypes.addressof(sh), p, F16, p, p, p, 2, 10, 8, 32, 1, 10, 4, 1,
                                      f(1), f(1), f(1), f(1), 0, p, 4096, None) == BAD_PARAM


def test_other_queries_are_zero_where_their_entries_answer_not_supported(lib):
    """The queries whose 0 the header defines as "unsupported": bevops_conv3x3_c32_packed_weight_size,
    bevops_lss_voxel_prepare_workspace_size and bevops_value_proj_packed_size, against the host-side rejections of
    their entries (every call below returns before a launch).  The other queries' 0 means something else -- "no
    scratch needed" (qkv, centerpoint_decode, grid_sampler_2d: the planar kernel runs) or bad dimensions, which the
    entry reports as BAD_PARAM (mdconv, bev_nms) -- and is no statement about NOT_SUPPORTED (design/buffers.md)."""
    buf = (ctypes.c_char * 512)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 128
    for cin in (32, 64, 96, 128, 192, 256, 320, 512, 768):
        size = lib.bevops_conv3x3_c32_packed_weight_size(F16, cin)
        assert (size > 0) == (cin in (64, 128, 256, 512, 768)) and size in (0, 9 * cin * 32 * 2)
        if size == 0:
            assert lib.bevops_conv3x3_c32_pack_weight(F16, p, p, 27, cin, None) == NOT_SUPPORTED
            assert lib.bevops_conv3x3_c32_forward_nhwc(F16, p, p, None, p, 1, 4, 4, cin, None) == NOT_SUPPORTED
    assert lib.bevops_conv3x3_c32_packed_weight_size(F32, 64) == 0
    assert lib.bevops_conv3x3_c32_pack_weight(F32, p, p, 27, 64, None) == NOT_SUPPORTED
    grid = (ctypes.c_float * 9)(-51.2, -51.2, -5.0, 0.8, 0.8, 8.0, 128.0, 128.0, 1.0)
    for dims in ((1, 1, 4096, 2048), (4096, 2048, 1, 1), (6, 59, 512, 512)):       # more than 2^22 points
        assert lib.bevops_lss_voxel_prepare_workspace_size(*dims) == 0
        assert lib.bevops_lss_voxel_prepare(p, p, ctypes.addressof(grid), p, p, p, p, p, p, None, 1, *dims, p, 1 << 40,
                                            None) == NOT_SUPPORTED
    assert lib.bevops_lss_voxel_prepare_workspace_size(6, 59, 16, 44) > 0
    base = [[116, 200], [58, 100], [29, 50], [15, 25]]
    nk = sum(h * w for h, w in base)
    sh = _host(base)
    one = _host([[15, 25]])
    # (shapes, nk, heads, channels, levels, queries, points): the sampler's two-level staging needs >= 2048 queries
    for shapes, keys, heads, ch, L, nq, P, ok in ((sh, nk, 8, 32, 4, 40000, 8, True), (sh, nk, 8, 32, 4, 2048, 8, True),
                                                  (sh, nk, 8, 32, 4, 2047, 8, False), (sh, nk, 4, 32, 4, 40000, 8, False),
                                                  (sh, nk, 8, 48, 4, 40000, 8, False), (sh, nk, 8, 32, 4, 40000, 4, False),
                                                  (one, 375, 8, 32, 1, 2500, 8, False)):
        size = lib.bevops_value_proj_packed_size(ctypes.addressof(shapes), 6, keys, heads, ch, L, nq, P)
        assert (size > 0) == ok, (keys, heads, ch, L, nq, P, size)
        if not ok:
            assert lib.bevops_value_proj_packed(p, p, p, ctypes.addressof(shapes), p, 1 << 40, 6, keys, heads, ch, L, nq, P,
                                                None) == NOT_SUPPORTED, (keys, heads, ch, L, nq, P)
