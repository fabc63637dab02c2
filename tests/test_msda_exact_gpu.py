"""Bit-exact tests of the fp32 / fp16 MSDA kernel families and the fused SCA entries against the float64 reference
of tests/util_exact_msda.py, on lattice operands that leave the kernels nothing to round except the final store
(tier 1: whole outputs, np.array_equal), and a derived per-output bound on random logits (tier 2).

Families (bevops_msda_set_variant): 0 automatic, 1 / 2 quad kernel with the other point splits, 99 generic, 10 never
head-major, 11 hm, 15 hm2, 16 hm3, 17 hm4, 1000 / 1001 hm5 with / without its visibility pre-pass.  A forced family
outside its domain must answer NOT_SUPPORTED (supported() below says where), never fall back silently.

Narrowing (design/msda.md, "What is pinned bit for bit").  hm3 / hm4 / hm5 blend the four corners of a sample from an
LDS-resident level in packed binary16 before the fp32 accumulation.  From 2 048 queries on, where those kernels stage
the trailing levels of a pyramid, they are therefore compared on the `*-narrow` operands (value amplitude 16 on the
staged levels, same locations and logits); every other family, and these three wherever they stage nothing, runs the
full amplitude.  The fused SCA entries sample with the same kernels and use the narrow operands too; their reference
models the binary16 rounding of every camera's row and the fp32 masked sum (util_exact_msda.expected_sca), so the
amplitude needs no further restriction for the camera reduce.
"""
import functools

import numpy as np
import pytest
import torch

import util_exact_msda as X

pytestmark = pytest.mark.gpu

FP32_VARIANTS = (0, 1, 2, 99, 10)
FP16_VARIANTS = (0, 1, 2, 99, 10, 11, 15, 16, 17, 1000, 1001)
BLEND_FAMILIES = (16, 17, 1000, 1001)          # hm3, hm4, hm5: packed-fp16 blend of LDS-resident levels


def supported(variant, name):
    """Does the forced family take the shape?  hm4 has no kernel for 4 x 8 points with every level staged; hm5 is the
    4-level x 8-point x 4-anchor kernel with two big and two staged levels.  Everything else takes every shape here
    (hm / hm2 are not forced: the call falls through to the layout-preserving kernels)."""
    if variant == 17:
        return not name.startswith("staged")
    if variant in (1000, 1001):
        return name.startswith("ragged")
    return True


def operands_for(variant, shape):
    """Case name of `shape` ('ragged' / 'staged': full or narrow by family; others as they are)."""
    if shape in ("ragged", "staged"):
        return f"{shape}-{'narrow' if variant in BLEND_FAMILIES else 'full'}"
    return shape


@pytest.fixture(scope="module")
def ctx():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    return bev, L, L.load_library()


@functools.lru_cache(maxsize=None)
def case_data(cid):
    c = X.CASES[cid]
    o = X.make_ops(c)
    return c, o, X.reference(c, o)


@functools.lru_cache(maxsize=None)
def device_args(cid, dtype):
    """(value, shapes, ref, off, logit) on the device; shared cases: off / logit as stride-0 views over the cameras."""
    c, o, _ = case_data(cid)
    dt = torch.float32 if dtype == "fp32" else torch.float16
    t = {k: torch.from_numpy(o[k]).to(dt).cuda() for k in ("value", "ref", "off", "logit")}
    for k in t:
        assert torch.equal(t[k].double().cpu(), torch.from_numpy(o[k])), k     # every operand is a binary16 number
    return t["value"], torch.from_numpy(o["shapes"]), t["ref"], t["off"], t["logit"]


def run_variant(ctx, fn, args, variant):
    _, _, handle = ctx
    handle.bevops_msda_set_variant(variant)
    try:
        out = fn(*args)
        torch.cuda.synchronize()
    finally:
        handle.bevops_msda_set_variant(0)
    return out.cpu().numpy()


def assert_bits(got, want, what):
    if not np.array_equal(got, want):
        bad = got != want
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ ({bad.mean():.2%}); first at {i}: "
                             f"got {float(got[i])!r}, want {float(want[i])!r}; max |diff| "
                             f"{np.abs(got.astype(np.float64) - want.astype(np.float64)).max():.4g}")


SHAPES = ("small-1", "small-17", "small-65", "tsa", "ragged", "staged")


# ------------------------------------------------------------------------------------------------ plain MSDA
@pytest.mark.parametrize("variant", FP32_VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_families_bit_exact(ctx, shape, variant):
    bev = ctx[0]
    cid = operands_for(variant, shape) + "-t1"
    c, o, r = case_data(cid)
    args = device_args(cid, "fp32")
    want = X.expected(r, "fp32")
    got = run_variant(ctx, bev.multi_scale_deformable_attn, args, variant)
    assert_bits(got, want, f"fp32 {cid} variant {variant}")
    assert np.array_equal(run_variant(ctx, bev.multi_scale_deformable_attn, args, variant), got)     # deterministic


@pytest.mark.parametrize("variant", FP16_VARIANTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fp16_families_bit_exact(ctx, shape, variant):
    bev, L, _ = ctx
    cid = operands_for(variant, shape) + "-t1"
    c, o, r = case_data(cid)
    args = device_args(cid, "fp16")
    if not supported(variant, shape):
        with pytest.raises(L.BevopsError) as e:
            run_variant(ctx, bev.multi_scale_deformable_attn, args, variant)
        assert e.value.status == L.NOT_SUPPORTED
        return
    want = X.expected(r, "fp16")
    got = run_variant(ctx, bev.multi_scale_deformable_attn, args, variant)
    assert_bits(got, want, f"fp16 {cid} variant {variant}")
    assert np.array_equal(run_variant(ctx, bev.multi_scale_deformable_attn, args, variant), got)     # deterministic


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_other_entries_bit_exact(ctx, shape, dtype):
    """multi_scale_deformable_attn_local (the quad kernel whatever the size) and multi_scale_deformable_attn2."""
    bev = ctx[0]
    cid = operands_for(0, shape) + "-t1"
    c, o, r = case_data(cid)
    args = device_args(cid, dtype)
    want = X.expected(r, dtype)
    for fn in (bev.multi_scale_deformable_attn_local, bev.multi_scale_deformable_attn2):
        got = run_variant(ctx, fn, args, 0)
        assert_bits(got, want, f"{fn.__name__} {dtype} {cid}")
        assert np.array_equal(run_variant(ctx, fn, args, 0), got)


@pytest.mark.parametrize("shape", SHAPES)
def test_prepacked_entry_bit_exact(ctx, shape):
    """msda_pack_value + multi_scale_deformable_attn_prepacked (hm4 on its own planes), where hm4 has a kernel."""
    bev, L, _ = ctx
    from bevformer_tensorrt_amd.functions.multi_scale_deformable_attn import (msda_pack_value,
                                                                              multi_scale_deformable_attn_prepacked)
    cid = operands_for(17, shape) + "-t1"
    c, o, r = case_data(cid)
    value, sh, ref, off, logit = device_args(cid, "fp16")
    if not supported(17, shape):
        with pytest.raises(L.BevopsError) as e:
            msda_pack_value(value, sh, c["nq"], c["P"])
        assert e.value.status == L.NOT_SUPPORTED
        return
    packed = msda_pack_value(value, sh, c["nq"], c["P"])
    want = X.expected(r, "fp16")
    got = multi_scale_deformable_attn_prepacked(packed, ref, off, logit)
    torch.cuda.synchronize()
    assert_bits(got.cpu().numpy(), want, f"prepacked {cid}")
    again = multi_scale_deformable_attn_prepacked(packed, ref, off, logit)
    assert torch.equal(again, got)


@pytest.mark.parametrize("variant", [0, 99, 11, 15, 16, 17])
@pytest.mark.parametrize("shape", ["sca-ragged", "sca-staged"])
def test_shared_offsets_bit_exact(ctx, shape, variant):
    """shared_offsets = 1 of bevops_msda_forward_ws: one [1, nq, heads, .] copy of the offsets / logits for all cameras
    (the wrapper hands stride-0 views over as such).  The operands are the narrow ones for every family."""
    bev, L, _ = ctx
    cid = shape + "-t1"
    c, o, r = case_data(cid)
    value, sh, ref, off, logit = device_args(cid, "fp16")
    args = (value, sh, ref, off.expand(c["bs"], -1, -1, -1), logit.expand(c["bs"], -1, -1, -1))
    if variant == 17 and shape == "sca-staged":
        with pytest.raises(L.BevopsError) as e:
            run_variant(ctx, bev.multi_scale_deformable_attn, args, variant)
        assert e.value.status == L.NOT_SUPPORTED
        return
    want = X.expected(r, "fp16")
    got = run_variant(ctx, bev.multi_scale_deformable_attn, args, variant)
    assert_bits(got, want, f"shared {cid} variant {variant}")
    assert np.array_equal(run_variant(ctx, bev.multi_scale_deformable_attn, args, variant), got)


# ------------------------------------------------------------------------------------------------- fused SCA
def _mask(o):
    return torch.from_numpy(o["mask"]).half().cuda()


def test_sca_mask_patterns_are_present():
    for cid in ("sca-ragged-t1", "sca-staged-t1"):
        c, o, _ = case_data(cid)
        m = o["mask"]
        seen = (m != 0).sum(0)
        assert set(np.unique(m)) == set(X.MASK_WEIGHTS)
        assert (seen == 0).sum() > 50 and (seen == c["bs"]).sum() > 50
        assert ((seen == 1) & (m.max(0) == 1.0)).sum() > 50           # the direct store of the planned sampler
        assert ((seen == 1) & (m.max(0) == 0.5)).sum() > 50           # one camera, but not weight 1: through the reduce


@pytest.mark.parametrize("shape", ["sca-ragged", "sca-staged"])
def test_fused_sca_sample_bit_exact(ctx, shape):
    """spatial_cross_attention_sample (bevops_sca_forward: hm3's masked sampler + sca_camera_reduce)."""
    bev = ctx[0]
    cid = shape + "-t1"
    c, o, r = case_data(cid)
    value, sh, ref, off, logit = device_args(cid, "fp16")
    want = X.expected_sca(c, o, r)
    got = bev.spatial_cross_attention_sample(value, sh, ref, off, logit, _mask(o))
    torch.cuda.synchronize()
    assert_bits(got.cpu().numpy(), want, f"spatial_cross_attention_sample {cid}")
    assert torch.equal(bev.spatial_cross_attention_sample(value, sh, ref, off, logit, _mask(o)), got)


def _packed_sca(ctx, cid, planned):
    """bevops_value_pack_planes + bevops_sca_forward_prepacked / _planned through the C ABI."""
    bev, L, handle = ctx
    c, o, r = case_data(cid)
    value, sh, ref, off, logit = device_args(cid, "fp16")
    mask = _mask(o)
    ncam, nk, heads, ch, nL, nq, P, ppg = c["bs"], c["nk"], c["heads"], c["C"], c["L"], c["nq"], c["P"], c["ppg"]
    st = L.current_stream_ptr(value.device)
    nbytes = handle.bevops_value_proj_packed_size(sh.data_ptr(), ncam, nk, heads, ch, nL, nq, P)
    assert nbytes > 0
    planes = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.check(handle.bevops_value_pack_planes(value.data_ptr(), sh.data_ptr(), planes.data_ptr(), nbytes, ncam, nk, heads,
                                            ch, nL, nq, P, st), "bevops_value_pack_planes")
    ws_bytes = handle.bevops_sca_prepacked_workspace_size(ncam, heads, ch, nq)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.full((1, nq, heads * ch), float("nan"), dtype=torch.float16, device="cuda")
    if planned:
        plan = bev.spatial_cross_attention_plan(mask)
        L.check(handle.bevops_sca_forward_planned(L.F16, planes.data_ptr(), nbytes, sh.data_ptr(), ref.data_ptr(),
                                                  off.data_ptr(), logit.data_ptr(), mask.data_ptr(), plan.data_ptr(),
                                                  plan.numel(), out.data_ptr(), ncam, nk, heads, ch, nL, nq, P, ppg,
                                                  ws.data_ptr(), ws_bytes, st), "bevops_sca_forward_planned")
    else:
        L.check(handle.bevops_sca_forward_prepacked(L.F16, planes.data_ptr(), nbytes, sh.data_ptr(), ref.data_ptr(),
                                                    off.data_ptr(), logit.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                                    ncam, nk, heads, ch, nL, nq, P, ppg, ws.data_ptr(), ws_bytes, st),
                "bevops_sca_forward_prepacked")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_fused_sca_prepacked_bit_exact(ctx):
    """bevops_sca_forward_prepacked (hm5's chunked masked sampler on packed planes + sca_camera_reduce)."""
    cid = "sca-ragged-t1"
    c, o, r = case_data(cid)
    want = X.expected_sca(c, o, r)
    got = _packed_sca(ctx, cid, planned=False)
    assert_bits(got, want, "bevops_sca_forward_prepacked")
    assert np.array_equal(_packed_sca(ctx, cid, planned=False), got)


def test_fused_sca_outside_the_packed_domain_is_not_supported(ctx):
    """Every level staged: the packed planes (two big + two staged levels) do not exist for this pyramid."""
    _, L, handle = ctx
    c, _, _ = case_data("sca-staged-t1")
    sh = torch.tensor(c["levels"], dtype=torch.int32)
    assert handle.bevops_value_proj_packed_size(sh.data_ptr(), c["bs"], c["nk"], 8, 32, 4, c["nq"], 8) == 0


KNOB_DEFAULTS = (3002, 3012, 3010, 3014)


@pytest.mark.parametrize("knobs", [(), (3013,), (3015,), (3013, 3015), (3001,), (3003, 3013), (3011,)])
def test_fused_sca_planned_bit_exact(ctx, knobs):
    """bevops_sca_forward_planned: balanced slices of a visibility plan, single-camera pairs of weight 1 stored
    directly (3012, default) or through the scratch (3013), the folded build (3014, default) or the round-5 build
    (3015), 1 / 2 (default) / 3 slices per CU, the rolled camera reduce (3011)."""
    handle = ctx[2]
    cid = "sca-ragged-t1"
    c, o, r = case_data(cid)
    want = X.expected_sca(c, o, r)
    try:
        for k in knobs:
            handle.bevops_msda_set_variant(k)
        got = _packed_sca(ctx, cid, planned=True)
        again = _packed_sca(ctx, cid, planned=True)
    finally:
        for k in KNOB_DEFAULTS:
            handle.bevops_msda_set_variant(k)
        handle.bevops_msda_set_variant(0)
    assert_bits(got, want, f"bevops_sca_forward_planned knobs {knobs}")
    assert np.array_equal(again, got)


@pytest.mark.parametrize("planned", [False, True])
def test_projected_sca_bit_exact(ctx, planned):
    """spatial_cross_attention_projected at K = 256: features = integers * 2^-4, weight = a signed permutation * 2^4,
    integer bias, so the value projection (tsgemm, the epilogue that writes the sampler's planes) produces exactly the
    lattice's integers and the sampler is exact on them: GEMM epilogue, plane layout and sampler in one exact test."""
    bev = ctx[0]
    cid = "sca-ragged-t1"
    c, o, r = case_data(cid)
    _, sh, ref, off, logit = device_args(cid, "fp16")
    feats, weight, bias = (torch.from_numpy(a).half().cuda() for a in X.projection_operands(c, o))
    mask = _mask(o)
    plan = bev.spatial_cross_attention_plan(mask) if planned else None
    want = X.expected_sca(c, o, r)
    got = bev.spatial_cross_attention_projected(feats, weight, bias, sh, ref, off, logit, mask, c["heads"], plan=plan)
    torch.cuda.synchronize()
    assert_bits(got.cpu().numpy(), want, f"spatial_cross_attention_projected planned={planned}")
    again = bev.spatial_cross_attention_projected(feats, weight, bias, sh, ref, off, logit, mask, c["heads"], plan=plan)
    assert torch.equal(again, got)


# ---------------------------------------------------------------------------------------------------- tier 2
TIER2 = [(s, v) for s in ("tsa", "ragged", "staged") for v in FP16_VARIANTS if supported(v, s)]


@pytest.mark.parametrize("shape,variant", TIER2)
def test_tier2_random_logits_within_the_derived_bound(ctx, shape, variant):
    """Random logits on the lattice locations and values: |out - float64 reference| <= 3 * 2^-11 * A per output,
    A = sum_j softmax_j sum_corners c |v| (util_exact_msda.tier2_bar: the packed weight, the stored result, and one
    2^-11 for __expf, the reciprocal and the fp32 accumulation together); exactly 0 where A is 0.  Every family on every shape it takes (the others answer NOT_SUPPORTED:
    test_fp16_families_bit_exact).  Prints the largest err / A."""
    bev = ctx[0]
    cid = operands_for(variant, shape) + "-t2"
    c, o, r = case_data(cid)
    args = device_args(cid, "fp16")
    got = run_variant(ctx, bev.multi_scale_deformable_attn, args, variant).astype(np.float64)
    err = np.abs(got - r["out"])
    bar = X.tier2_bar(r)
    pos = r["A"] > 0
    ratio = (err[pos] / r["A"][pos]).max()
    print(f"\ntier2 {cid} variant {variant}: max err / A = {ratio:.3e} = {ratio * 2048:.2f} x 2^-11, "
          f"max |err| = {err.max():.3e}")
    assert np.isfinite(got).all()
    assert (got[~pos] == 0).all()                       # no in-gate sample with a non-zero value: exactly 0
    over = err > bar
    assert not over.any(), (int(over.sum()), float(ratio))
