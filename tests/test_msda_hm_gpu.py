"""GPU parity for the head-major fp16 MSDA path (msda_hm.hip): re-layout + octet pairing
+ optional LDS staging.  Same tolerances as tests/test_msda_gpu.py (fp16: 1e-2 element-wise
vs the fp32 oracle on fp16-rounded inputs)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = {"layout_preserving": 10, "hm_no_staging": 11, "hm2_dot2_mailbox": 15, "hm3_padded_lds": 16}

SHAPES = {
    # (bs, levels, nq, P, ppg)
    "tiny_sca": (6, [[15, 25]], 2500, 8, 4),
    "tiny_tsa": (2, [[50, 50]], 2500, 4, 1),
    "small_sca": (6, [[23, 40]], 22500, 8, 4),
    "base_sca_q4k": (6, [[116, 200], [58, 100], [29, 50], [15, 25]], 4000, 8, 4),
    "odd_widths": (3, [[7, 9], [5, 3], [3, 1], [1, 1]], 2100, 4, 2),     # odd W, 1-pixel-wide maps
    "ragged_nq": (2, [[12, 17], [6, 9]], 2049, 2, 1),
    "lp16": (2, [[10, 12], [5, 6]], 300, 8, 2),
}


@pytest.fixture(scope="module")
def ctx():
    import bevformer_tensorrt_amd as b
    from bevformer_tensorrt_amd.utils import load_library
    return b, load_library()


def gen(shape, seed=0, ref_lo=-0.1, ref_hi=1.1, off_std=1.5):
    bs, levels, nq, P, ppg = shape
    heads, C = 8, 32
    g = torch.Generator().manual_seed(seed)
    L = len(levels)
    nk = sum(h * w for h, w in levels)
    value = torch.randn(bs, nk, heads, C, generator=g)
    ref = torch.rand(bs, nq, 1, 2 * ppg, generator=g) * (ref_hi - ref_lo) + ref_lo
    off = torch.randn(bs, nq, heads, L * P * 2, generator=g) * off_std
    logit = torch.randn(bs, nq, heads, L * P, generator=g)
    sh = torch.tensor(levels, dtype=torch.int32)
    return [value.half().cuda(), sh.cuda(), ref.half().cuda(), off.half().cuda(), logit.half().cuda()]


def run(ctx, args, variant):
    bev, lib = ctx
    lib.bevops_msda_set_variant(variant)
    try:
        out = bev.multi_scale_deformable_attn(*args)
        torch.cuda.synchronize()
    finally:
        lib.bevops_msda_set_variant(0)
    return out


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("variant", ["hm_no_staging", "hm2_dot2_mailbox", "hm3_padded_lds"])
def test_hm_vs_oracle(ctx, oracle_mod, name, variant):
    args = gen(SHAPES[name])
    out = run(ctx, args, VARIANTS[variant]).float().cpu().numpy()
    v, sh, r, o, w = (a.float().cpu().numpy() if a.is_floating_point() else a.cpu().numpy() for a in args)
    want = oracle_mod.msda_f32(v, sh, r, o, w)
    assert np.abs(out - want).max() <= 1e-2


@pytest.mark.parametrize("shape", ["base_sca", "base_tsa"])
def test_hm_matches_layout_preserving_kernel_at_full_size(ctx, shape):
    full = {"base_sca": (6, [[116, 200], [58, 100], [29, 50], [15, 25]], 40000, 8, 4),
            "base_tsa": (2, [[200, 200]], 40000, 4, 1)}[shape]
    args = gen(full, ref_lo=0.0, ref_hi=1.0, off_std=1.0)
    base = run(ctx, args, VARIANTS["layout_preserving"]).float()
    for name in ("hm_no_staging", "hm2_dot2_mailbox", "hm3_padded_lds"):
        o = run(ctx, args, VARIANTS[name]).float()
        # all accumulate in fp32 and store fp16; hm2 additionally carries the per-corner weights
        # as half2 into v_dot2c_f32_f16
        tol = 6e-3 if name.startswith(("hm2", "hm3")) else 2e-3
        assert (o - base).abs().max().item() <= tol, name
    # automatic choice == one of the above, and deterministic
    a = run(ctx, args, 0)
    assert torch.equal(a, run(ctx, args, 0))
    assert (a.float() - base).abs().max().item() <= 6e-3


def test_hm_out_of_view_and_zero_pads(ctx):
    """All samples out of range -> exact zeros; and NaNs planted in unrelated workspace bytes
    (previous larger call) never leak: pads are rewritten as zeros by the repack kernel."""
    bev, lib = ctx
    big = gen(SHAPES["small_sca"])
    run(ctx, big, 11)                                   # leaves a large, dirty workspace behind
    args = gen(SHAPES["odd_widths"])
    args[2] = args[2] + 7.0
    out = run(ctx, args, 11)
    assert torch.count_nonzero(out).item() == 0
    args = gen(SHAPES["odd_widths"])
    a, b = run(ctx, args, 11), run(ctx, args, 10)
    assert torch.isfinite(a).all() and (a.float() - b.float()).abs().max().item() <= 2e-3
    c = run(ctx, args, 15)
    assert torch.isfinite(c).all() and (c.float() - b.float()).abs().max().item() <= 6e-3
    args[2] = args[2] + 7.0
    assert torch.count_nonzero(run(ctx, args, 15)).item() == 0
    assert torch.count_nonzero(run(ctx, args, 16)).item() == 0
    for name in ("odd_widths", "small_sca"):            # small_sca: the whole plane lives in LDS
        args = gen(SHAPES[name])
        d = run(ctx, args, 16)
        assert torch.isfinite(d).all()
        assert (d.float() - run(ctx, args, 10).float()).abs().max().item() <= 6e-3


@pytest.mark.parametrize("variant,dtype", [(v, torch.float16) for v in (0, 10, 11, 15, 16, 99)] +
                         [(v, torch.float32) for v in (0, 10, 99)])     # the head-major kernels are fp16-only
def test_camera_shared_offsets_equal_repeated(ctx, variant, dtype):
    """sampling_offsets / attention_weights passed as stride-0 expanded views (the SCA query is
    the same for every camera, spatial_cross_attention.py:254) must give exactly what the
    materialised repeat gives, on every kernel family."""
    bev, lib = ctx
    args = gen((6, [[20, 32], [10, 16], [5, 8], [3, 4]], 2500, 8, 4), ref_lo=-0.2, ref_hi=1.2)
    args = [a.to(dtype) if a.is_floating_point() else a for a in args]
    off1, w1 = args[3][:1].contiguous(), args[4][:1].contiguous()
    rep = [args[0], args[1], args[2], off1.repeat(6, 1, 1, 1), w1.repeat(6, 1, 1, 1)]
    exp = [args[0], args[1], args[2], off1.expand(6, -1, -1, -1), w1.expand(6, -1, -1, -1)]
    a = run(ctx, rep, variant)
    b = run(ctx, exp, variant)
    assert torch.equal(a, b)


def test_full_size_properties_linearity_and_partition_of_unity(ctx):
    """Size-independent properties of the default fp16 path at the full base SCA size
    (6 cams x 30 825 keys x 40 000 queries x 4 levels x 8 points):
      * partition of unity: a constant value map with every sample strictly inside its level
        gives exactly that constant (softmax weights and bilinear weights both sum to 1);
      * linearity in `value`: out(a + b) = out(a) + out(b) up to fp16 rounding."""
    full = (6, [[116, 200], [58, 100], [29, 50], [15, 25]], 40000, 8, 4)
    args = gen(full, ref_lo=0.25, ref_hi=0.75, off_std=0.5)
    ones = [torch.full_like(args[0], 0.75)] + args[1:]
    out = run(ctx, ones, 0).float()
    assert (out - 0.75).abs().max().item() <= 2e-3
    a = args[0]
    b = torch.randn(a.shape, generator=torch.Generator().manual_seed(7)).half().cuda()
    oa = run(ctx, [a] + args[1:], 0).float()
    ob = run(ctx, [b] + args[1:], 0).float()
    oab = run(ctx, [(a.float() + b.float()).half()] + args[1:], 0).float()
    assert (oab - (oa + ob)).abs().max().item() <= 1e-2
