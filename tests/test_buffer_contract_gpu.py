"""Buffer contract of the C ABI (include/bevops.h): an entry writes only its output, stays inside the scratch bytes
its own size query reports, and the alignment the header documents is sufficient.

The standard check (design/buffers.md): inputs, outputs and scratch live in a guarded arena (tests/util_arena.py);
scratch is exactly the bytes the entry's size query returns and outputs exactly their size, every buffer at the
documented alignment and no better; the call runs once per poison (0xFF: NaN as a float, 0x55: finite) with output and
scratch pre-filled with the poison; status 0; every guard byte intact; outputs bit-identical under the two poisons (a
read of a guard, of unwritten scratch or of stale output shows as NaN or as a difference) and bit-identical to the
ordinary wrapper call; and the wrapper result within the operator's existing bar of its existing reference on the
shape used here (helpers imported from the operator's own test module).  Kernel families the library would silently
fall back from are pinned with the *_set_variant hooks, so their own status comes back."""
import numpy as np
import pytest
import torch

from util_arena import POISONS, Arena

import test_msda_hm5_gpu as hm5_tests
import test_msda_hm_gpu as hm_tests
import test_sca_fused_gpu as sca_tests
from test_msda_hm4_gpu import same_as_quad
from test_msda_int8_gpu import quantize

pytestmark = pytest.mark.gpu

MiB = 1 << 20
MSDA_WS_ALIGN = 128     # bevops_msda_forward_ws / bevops_sca_forward workspace, packed planes (include/bevops.h)
TENSOR_ALIGN = 16       # "tensors are dense, row-major, 16-byte aligned"


@pytest.fixture(scope="module")
def ctx():
    import bevformer_tensorrt_amd as b
    from bevformer_tensorrt_amd.utils import lib as L
    return b, L.load_library(), L


def fmod(name):
    """A module of bevformer_tensorrt_amd.functions (several share their name with the function the package exports)."""
    import importlib
    return importlib.import_module("bevformer_tensorrt_amd.functions." + name)


def bits(t):
    t = t.permute(0, 2, 3, 1) if t.dim() == 4 and not t.is_contiguous() else t
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def both_poisons(capacity, body):
    """Run body(arena) -> tensors once per poison; guards intact, results equal bit for bit.  Returns the results."""
    runs = []
    for poison in POISONS:
        arena = Arena(capacity, poison)
        outs = body(arena)
        arena.check()
        runs.append([o.clone() for o in outs])
        del arena, outs
    for i, (a, b) in enumerate(zip(*runs)):
        assert same_bits(a, b), f"output {i} differs between the two poisons: it depends on bytes the call never wrote"
    return runs[0]


# ---- the arena itself ----------------------------------------------------------------------------------------------
def test_arena_detects_overrun_and_guard_read():
    """torch ops only, inside the test's own allocation: a write one element past a carved view is reported with the
    buffer, the side and the offsets; a read of a guard yields NaN (0xFF) or the poison value (0x55)."""
    for poison in POISONS:
        arena = Arena(1 * MiB, poison)
        x = arena.empty((5, 7), torch.float16, TENSOR_ALIGN, "x")
        y = arena.place(torch.arange(24, dtype=torch.float32).view(1, 2, 3, 4), TENSOR_ALIGN, "y", channels_last=True)
        assert x.data_ptr() % 16 == 0 and x.data_ptr() % 32 != 0 and x.is_contiguous()
        assert y.is_contiguous(memory_format=torch.channels_last) and y.flatten().sum().item() == 276.0
        x.zero_()
        arena.check()
        name, start, nbytes, guard = arena.views[0]
        assert (name, nbytes) == ("x", 70) and guard >= 64 * 1024
        whole = arena.buf.view(torch.float16)
        behind = whole[(start + nbytes) // 2].clone()   # the element one past the view, through the arena itself
        front = whole[start // 2 - 1]
        if poison == 0xFF:
            assert torch.isnan(behind) and torch.isnan(front) and torch.isnan((behind * 0.0))
        else:
            assert behind.view(torch.int16).item() == 0x5555 and torch.isfinite(front)
        whole[(start + nbytes) // 2] = 1.0              # the one-element overrun
        assert arena.disturbed() == [("x", "behind", 0, 1, 2)]
        with pytest.raises(AssertionError, match="x: 2 bytes behind, offsets 0..1"):
            arena.check()
        whole[(start + nbytes) // 2] = behind
        arena.buf[start - 3] = 0                        # ... and a byte in front
        assert arena.disturbed() == [("x", "front", 2, 2, 1)]
        # scratch guards are as wide as the buffer (to 8 MiB)
        arena2 = Arena(1 * MiB, poison)
        arena2.carve(200 * 1024, 128, "ws", scratch=True)
        assert arena2.views[0][3] == 200 * 1024


# ---- MSDA through the wrapper (it has out=) with exact-size lent scratch ----------------------------------------------
def msda_capacity(args):
    """Room for the operands, the largest head-major re-layout (two copies of `value` in 128-byte entries) and guards."""
    value = args[0]
    return 6 * value.numel() * value.element_size() + sum(a.numel() * a.element_size() for a in args) + 64 * MiB


def msda_contract(ctx, monkeypatch, args, variant, scales=None, head_major=True):
    """The standard check of bevops_msda_forward_ws for one forced family: returns (arena result, wrapper result)."""
    bev, lib, L = ctx
    M = fmod("multi_scale_deformable_attn")
    from bevformer_tensorrt_amd.utils import workspace
    names = ("value", "shapes", "ref", "off", "logit")
    dt = L.torch_dtype_code(args[0])
    bs, nk, heads, ch = args[0].shape
    Lv, nq = args[1].shape[0], args[3].shape[1]
    P = args[4].shape[-1] // Lv
    lib.bevops_msda_set_variant(variant)
    try:
        plain = M._msda(*args, scales or (1.0,) * 4)
        torch.cuda.synchronize()
        shapes_host = args[1].cpu().contiguous()
        need = lib.bevops_msda_workspace_size_shapes(dt, shapes_host.data_ptr(), bs, nk, heads, ch, Lv, nq, P)
        assert need > 0

        def body(arena):
            placed = [arena.place(a, 4 if n == "shapes" else TENSOR_ALIGN, n) for n, a in zip(names, args)]
            out = arena.empty(plain.shape, plain.dtype, TENSOR_ALIGN, "out")
            log = []
            monkeypatch.setattr(workspace, "lend", arena.lender(MSDA_WS_ALIGN, log))
            M._msda(*placed, scales or (1.0,) * 4, out=out)      # raises on a non-zero status
            torch.cuda.synchronize()
            assert [n for _, n, _ in log] == [need], "scratch is exactly the shape-aware query's bytes"
            if head_major:      # the family under test ran: it re-laid `value` out into the scratch it was lent
                assert bool((log[0][2] != arena.poison).any()), "workspace untouched: the library fell back"
            return [out]
        got = both_poisons(msda_capacity(args), body)[0]
    finally:
        lib.bevops_msda_set_variant(0)
        monkeypatch.undo()
        workspace.release()
    assert same_bits(got, plain), "arena call differs from the ordinary wrapper call"
    return got, plain


HM_CASES = [(name, v) for name in ("odd_widths", "ragged_nq", "lp16") for v in (11, 15, 16)] + [("ragged_nq", 17)]
# (hm4 is instantiated for L*P in {4, 8, 32}: of the three ragged shapes only ragged_nq; hm5 needs 4 levels x 8 points)
HM5_SHAPES = {"other_level_sizes": dict(bs=3, nq=2600, seed=5, levels=[[90, 161], [45, 81], [23, 41], [1, 21]]),
              "base_levels_nq2049": dict(bs=2, nq=2049, seed=2049, levels=hm5_tests.LEVELS)}
_ORACLE = {}


def msda_oracle(oracle_mod, key, args):
    """The fp32 oracle of a shape, computed once per module run."""
    if key not in _ORACLE:
        _ORACLE[key] = hm5_tests.oracle(oracle_mod, args)
    return _ORACLE[key]


@pytest.mark.parametrize("name,variant", HM_CASES)
def test_msda_fp16_forced_family_ragged_shapes(ctx, monkeypatch, oracle_mod, name, variant):
    args = hm_tests.gen(hm_tests.SHAPES[name])
    got, plain = msda_contract(ctx, monkeypatch, args, variant)
    assert np.abs(plain.float().cpu().numpy() - msda_oracle(oracle_mod, name, args)).max() <= 1e-2


@pytest.mark.parametrize("variant", [11, 15, 16, 17, 1000, 1001])
@pytest.mark.parametrize("name", list(HM5_SHAPES))
def test_msda_fp16_forced_family_sca_pyramids(ctx, monkeypatch, oracle_mod, name, variant):
    s = HM5_SHAPES[name]
    args = hm5_tests.gen(s["bs"], s["nq"], seed=s["seed"], mode="edge", levels=s["levels"])
    got, plain = msda_contract(ctx, monkeypatch, args, variant)
    assert np.abs(plain.float().cpu().numpy() - msda_oracle(oracle_mod, name, args)).max() <= 1e-2


def msda_direct(ctx, arena, args, ws_bytes, scales=(1.0,) * 4, shapes_host=None):
    """bevops_msda_forward_ws on arena buffers with a workspace of exactly ws_bytes; returns (status, out, workspace)."""
    bev, lib, L = ctx
    names = ("value", "shapes", "ref", "off", "logit")
    value, sh, ref, off, logit = [arena.place(a, 4 if n == "shapes" else TENSOR_ALIGN, n) for n, a in zip(names, args)]
    bs, nk, heads, ch = value.shape
    Lv, nq = sh.shape[0], off.shape[1]
    P = logit.shape[-1] // Lv
    out = arena.empty((bs, nq, heads, ch), value.dtype, TENSOR_ALIGN, "out")
    ws = arena.carve(ws_bytes, MSDA_WS_ALIGN, "workspace", scratch=True)
    st = lib.bevops_msda_forward_ws(L.torch_dtype_code(value), value.data_ptr(), sh.data_ptr(), shapes_host.data_ptr(),
                                    ref.data_ptr(), L.torch_dtype_code(ref), off.data_ptr(), logit.data_ptr(),
                                    out.data_ptr(), bs, nk, heads, ch, Lv, nq, P, ref.shape[-1] // 2, *scales, 0,
                                    ws.data_ptr(), ws_bytes, L.current_stream_ptr(value.device))
    torch.cuda.synchronize()
    return st, out, ws


@pytest.mark.parametrize("variant", [11, 15])
@pytest.mark.parametrize("name", ["odd_widths", "ragged_nq", "lp16"])
def test_msda_fp16_coarse_query_is_enough_for_hm_and_hm2(ctx, name, variant):
    """hm / hm2 (msda_hm.hip) need no level shapes: they accept the coarser bevops_msda_workspace_size and must stay
    inside it."""
    bev, lib, L = ctx
    args = hm_tests.gen(hm_tests.SHAPES[name])
    bs, nk, heads, ch = args[0].shape
    Lv, nq = args[1].shape[0], args[3].shape[1]
    P = args[4].shape[-1] // Lv
    shapes_host = args[1].cpu().contiguous()
    lib.bevops_msda_set_variant(variant)
    try:
        coarse = lib.bevops_msda_workspace_size(L.F16, bs, nk, heads, ch, Lv, nq, P)
        assert 0 < coarse <= lib.bevops_msda_workspace_size_shapes(L.F16, shapes_host.data_ptr(), bs, nk, heads, ch, Lv, nq, P)
        plain = bev.multi_scale_deformable_attn(*args)

        def body(arena):
            st, out, ws = msda_direct(ctx, arena, args, coarse, shapes_host=shapes_host)
            assert st == 0
            assert bool((ws != arena.poison).any()), "workspace untouched: the library fell back"
            return [out]
        got = both_poisons(msda_capacity(args), body)[0]
    finally:
        lib.bevops_msda_set_variant(0)
    assert same_bits(got, plain)


@pytest.mark.parametrize("variant", [17, 19])
def test_msda_int8_hm4_accepts_the_coarse_query(ctx, variant):
    """The int8 bevops_msda_workspace_size is an upper bound of the exact size: hm4 lent exactly that many bytes runs
    (the workspace is written) and stays inside them -- on the pyramid with a one-row level, where the bound is tight."""
    bev, lib, L = ctx
    args, scales = int8_args(HM5_SHAPES["other_level_sizes"], torch.float32)
    bs, nk, heads, ch = args[0].shape
    Lv, nq, P = args[1].shape[0], args[3].shape[1], 8
    shapes_host = args[1].cpu().contiguous()
    lib.bevops_msda_set_variant(variant)
    try:
        coarse = lib.bevops_msda_workspace_size(L.I8, bs, nk, heads, ch, Lv, nq, P)
        assert coarse >= lib.bevops_msda_workspace_size_shapes(L.I8, shapes_host.data_ptr(), bs, nk, heads, ch, Lv, nq, P) > 0
        plain = bev.multi_scale_deformable_attn_int8(*args, *scales)

        def body(arena):
            st, out, ws = msda_direct(ctx, arena, args, coarse, scales, shapes_host=shapes_host)
            assert st == 0
            assert bool((ws != arena.poison).any()), "workspace untouched: the library fell back"
            return [out]
        got = both_poisons(msda_capacity(args) + 2 * coarse, body)[0]
    finally:
        lib.bevops_msda_set_variant(0)
    assert same_bits(got, plain)


def int8_args(s, ref_dtype):
    bs, levels, nq = s["bs"], s["levels"], s["nq"]
    heads, C, P, ppg = 8, 32, 8, 4
    g = torch.Generator().manual_seed(s["seed"])
    nk = sum(h * w for h, w in levels)
    value = torch.randn(bs, nk, heads, C, generator=g)
    ref = torch.rand(bs, nq, 1, 2 * ppg, generator=g) * 1.2 - 0.1
    off = torch.randn(bs, nq, heads, len(levels) * P * 2, generator=g)
    logit = torch.randn(bs, nq, heads, len(levels) * P, generator=g)
    qv, s_v = quantize(value); qo, s_o = quantize(off); qw, s_w = quantize(logit)
    args = [qv.cuda(), torch.tensor(levels, dtype=torch.int32).cuda(), ref.to(ref_dtype).cuda(), qo.cuda(), qw.cuda()]
    return args, (s_v, s_o, s_w, 0.02)


@pytest.mark.parametrize("ref_dtype", [torch.float32, torch.float16], ids=["s8w_f32ref", "u8w_f16ref"])
@pytest.mark.parametrize("variant", [17, 19])
@pytest.mark.parametrize("name", list(HM5_SHAPES))
def test_msda_int8_hm4_both_plans_and_flavours(ctx, monkeypatch, oracle_mod, name, variant, ref_dtype):
    """int8 hm4 on the two-blocks (17) and the one-block plan (19), x127 and x255 weights.  (hm4 has no kernel for the
    L*P = 16 ragged shapes and the entry itself turns P = 2 away for int8: the two SCA pyramids are its ragged cases
    here -- a one-row level, a last chunk of one query.)  Reference: the layout-preserving int8 kernel at the bar of
    tests/test_msda_hm4_gpu.py, and the C oracle of the integer arithmetic at the bar of tests/test_msda_int8_gpu.py."""
    bev, lib, L = ctx
    args, scales = int8_args(HM5_SHAPES[name], ref_dtype)
    got, plain = msda_contract(ctx, monkeypatch, args, variant, scales)
    lib.bevops_msda_set_variant(10)
    try:
        quad = bev.multi_scale_deformable_attn_int8(*args, *scales)
    finally:
        lib.bevops_msda_set_variant(0)
    same_as_quad(plain, quad, ref_dtype, name)
    key = (name, "s8", ref_dtype)
    if key not in _ORACLE:
        qv, sh, ref, qo, qw = (a.cpu() for a in args)
        _ORACLE[key] = oracle_mod.msda_s8(qv.numpy(), scales[0], sh.numpy(), ref.float().numpy(), qo.numpy(), scales[1],
                                          qw.numpy(), scales[2], scales[3],
                                          u8_weights=(ref_dtype == torch.float16)).astype(np.int32)
    d = np.abs(plain.cpu().numpy().astype(np.int32) - _ORACLE[key])
    assert d.max() <= 1 and (d > 0).mean() <= 0.01


@pytest.mark.parametrize("flavour", ["fp16", "s8w_f32ref", "u8w_f16ref"])
def test_msda_pack_value_and_prepacked(ctx, oracle_mod, flavour):
    """bevops_msda_pack_value + bevops_msda_forward_prepacked: `packed` is exactly bevops_msda_packed_size bytes at
    128; the pack writes inside it, the sampler reads inside it; equal bits to the wrapper pair."""
    bev, lib, L = ctx
    s = HM5_SHAPES["other_level_sizes"]
    if flavour == "fp16":
        args, scales = hm5_tests.gen(s["bs"], s["nq"], seed=s["seed"], mode="edge", levels=s["levels"]), (1.0,) * 4
    else:
        args, scales = int8_args(s, torch.float32 if flavour.startswith("s8w") else torch.float16)
    value, sh, ref, off, logit = args
    bs, nk, heads, ch = value.shape
    Lv, nq, P = sh.shape[0], off.shape[1], 8
    dt, rdt = L.torch_dtype_code(value), L.torch_dtype_code(ref)
    shapes_host = sh.cpu().contiguous()
    need = lib.bevops_msda_packed_size(dt, shapes_host.data_ptr(), bs, nk, heads, ch, Lv, nq, P)
    assert need > 0
    packed = bev.msda_pack_value(value, sh, nq, P, reference_dtype=ref.dtype)
    assert packed.data.numel() == need
    plain = bev.multi_scale_deformable_attn_prepacked(packed, ref, off, logit, scales)
    torch.cuda.synchronize()

    def body(arena):
        v, r, o, w = (arena.place(t, TENSOR_ALIGN, n) for t, n in zip((value, ref, off, logit), ("value", "ref", "off", "logit")))
        out = arena.empty(plain.shape, plain.dtype, TENSOR_ALIGN, "out")
        pk = arena.carve(need, MSDA_WS_ALIGN, "packed", scratch=True)
        st = L.current_stream_ptr(value.device)
        assert lib.bevops_msda_pack_value(dt, rdt, v.data_ptr(), shapes_host.data_ptr(), pk.data_ptr(), need, bs, nk, heads,
                                          ch, Lv, nq, P, st) == 0
        assert lib.bevops_msda_forward_prepacked(dt, pk.data_ptr(), need, shapes_host.data_ptr(), r.data_ptr(), rdt,
                                                 o.data_ptr(), w.data_ptr(), out.data_ptr(), bs, nk, heads, ch, Lv, nq, P, 4,
                                                 *scales, 0, st) == 0
        return [out]
    got = both_poisons(msda_capacity(args), body)[0]
    assert same_bits(got, plain)
    if flavour == "fp16":
        assert np.abs(plain.float().cpu().numpy() - msda_oracle(oracle_mod, "other_level_sizes", args)).max() <= 1e-2
    else:
        lib.bevops_msda_set_variant(10)
        try:
            quad = bev.multi_scale_deformable_attn_int8(*args, *scales)
        finally:
            lib.bevops_msda_set_variant(0)
        same_as_quad(plain, quad, ref.dtype, flavour)


# ---- fused SCA ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "ragged_chunk"])
def test_sca_forward(ctx, oracle_mod, name):
    bev, lib, L = ctx
    value, sh, ref, off, logit, mask = sca_tests.gen(sca_tests.SHAPES[name])
    ncam, nk, heads, ch = value.shape
    Lv, nq = sh.shape[0], off.shape[1]
    P = logit.shape[-1] // Lv
    shapes_host = sh.cpu().contiguous()
    need = lib.bevops_sca_workspace_size(L.F16, shapes_host.data_ptr(), ncam, nk, heads, ch, Lv, nq, P)
    assert need > 0
    plain = bev.spatial_cross_attention_sample(value, sh, ref, off, logit, mask)
    torch.cuda.synchronize()

    def body(arena):
        v, r, o, w, m = (arena.place(t, TENSOR_ALIGN, n) for t, n in
                         zip((value, ref, off, logit, mask), ("value", "ref", "off", "logit", "mask")))
        out = arena.empty(plain.shape, plain.dtype, TENSOR_ALIGN, "out")
        ws = arena.carve(need, MSDA_WS_ALIGN, "workspace", scratch=True)
        assert lib.bevops_sca_forward(L.F16, v.data_ptr(), shapes_host.data_ptr(), r.data_ptr(), o.data_ptr(), w.data_ptr(),
                                      m.data_ptr(), out.data_ptr(), ncam, nk, heads, ch, Lv, nq, P, ref.shape[-1] // 2,
                                      ws.data_ptr(), need, L.current_stream_ptr(value.device)) == 0
        return [out]
    got = both_poisons(4 * need + 64 * MiB, body)[0]
    assert same_bits(got, plain)
    v, s_, r, o, w = (a.float().cpu().numpy() if a.is_floating_point() else a.cpu().numpy()
                      for a in (value, sh, ref, off.expand(ncam, -1, -1, -1).contiguous(),
                                logit.expand(ncam, -1, -1, -1).contiguous()))
    q = oracle_mod.msda_f32(v, s_, r, o, w).reshape(ncam, -1, 256)
    want = (q * mask.float().cpu().numpy()[:, :, None]).sum(0, keepdims=True)
    assert np.abs(plain.float().cpu().numpy() - want).max() <= 1e-2


def projected_case():
    """The projected SCA path on the smallest ragged pyramid of its sampler's tests (tests/test_msda_hm5_gpu.py:
    other_level_sizes -- odd widths, a one-row level; 3 cameras, 2600 queries = two chunks and a ragged one)."""
    s = HM5_SHAPES["other_level_sizes"]
    g = torch.Generator().manual_seed(7)
    ncam, nq, heads, embed = s["bs"], s["nq"], 8, 256
    nk = sum(h * w for h, w in s["levels"])
    feats = (torch.randn(ncam, nk, embed, generator=g) * 0.5).half().cuda()
    wgt = (torch.randn(embed, embed, generator=g) / 16).half().cuda()
    bias = (torch.randn(embed, generator=g) * 0.1).half().cuda()
    off = (torch.randn(1, nq, heads, 64, generator=g) * 2).half().cuda()
    w = torch.randn(1, nq, heads, 32, generator=g).half().cuda()
    ref = (torch.rand(ncam, nq, 1, 8, generator=g) * 1.2 - 0.1).half().cuda()
    vis = torch.rand(ncam, nq, generator=g) < torch.tensor([0.05, 0.9, 0.3]).view(3, 1)
    bm = (vis.float() / vis.sum(0).clamp(min=1)).half().cuda()
    sh = torch.tensor(s["levels"], dtype=torch.int32)
    return feats, wgt, bias, sh, ref, off, w, bm, heads


@pytest.mark.parametrize("mode", ["prepacked", "planned_3012_3014", "planned_3013_3015"])
def test_value_proj_packed_and_sca_prepacked_planned(ctx, mode):
    """bevops_value_proj_packed (planes exactly bevops_value_proj_packed_size bytes at 128) feeding
    bevops_sca_forward_prepacked, or bevops_sca_plan_build (plan exactly bevops_sca_plan_size bytes at 16) +
    bevops_sca_forward_planned under both settings of the direct-store and the folded-broadcast knobs; the sampler's
    workspace is exactly bevops_sca_prepacked_workspace_size bytes at 16."""
    bev, lib, L = ctx
    feats, wgt, bias, sh, ref, off, w, bm, heads = projected_case()
    ncam, nk, embed = feats.shape
    nq, ch, Lv, P, ppg = off.shape[1], embed // heads, 4, 8, 4
    pk_bytes = lib.bevops_value_proj_packed_size(sh.data_ptr(), ncam, nk, heads, ch, Lv, nq, P)
    ws_bytes = lib.bevops_sca_prepacked_workspace_size(ncam, heads, ch, nq)
    plan_bytes = lib.bevops_sca_plan_size(ncam, nq)
    assert pk_bytes > 0 and ws_bytes > 0 and plan_bytes > 0
    knobs = {"prepacked": (), "planned_3012_3014": (3012, 3014), "planned_3013_3015": (3013, 3015)}[mode]
    try:
        for k in knobs:
            lib.bevops_msda_set_variant(k)
        plan_t = bev.spatial_cross_attention_plan(bm) if knobs else None
        plain = bev.spatial_cross_attention_projected(feats, wgt, bias, sh, ref, off, w, bm, heads, plan=plan_t)
        torch.cuda.synchronize()

        def body(arena):
            x, wg, b, r, o, lw, m = (arena.place(t, TENSOR_ALIGN, n) for t, n in zip(
                (feats, wgt, bias, ref, off, w, bm), ("feats", "weight", "bias", "ref", "off", "logit", "mask")))
            out = arena.empty(plain.shape, plain.dtype, TENSOR_ALIGN, "out")
            pk = arena.carve(pk_bytes, MSDA_WS_ALIGN, "packed", scratch=True)
            ws = arena.carve(ws_bytes, TENSOR_ALIGN, "workspace", scratch=True)
            st = L.current_stream_ptr(feats.device)
            assert lib.bevops_value_proj_packed(x.data_ptr(), wg.data_ptr(), b.data_ptr(), sh.data_ptr(), pk.data_ptr(),
                                                pk_bytes, ncam, nk, heads, ch, Lv, nq, P, st) == 0
            if not knobs:
                assert lib.bevops_sca_forward_prepacked(L.F16, pk.data_ptr(), pk_bytes, sh.data_ptr(), r.data_ptr(),
                                                        o.data_ptr(), lw.data_ptr(), m.data_ptr(), out.data_ptr(), ncam, nk,
                                                        heads, ch, Lv, nq, P, ppg, ws.data_ptr(), ws_bytes, st) == 0
                return [out]
            plan = arena.carve(plan_bytes, TENSOR_ALIGN, "plan", scratch=True)
            assert lib.bevops_sca_plan_build(L.F16, m.data_ptr(), ncam, nq, plan.data_ptr(), plan_bytes, st) == 0
            assert lib.bevops_sca_forward_planned(L.F16, pk.data_ptr(), pk_bytes, sh.data_ptr(), r.data_ptr(), o.data_ptr(),
                                                  lw.data_ptr(), m.data_ptr(), plan.data_ptr(), plan_bytes, out.data_ptr(),
                                                  ncam, nk, heads, ch, Lv, nq, P, ppg, ws.data_ptr(), ws_bytes, st) == 0
            return [out]
        got = both_poisons(2 * pk_bytes + 2 * ws_bytes + feats.numel() * 2 + 64 * MiB, body)[0]
    finally:
        for k in (3012, 3014, 0):
            lib.bevops_msda_set_variant(k)
    assert same_bits(got, plain)
    # the operator's existing reference and bar (test_projected_path_matches_projection_plus_fused_sampling)
    value = torch.nn.functional.linear(feats, wgt, bias).view(ncam, nk, heads, 32)
    want = bev.spatial_cross_attention_sample(value, sh, ref, off, w, bm).float()
    err = (plain.float() - want).abs()
    assert torch.isfinite(plain.float()).all() and err.max().item() <= 2e-2 and err.mean().item() <= 5e-4


# ---- wrappers without out=: their allocations are served from the arena ---------------------------------------------
class ArenaTorch:
    """Stands in for the `torch` module inside ONE wrapper module for the duration of a call: `empty`, `empty_like` and
    `zeros` on the GPU come from the arena -- exactly the bytes of the tensor, at TENSOR_ALIGN, guarded, pre-filled
    with the poison -- and everything else is torch's.  The wrapper then hands arena pointers to the entry it wraps,
    which is what a direct ctypes call with arena pointers does, without restating every argument list here."""

    def __init__(self, arena):
        self._arena, self._n = arena, 0
        self.scratch = []       # bytes of the 1-D uint8 buffers the wrapper allocated for itself (workspace, packed operands)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, memory_format=None, **kw):
        assert not kw, f"ArenaTorch.empty: arguments it does not know how to honour: {sorted(kw)}"
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        count = int(np.prod(shape)) if shape else 1
        if device is None or torch.device(device).type != "cuda" or count == 0:
            return torch.empty(*size, dtype=dtype, device=device)
        self._n += 1
        scratch = dtype is torch.uint8 and len(shape) == 1      # a wrapper's own workspace / packed operand: wide guards
        if scratch:
            self.scratch.append(count)
        return self._arena.empty(shape, dtype or torch.float32, TENSOR_ALIGN, f"alloc{self._n}", scratch=scratch,
                                 channels_last=memory_format is torch.channels_last)

    def empty_like(self, x, **kw):
        assert not set(kw) - {"dtype"}, sorted(kw)
        return self.empty(x.shape, dtype=kw.get("dtype", x.dtype), device=x.device,
                          memory_format=torch.channels_last if is_channels_last(x) else None)

    def zeros(self, *size, dtype=None, device=None, **kw):
        t = self.empty(*size, dtype=dtype, device=device, **kw)
        return t.zero_()


def is_channels_last(t):
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def wrapper_contract(monkeypatch, modules, call, inputs, inplace=(), ws_align=TENSOR_ALIGN, capacity=64 * MiB,
                     bitwise=True, scratch_sizes=None, own_scratch=None, verify=None, entries=(), not_entries=()):
    """The standard check through a wrapper: `call(**inputs)` once on ordinary tensors, then once per poison with
    every device tensor of `inputs` placed in the arena, the wrapper's allocations and lent scratch served from it.
    `inplace`: inputs the entry overwrites (cloned per run).  `bitwise=False` (an entry that is not run-to-run
    deterministic by design): the arena result goes to `verify` instead of being compared with the ordinary call's
    bits.  `scratch_sizes`: the sizes `lend` must be asked for; `own_scratch`: the sizes of the 1-D uint8 buffers the
    wrapper must allocate for itself (its workspace, its packed operands), so that scratch cannot quietly leave the
    arena.  `entries` / `not_entries`: C-ABI entries every run must / must not reach (where the wrapper routes).
    Returns the ordinary call's outputs as a list."""
    from bevformer_tensorrt_amd.utils import workspace

    def as_list(r):
        return list(r) if isinstance(r, (tuple, list)) else [r]

    from bevformer_tensorrt_amd.utils import load_library
    lib, reached = load_library(), {}
    routing = pytest.MonkeyPatch()
    for name in tuple(entries) + tuple(not_entries):
        def counted(*a, _f=getattr(lib, name), _n=name):
            reached[_n] = reached.get(_n, 0) + 1
            return _f(*a)
        routing.setattr(lib, name, counted)

    def fresh(k, v):
        return v.clone(memory_format=torch.preserve_format) if k in inplace else v
    try:
        plain = as_list(call(**{k: fresh(k, v) for k, v in inputs.items()}))
        torch.cuda.synchronize()
    except BaseException:
        routing.undo()
        raise

    def body(arena):
        placed = {k: arena.place(v, TENSOR_ALIGN, k, channels_last=is_channels_last(v))
                  if torch.is_tensor(v) and v.is_cuda else v for k, v in inputs.items()}
        log = []
        proxy = ArenaTorch(arena)
        with pytest.MonkeyPatch.context() as patch:      # (its own context: the caller's patches stay in force)
            for m in modules:
                patch.setattr(m, "torch", proxy)
            patch.setattr(workspace, "lend", arena.lender(ws_align, log))
            outs = as_list(call(**placed))
            torch.cuda.synchronize()
        lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.buf.numel()
        for o in outs:
            assert lo <= o.data_ptr() < hi, "an output was allocated outside the arena"
        if scratch_sizes is not None:
            assert [n for _, n, _ in log] == list(scratch_sizes), ([n for _, n, _ in log], scratch_sizes)
        if own_scratch is not None:
            assert proxy.scratch == list(own_scratch), (proxy.scratch, own_scratch)
        return outs
    try:
        got = both_poisons(capacity, body)
    finally:
        routing.undo()
        workspace.release()
        for m in modules:       # packed operands cached per weight tensor would keep the arenas alive
            for cache in vars(m).values():
                if type(cache).__name__ == "_TensorCache":
                    cache._d.clear()
    for name in entries:
        assert reached.get(name, 0) == 1 + len(POISONS), f"{name} was reached {reached.get(name, 0)} times"
    for name in not_entries:
        assert name not in reached, f"{name} was reached: the wrapper routed elsewhere"
    if bitwise:
        for i, (a, b) in enumerate(zip(got, plain)):
            assert same_bits(a, b), f"output {i}: arena call differs from the ordinary wrapper call"
    if verify is not None:
        verify(got)
    return plain


def dense_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).half().cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half().cuda()
    b = torch.randn(N, generator=g).half().cuda()
    r = torch.randn(M, N, generator=g).half().cuda()
    return x, w, b, r


def dense_bar(got, x, w, b, r, relu, floor=0.0):
    """The fp32 reference of tests/test_tile_gemm_gpu.py at the bar of the operator's own module: tsgemm 1e-3 |want| +
    2e-3, tile / small GEMM 1e-3 max(|want|, 1) + 2e-3 (floor = 1)."""
    from test_tile_gemm_gpu import _ref
    want = _ref(x, w, b, r, relu)
    err = (got.float() - want).abs()
    assert bool((err <= 1e-3 * want.abs().clamp_min(floor) + 2e-3).all()), float(err.max())


# rows: one more and one less than two row tiles; columns / k: the smallest legal count that is
# no multiple of the tile (tsgemm's domain is whole column tiles: N % 256 == 0, K % 64 == 0 -> one of each, K = 192 = 3 steps)
GEMMS = {"tsgemm": (160, 256, 192), "tile_gemm": (128, 136, 72), "small_gemm": (32, 72, 64)}


@pytest.mark.parametrize("rows", [-1, 1])
@pytest.mark.parametrize("name", list(GEMMS))
def test_gemm_f16_tail_rows(ctx, monkeypatch, name, rows):
    mod = fmod("linear")
    tile, N, K = GEMMS[name]
    M = 2 * tile + rows          # three row tiles, the last of one row / one row short
    x, w, b, r = dense_operands(M, N, K, M + N + K)
    fn = getattr(mod, name)
    plain = wrapper_contract(monkeypatch, [mod], lambda x, w, b, r: fn(x, w, b, r, True), dict(x=x, w=w, b=b, r=r))[0]
    assert plain.shape == (M, N)
    dense_bar(plain, x, w, b, r, True, floor=0.0 if name == "tsgemm" else 1.0)


@pytest.mark.parametrize("M", [159, 161])
def test_tsgemm_ln_tail_rows(ctx, monkeypatch, M):
    import torch.nn.functional as TF
    mod = fmod("linear")
    N, K = 256, 192
    x, w, b, r = dense_operands(M, N, K, M + K)
    g = torch.Generator().manual_seed(M)
    gam, bet = (1 + 0.2 * torch.randn(N, generator=g)).half().cuda(), (0.1 * torch.randn(N, generator=g)).half().cuda()
    plain = wrapper_contract(monkeypatch, [mod], lambda **a: mod.tsgemm_ln(a["x"], a["w"], a["b"], a["r"], a["gam"], a["bet"], 1e-5),
                             dict(x=x, w=w, b=b, r=r, gam=gam, bet=bet))[0]
    y = x.float() @ w.float().t() + b.float() + r.float()       # the reference and bars of test_tsgemm_with_layer_norm_epilogue
    want = TF.layer_norm(y.half().float(), (N,), gam.float(), bet.float(), 1e-5)
    err = (plain.float() - want).abs()
    assert err.max().item() <= 2e-2 and err.mean().item() <= 6e-4


def int8_dense(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).half().cuda()
    w = torch.randn(N, K, generator=g) / K ** 0.5
    s_x, s_w = float(x.abs().max()) / 127, float(w.abs().max()) / 127
    wq = torch.clamp(torch.round(w / s_w), -127, 127).to(torch.int8).cuda()
    q = torch.clamp(torch.round(x.float().cpu() / s_x), -127, 127).to(torch.int8).cuda()
    b = torch.randn(N, generator=g).cuda()
    r = torch.randn(M, N, generator=g).half().cuda()
    return x, q, s_x, wq, s_w, b, r


def int8_dense_bar(got, q, s_x, wq, s_w, b, r, relu=True):
    """Exact integer sums, de-quantised in float64: the reference and bar of tests/test_linear_q_gpu.py."""
    acc = q.cpu().long() @ wq.cpu().long().t()
    want = acc.double() * (s_x * s_w) + b.cpu().double() + (0 if r is None else r.cpu().double())
    want = torch.relu(want) if relu else want
    err = (got.cpu().double() - want).abs().max().item()
    assert err <= 2e-3 * max(1.0, want.abs().max().item()), err


@pytest.mark.parametrize("M", [127, 129])
@pytest.mark.parametrize("entry", ["linear_int8", "linear_int8_fused", "linear_int8_chain", "tsgemm_s8"])
def test_int8_linears_tail_rows(ctx, monkeypatch, entry, M):
    """128-row tiles; N = 136, K = 80: neither a multiple of the 128 / 64-column tile nor of the k-step (K % 16 == 0 is
    the domain).  tsgemm_s8: 160-row tiles, whole column tiles only (N = 256, K = 128)."""
    chain = fmod("int8_chain")
    mod = fmod("linear")
    if entry == "tsgemm_s8":
        M, N, K = M + 32, 256, 128
    else:
        N, K = 136, 80
    x, q, s_x, wq, s_w, b, r = int8_dense(M, N, K, M + N)
    if entry in ("linear_int8", "linear_int8_fused"):
        a = q if entry == "linear_int8" else x
        plain = wrapper_contract(monkeypatch, [mod], lambda a, wq, b, r: mod.linear_int8(a, s_x, wq, s_w, b, r, relu=True),
                                 dict(a=a, wq=wq, b=b, r=r), entries=["bevops_" + entry])[0]
    else:
        monkeypatch.setitem(chain._TS_S8, "enabled", entry == "tsgemm_s8")
        other = "linear_int8_chain" if entry == "tsgemm_s8" else "tsgemm_s8"
        plain = wrapper_contract(monkeypatch, [chain], lambda a, wq, b, r: chain.linear_int8_chain(a, s_x, wq, s_w, b, r, relu=True),
                                 dict(a=q, wq=wq, b=b, r=r), entries=["bevops_" + entry], not_entries=["bevops_" + other])[0]
    if entry == "linear_int8_fused":     # its own quantiser: x * fl(1 / s), emulated in float64 as test_linear_q_gpu.py does
        r32 = np.float32(1.0) / np.float32(s_x)
        q = torch.from_numpy(np.clip(np.rint(x.cpu().numpy().astype(np.float64) * np.float64(r32)), -127, 127).astype(np.int8))
    int8_dense_bar(plain, q, s_x, wq, s_w, b, r)


def conv_operands(B, C, H, W, Cout, k, stride, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, C, k, k, generator=g) / (k * k * C) ** 0.5).half().cuda()
    b = torch.randn(Cout, generator=g).half().cuda()
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    r = torch.randn(B, Cout, Ho, Wo, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    return x, w, b, r


# output pixels one more / one less than the 128-row tile: 3 x 43 = 129, 127 x 1; Cin = 32 (the smallest), Cout = 24 (no
# multiple of 8 x 8); stride 2 from the sizes that give the same pixel counts
CONV_CASES = [(1, 32, 3, 43, 24, 3, 1), (1, 32, 127, 1, 24, 3, 1), (1, 32, 3, 43, 24, 1, 1), (1, 32, 127, 1, 24, 1, 1),
              (1, 32, 5, 86, 24, 3, 2), (1, 32, 253, 1, 24, 3, 2), (1, 32, 6, 85, 24, 1, 2), (1, 32, 254, 2, 24, 1, 2)]


@pytest.mark.parametrize("B,C,H,W,Cout,k,stride", CONV_CASES)
def test_conv_tile_f16_tail_pixels(ctx, monkeypatch, B, C, H, W, Cout, k, stride):
    mod = fmod("conv")
    x, w, b, r = conv_operands(B, C, H, W, Cout, k, stride, H + W + k + stride)
    plain = wrapper_contract(monkeypatch, [mod], lambda x, w, b, r: mod.conv_nhwc(x, w, b, True, r, stride),
                             dict(x=x, w=w, b=b, r=r))[0]
    assert plain.shape[2] * plain.shape[3] in (127, 129)
    want = torch.relu(torch.nn.functional.conv2d(x.float(), w.float(), b.float(), stride, k // 2) + r.float())
    err = (plain.float() - want).abs()      # reference and bar of tests/test_tile_gemm_gpu.py
    assert bool((err <= 1e-3 * want.abs().clamp_min(1.0) + 2e-3).all()), float(err.max())


@pytest.mark.parametrize("entry", ["conv_tile_int8_fused", "conv_tile_int8"])
@pytest.mark.parametrize("H,W,k,stride", [(3, 43, 3, 1), (127, 1, 1, 1), (5, 86, 3, 2)])
def test_conv_tile_int8_tail_pixels(ctx, monkeypatch, entry, H, W, k, stride):
    conv = fmod("conv")
    chain = fmod("int8_chain")
    B, C, Cout = 1, 64, 24
    g = torch.Generator().manual_seed(H + W + k)
    x = torch.randn(B, C, H, W, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    w = torch.randn(Cout, C, k, k, generator=g) / (k * k * C) ** 0.5
    b = torch.randn(Cout, generator=g).cuda()
    s_x, s_w = float(x.abs().max()) / 127, float(w.abs().max()) / 127
    wq = torch.clamp(torch.round(w / s_w), -127, 127).to(torch.int8)
    taps = wq.permute(0, 2, 3, 1).contiguous().cuda()
    r32 = np.float32(1.0) / np.float32(s_x)
    q = np.clip(np.rint(x.cpu().numpy().astype(np.float64) * np.float64(r32)), -127, 127)
    acc = torch.nn.functional.conv2d(torch.from_numpy(q).double(), wq.double(), None, stride, k // 2)
    if entry == "conv_tile_int8_fused":
        r = torch.randn(acc.shape, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        plain = wrapper_contract(monkeypatch, [conv], lambda x, taps, b, r: conv.conv_int8_nhwc(x, s_x, taps, s_w, b, True, r, stride),
                                 dict(x=x, taps=taps, b=b, r=r))[0]
        want = torch.relu(acc * (s_x * s_w) + b.cpu().double().view(1, -1, 1, 1) + r.cpu().double())
    else:
        xq = torch.from_numpy(q.astype(np.int8)).cuda().contiguous(memory_format=torch.channels_last)
        plain = wrapper_contract(monkeypatch, [chain], lambda xq, taps, b: chain.conv_int8_chain_nhwc(xq, s_x, taps, s_w, b, True, stride),
                                 dict(xq=xq, taps=taps, b=b))[0]
        want = torch.relu(acc * (s_x * s_w) + b.cpu().double().view(1, -1, 1, 1))
    err = (plain.cpu().double() - want).abs().max().item()       # bar of test_conv_int8_matches_integer_reference
    assert err <= 2e-3 * max(1.0, want.abs().max().item()), err


@pytest.mark.parametrize("H,W", [(17, 15), (15, 17), (16, 33)])
def test_conv3x3_c64_tail_tiles(ctx, monkeypatch, H, W):
    """16 x 16-pixel output tiles: one more and one less in each direction.  Bit-identical to bevops_conv_tile_f16
    (its header comment), which carries the fp32 reference."""
    mod = fmod("conv")
    x, w, b, _ = conv_operands(2, 64, H, W, 64, 3, 1, H * W)
    plain = wrapper_contract(monkeypatch, [mod], lambda x, w, b: mod.conv3x3_c64(x, w, b, True), dict(x=x, w=w, b=b))[0]
    assert same_bits(plain, mod.conv_nhwc(x, w, b, True))
    want = torch.relu(torch.nn.functional.conv2d(x.float(), w.float(), b.float(), 1, 1))
    assert bool(((plain.float() - want).abs() <= 1e-3 * want.abs().clamp_min(1.0) + 2e-3).all())


@pytest.mark.parametrize("n,heads", [(31, 2), (33, 1), (129, 4)])
def test_mha_selfattn_tail_queries(ctx, monkeypatch, n, heads):
    import torch.nn.functional as TF
    mod = fmod("attention")
    g = torch.Generator().manual_seed(n + heads)
    qkv = torch.randn(n, 3, heads, 32, generator=g).half().cuda()
    plain = wrapper_contract(monkeypatch, [mod], lambda qkv: mod.self_attention_qkv(qkv), dict(qkv=qkv))[0]
    q, k, v = (qkv[:, i].float().transpose(0, 1) for i in range(3))
    want = TF.scaled_dot_product_attention(q[None], k[None], v[None])[0].transpose(0, 1).reshape(n, heads * 32)
    err = (plain.float() - want).abs()       # reference and bars of tests/test_attention_gpu.py
    assert err.max().item() <= 4e-3 * max(1.0, want.abs().max().item()) and err.mean().item() <= 3e-4


@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
@pytest.mark.parametrize("n,c,h,w", [(2, 64, 7, 9), (1, 8, 1, 1), (3, 16, 2, 5)])
def test_bias_relu_maxpool_odd_sizes(ctx, monkeypatch, n, c, h, w, int8):
    import torch.nn.functional as TF
    chain = fmod("int8_chain")
    mod = fmod("modulated_deformable_conv2d")
    g = torch.Generator().manual_seed(n + c + h + w)
    x = torch.randn(n, c, h, w, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    b = torch.randn(c, generator=g).half().cuda()
    two_pass = TF.max_pool2d(mod.bias_act_nhwc_(x.clone(memory_format=torch.channels_last), b, None, True), 3, 2, 1)
    if not int8:
        plain = wrapper_contract(monkeypatch, [mod], lambda x, b: mod.bias_relu_maxpool_nhwc(x, b), dict(x=x, b=b))[0]
        assert torch.equal(plain, two_pass)          # the reference of tests/test_epilogue_gpu.py, bit for bit
    else:
        s = 0.05
        plain = wrapper_contract(monkeypatch, [chain], lambda x, b: chain.bias_relu_maxpool_nhwc_int8(x, b, s), dict(x=x, b=b))[0]
        from test_int8_chain_gpu import _close_int8
        want = TF.max_pool2d(torch.relu(x.float() + b.float().view(1, -1, 1, 1)), 3, 2, 1)
        _close_int8(plain, torch.clamp(torch.round(want / s), -127, 127))      # reference and bar of test_stem_pool_int8


# ---- streaming passes ------------------------------------------------------------------------------------------------
def stream_case(entry, rows):
    """(modules, call, inputs, in-place names, check(outputs)) of one streaming entry on `rows` rows of its smallest
    legal width: the element count is one 8-element vector x 256 lanes more or less than whole blocks."""
    lin = fmod("linear")
    mod = fmod("modulated_deformable_conv2d")
    g = torch.Generator().manual_seed(rows)
    if entry == "bias_act_nhwc":
        x, b, r = (torch.randn(s, generator=g).half().cuda() for s in ((rows, 8), (8,), (rows, 8)))
        want = torch.relu(x.float() + b.float() + r.float())        # reference and bar of tests/test_model_gpu.py
        return [mod], lambda x, b, r: mod.bias_act_nhwc_(x, b, r, True), dict(x=x, b=b, r=r), ("x",), \
            lambda o: (o[0].float() - want).abs().max().item() <= 2e-3 * max(1.0, want.abs().max().item())
    if entry == "layer_norm":
        x, gam, bet = (torch.randn(s, generator=g).half().cuda() for s in ((rows, 64), (64,), (64,)))
        want = torch.nn.functional.layer_norm(x.float(), (64,), gam.float(), bet.float(), 1e-5)
        return [lin], lambda x, gam, bet: lin.layer_norm(x, gam, bet, 1e-5), dict(x=x, gam=gam, bet=bet), (), \
            lambda o: (o[0].float() - want).abs().max().item() <= 2e-3 * max(1.0, want.abs().max().item())
    if entry == "upsample_add_nhwc":
        a = torch.randn(1, 8, rows, 1, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        b = torch.randn(1, 8, (rows + 1) // 2, 1, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
        want = a + torch.nn.functional.interpolate(b, size=(rows, 1), mode="nearest")
        return [mod], lambda a, b: mod.upsample_add_nhwc_(a, b), dict(a=a, b=b), ("a",), lambda o: torch.equal(o[0], want)
    if entry == "feat_embed_nhwc":
        src = torch.randn(2, rows, 64, generator=g).half().cuda()
        cam, lvl = (torch.randn(2, 64, generator=g) * 0.1).half().cuda(), (torch.randn(64, generator=g) * 0.1).half().cuda()
        dst = torch.zeros(2, rows, 64, dtype=torch.half, device="cuda")
        want = src + cam[:, None, :] + lvl[None, None, :]
        return [mod], lambda src, cam, lvl, dst: mod.feat_embed_nhwc(src, cam, lvl, dst), \
            dict(src=src, cam=cam, lvl=lvl, dst=dst), ("dst",), lambda o: torch.equal(o[0], want)
    if entry == "tsa_split":
        heads, points = 8, 4
        both = torch.randn(rows, heads * 2 * points * 3, generator=g).half().cuda()
        n_off = 2 * heads * points * 2
        off = both[:, :n_off].view(1, rows, heads, 2, 1, points, 2).permute(0, 3, 1, 2, 4, 5, 6).contiguous().view(2, rows, heads, -1)
        w = both[:, n_off:].view(1, rows, heads, 2, 1, points).permute(0, 3, 1, 2, 4, 5).contiguous().view(2, rows, heads, -1)
        return [lin], lambda both: lin.tsa_split(both, heads, points), dict(both=both), (), \
            lambda o: torch.equal(o[0], off) and torch.equal(o[1], w)
    if entry == "queue_mean2":
        x = (torch.randn(2, rows, 8, generator=g) * 3).half().cuda()
        return [lin], lambda x: lin.queue_mean2(x), dict(x=x), (), lambda o: torch.equal(o[0], torch.mean(x, dim=0, keepdim=True))
    if entry == "quantize_rows":
        x = torch.randn(rows, 8, generator=g).half().cuda()
        s = float(x.abs().max()) / 127
        want = torch.clamp(torch.round(x.float().cpu() / s), -127, 127).to(torch.int8)
        return [lin], lambda x: lin.quantize_rows(x, s), dict(x=x), (), lambda o: torch.equal(o[0].cpu(), want)
    if entry == "dequantize_rows":
        q = torch.randint(-127, 128, (rows, 8), generator=g).to(torch.int8).cuda()
        return [lin], lambda q: lin.dequantize_rows(q, 0.0371), dict(q=q), (), \
            lambda o: torch.equal(o[0].cpu(), (q.cpu().float() * 0.0371).half())
    raise KeyError(entry)


STREAM_ENTRIES = ["bias_act_nhwc", "layer_norm", "upsample_add_nhwc", "feat_embed_nhwc", "tsa_split", "queue_mean2",
                  "quantize_rows", "dequantize_rows"]


@pytest.mark.parametrize("rows", [2 * 256 - 1, 2 * 256 + 1])
@pytest.mark.parametrize("entry", STREAM_ENTRIES)
def test_streaming_pass_tail_elements(ctx, monkeypatch, entry, rows):
    """One parametrised test over the streaming entries: 8-element (16-byte) vectors, 256-lane blocks; `rows` rows of
    one vector each (or of the smallest legal width) put the element count one vector above / below whole blocks.
    The in-place entries run on arena views directly.  References: the framework expressions their own tests use."""
    modules, call, inputs, inplace, check = stream_case(entry, rows)
    plain = wrapper_contract(monkeypatch, modules, call, inputs, inplace=inplace)
    assert check(plain)


# ---- tiled entries, continued: rotate, pooling, stem, the offset convolution ------------------------------------------
@pytest.mark.parametrize("variant", [0, 1], ids=["wide", "narrow"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("shape", [(9, 31, 40), (5, 7, 9)])
def test_rotate_partial_blocks(ctx, monkeypatch, oracle_mod, shape, interp, dtype, variant):
    """bevops_rotate_forward with the 16-byte stores through LDS (0) and the per-lane stores (1): partial 8-pixel runs,
    partial channel chunks, planes that are not 16-byte multiples."""
    bev, lib, L = ctx
    mod = fmod("rotate")
    C, H, W = shape
    img = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).to(dtype).cuda()
    angle, center = 17.5, (W * 0.45, H * 0.55)
    ang, ctr = torch.tensor(angle).cuda(), torch.tensor(center).cuda()
    prev = lib.bevops_rotate_set_variant(variant)
    try:
        plain = wrapper_contract(monkeypatch, [mod], lambda img, ang, ctr: mod.rotate(img, ang, ctr, interp),
                                 dict(img=img, ang=ang, ctr=ctr))[0]
    finally:
        lib.bevops_rotate_set_variant(prev)
    out = plain.float().cpu().numpy()       # reference and bars of tests/test_sampler_gpu.py::test_rotate_model_shapes
    want = oracle_mod.rotate(img.float().cpu().numpy(), angle, center, 0 if interp == "bilinear" else 1)
    if interp == "nearest":
        assert float((out != want).mean()) <= 2e-3
    elif dtype == torch.float32:
        np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4)
    else:
        assert np.abs(out - want).max() <= 1e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("interp", ["nearest", "bilinear"])
@pytest.mark.parametrize("C,H,W", [(64, 31, 45), (8, 5, 7)])
def test_rotate_hwc(ctx, monkeypatch, C, H, W, interp, dtype):
    mod = fmod("rotate")
    img = torch.randn(C, H, W, generator=torch.Generator().manual_seed(C + H)).to(dtype).cuda()
    ang, ctr = torch.tensor(-101.0).cuda(), torch.tensor([W * 0.45, H * 0.3]).cuda()
    hwc = img.permute(1, 2, 0).contiguous()
    plain = wrapper_contract(monkeypatch, [mod], lambda hwc, ang, ctr: mod.rotate_hwc(hwc, ang, ctr, interp),
                             dict(hwc=hwc, ang=ang, ctr=ctr))[0]
    assert torch.equal(plain.permute(2, 0, 1), mod.rotate(img, ang, ctr, interp))    # the reference of its own test


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("N,C,H,W,Ho,Wo", [(2, 16, 9, 11, 40, 37), (3, 8, 5, 7, 13, 6)])
def test_grid_sampler_2d_staged(ctx, monkeypatch, oracle_mod, N, C, H, W, Ho, Wo, dtype):
    """bevops_grid_sampler_2d_forward_ws on shapes where the staged path applies: the workspace is exactly
    bevops_grid_sampler_2d_workspace_size bytes at 16."""
    bev, lib, L = ctx
    mod = fmod("grid_sampler")
    g = torch.Generator().manual_seed(N + Ho)
    x = torch.randn(N, C, H, W, generator=g).to(dtype).cuda()
    grid = ((torch.rand(N, 2, Ho, Wo, generator=g) * 2 - 1) * 12).to(dtype).cuda()
    need = lib.bevops_grid_sampler_2d_workspace_size(L.torch_dtype_code(x), N, C, H, W)
    assert need > 0 and Ho * Wo >= 2 * H * W
    for mi, mode in enumerate(("bilinear", "nearest")):
        plain = wrapper_contract(monkeypatch, [mod], lambda x, grid: mod.grid_sampler(x, grid, mode, "zeros", False),
                                 dict(x=x, grid=grid), scratch_sizes=[need])[0]
        out = plain.float().cpu().numpy()
        want = oracle_mod.grid_sampler(x.float().cpu().numpy(), grid.float().cpu().numpy(), mi, 0, False)
        if mi == 1:                          # bars of tests/test_sampler_gpu.py::test_grid_sampler_2d_reference_shape
            assert float((out != want).mean()) <= 1e-3
        elif dtype == torch.float32:
            np.testing.assert_allclose(out, want, rtol=1e-5, atol=2e-5)
        else:
            assert np.abs(out - want).max() <= 1e-2 * max(1.0, np.abs(want).max() / 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C", [64, 7])
def test_bev_pool_v2_and_indirect(ctx, monkeypatch, oracle_mod, dtype, C):
    """bevops_bev_pool_v2_forward and its _indirect sibling (interval count read on the device, padded arrays) at the
    BEVDet-R50 frustum with 7 channels (no vector multiple) and 64."""
    from util_bevpool import make_indices
    mod = fmod("bev_pool_v2")
    lss = fmod("lss_prepare")
    rd, rf, rb, ist, il = make_indices(6, 59, 16, 44, 128, 128, keep=0.72, seed=0)
    gen = torch.Generator().manual_seed(0)
    depth = torch.rand(6, 59, 16, 44, generator=gen).to(dtype).cuda()
    feat = torch.randn(6, 16, 44, C, generator=gen).to(dtype).cuda()
    idx = {k: torch.from_numpy(v).cuda() for k, v in dict(rd=rd, rf=rf, rb=rb, ist=ist, il=il).items()}
    plain = wrapper_contract(monkeypatch, [mod], lambda depth, feat, rd, rf, rb, ist, il:
                             mod.bev_pool_v2(depth, feat, rd, rf, rb, ist, il, 128, 128), dict(depth=depth, feat=feat, **idx))[0]
    want = oracle_mod.bev_pool_v2(depth.float().cpu().numpy(), feat.float().cpu().numpy(), rd, rf, rb, ist, il, 128, 128)
    got = plain.float().cpu().numpy()       # bars of tests/test_bev_pool_gpu.py::test_bevdet_r50_shape
    if dtype == torch.float32:
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-5)
    else:
        assert np.abs(got - want).max() <= 1e-2 * max(1.0, np.abs(want).max())
    cap = ist.size + 37                      # padded interval arrays, as lss_voxel_prepare leaves them
    pad = lambda a, n: torch.cat([torch.from_numpy(a), torch.zeros(n - a.size, dtype=torch.int32)]).cuda()
    idx2 = dict(rd=pad(rd, rd.size + 5), rf=pad(rf, rd.size + 5), rb=pad(rb, rd.size + 5), ist=pad(ist, cap), il=pad(il, cap),
                counts=torch.tensor([rd.size, ist.size], dtype=torch.int32).cuda())
    ind = wrapper_contract(monkeypatch, [lss], lambda depth, feat, rd, rf, rb, ist, il, counts:
                           lss.bev_pool_v2_indirect(depth, feat, rd, rf, rb, ist, il, counts, 128, 128),
                           dict(depth=depth, feat=feat, **idx2))[0]
    assert same_bits(ind, plain)             # its header comment: bit-identical for equal index arrays


@pytest.mark.parametrize("int8", [False, True], ids=["f16", "int8"])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n,h,w", [(2, 8, 8), (3, 7, 2), (2, 37, 130)])
def test_stem_pack_and_conv_pool(ctx, monkeypatch, n, h, w, variant, int8):
    """bevops_stem_pack (packed exactly bevops_stem_packed_size bytes at 16) + bevops_stem_conv_pool, both pooling
    variants, fp16 and int8 output: odd heights, widths off the 60-column block and the 15-column strip, a 2 x 2 result."""
    bev, lib, L = ctx
    mod = fmod("conv")
    from test_stem_gpu import _case, _want
    x, wt, b = _case(n, h, w, seed=h * 7 + w + n)
    want = _want(x, wt, b)
    s = float(want.max()) / 150.0 if int8 else None
    lib.bevops_stem_set_variant(variant)
    try:
        plain = wrapper_contract(monkeypatch, [mod], lambda x, wt, b: mod.stem_conv_pool(x, wt, b, s), dict(x=x, wt=wt, b=b),
                                 own_scratch=[lib.bevops_stem_packed_size()], entries=["bevops_stem_pack", "bevops_stem_conv_pool"])[0]
    finally:
        lib.bevops_stem_set_variant(0)
    if int8:                                 # bars of tests/test_stem_gpu.py
        d = (plain.float() - torch.clamp(torch.round(want / s), max=127)).abs()
        assert float(d.max()) <= 1.0 and float((d == 0).float().mean()) >= 0.995
    else:
        assert bool(((plain.float() - want).abs() <= 2e-3 * want.abs() + 2e-3).all())


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("B,Cin,H,W", [(3, 256, 7, 5), (2, 64, 13, 17), (1, 128, 9, 9)])
def test_conv3x3_c32_pack_and_forward(ctx, monkeypatch, B, Cin, H, W, variant):
    """bevops_conv3x3_c32_pack_weight (exactly bevops_conv3x3_c32_packed_weight_size bytes) +
    bevops_conv3x3_c32_forward_nhwc under its four variants: 35, 221 and 81 pixels per image against 32-pixel tiles
    and 8 x 8 tiles."""
    bev, lib, L = ctx
    mod = fmod("modulated_deformable_conv2d")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Cin, H, W, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.randn(27, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half().cuda()
    b = torch.randn(27, generator=g).half().cuda()
    lib.bevops_conv3x3_c32_set_variant(variant)
    try:
        plain = wrapper_contract(monkeypatch, [mod], lambda x, w, b: mod.conv_offset_nhwc(x, w, b), dict(x=x, w=w, b=b),
                                 own_scratch=[lib.bevops_conv3x3_c32_packed_weight_size(L.F16, Cin)],
                                 entries=["bevops_conv3x3_c32_pack_weight", "bevops_conv3x3_c32_forward_nhwc"])[0]
    finally:
        lib.bevops_conv3x3_c32_set_variant(0)
    want = torch.nn.functional.conv2d(x.float(), w.float(), b.float(), 1, 1)     # bars of tests/test_mdconv_gpu.py
    assert (plain[:, :27].float() - want).abs().max().item() <= 4e-3 * max(1.0, want.abs().max().item())
    assert not plain[:, 27:].any()


# ---- entries with lent scratch, continued --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_qkv_split_keys_workspace(ctx, monkeypatch, dtype):
    """bevops_qkv_forward where few query tiles meet many keys: the keys are split across blocks and the partial
    results go through a workspace of exactly bevops_qkv_workspace_size bytes at 16."""
    bev, lib, L = ctx
    mod = fmod("multi_head_attn")
    from test_qkv_gpu import _attention64, _inputs
    B, Lq, Lkv, E = 2, 64, 40000, 32
    q, k, v = _inputs(B, Lq, Lkv, E, 1.0, dtype)
    need = lib.bevops_qkv_workspace_size(L.torch_dtype_code(q), B, Lq, Lkv, E)
    assert need > 0
    plain = wrapper_contract(monkeypatch, [mod], lambda q, k, v: mod.qkv(q, k, v), dict(q=q, k=k, v=v), scratch_sizes=[need])[0]
    want = _attention64(q, k, v)
    err = (plain.double() - want).abs()      # bars of tests/test_qkv_gpu.py
    if dtype == torch.float32:
        assert err.mean().item() <= 1e-5 and err.max().item() <= 1e-4 * max(1.0, want.abs().max().item())
    else:
        assert err.max().item() <= 4e-3 * max(1.0, want.abs().max().item())
        assert err.mean().item() <= 3e-4 * max(1.0, want.abs().mean().item())


def test_bev_nms_fixtures(ctx, monkeypatch):
    """bevops_bev_nms on the smallest rotate and circle fixture: workspace exactly bevops_bev_nms_workspace_size bytes
    at 8, the five outputs guarded."""
    bev, lib, L = ctx
    import util_nms as U
    mod = fmod("nms")
    for kind in ("rotate", "circle"):
        case = min(U.cases(kind), key=lambda c: c["boxes"].size)
        t = lambda a: torch.from_numpy(a.copy()).cuda()
        B, N = case["scores"].shape
        need = lib.bevops_bev_nms_workspace_size(B, N)
        kw = U.kwargs_of(case)
        plain = wrapper_contract(monkeypatch, [mod], lambda boxes, scores, labels, count:
                                 mod.bev_nms(boxes, scores, labels, count, **kw, padded=True),
                                 dict(boxes=t(case["boxes"]), scores=t(case["scores"]), labels=t(case["labels"]),
                                      count=t(case["count"])), ws_align=8, scratch_sizes=[max(need, 8)])
        U.check_against_fixture(case, [o.cpu().numpy() for o in plain], "bev_nms in the arena")


def test_decoders_fixtures(ctx, monkeypatch):
    """bevops_nms_free_decode and bevops_centerpoint_decode in its two-launch form (workspace exactly
    bevops_centerpoint_decode_workspace_size bytes at 8) on fixtures of the reference's own coders."""
    bev, lib, L = ctx
    import util_decode as U
    mod = fmod("decode")
    from test_decode_gpu import _exact_part
    c = min(U.nf_cases(), key=lambda c: c["cls"].numel())
    cls, box = c["cls"].cuda(), c["box"].cuda()
    plain = wrapper_contract(monkeypatch, [mod], lambda cls, box: mod.nms_free_decode(
        cls, box, c["max_num"], U.NF_RANGE, c["thr"], padded=True), dict(cls=cls, box=box))
    want = U.golden_padded(c["items"], c["max_num"])
    _exact_part(plain, want, U.NF_COPIED, "nms_free_decode in the arena")     # count, labels, copied columns, zero tail
    two = [cc for cc in U.cp_cases() if lib.bevops_centerpoint_decode_workspace_size(*cc["heat"].shape, cc["max_num"]) > 0]
    assert two, "no fixture takes the two-launch form"
    cc = min(two, key=lambda cc: cc["heat"].numel())
    maps = U.cp_args(cc, device="cuda")
    need = lib.bevops_centerpoint_decode_workspace_size(*cc["heat"].shape, cc["max_num"])
    names = ("reg", "height", "dim", "rot", "vel", "heatmap")
    inputs = {n: m for n, m in zip(names, maps[:6]) if m is not None}
    rest = maps[6:]
    plain = wrapper_contract(monkeypatch, [mod], lambda **m: mod.centerpoint_decode(
        *[m.get(n) for n in names], *rest, padded=True), inputs, ws_align=8, scratch_sizes=[need])
    _exact_part(plain, U.golden_padded(cc["items"], cc["max_num"]), U.CP_COPIED, "centerpoint_decode in the arena")


# ---- streaming passes, second half: one case per entry and count -------------------------------------------------------
def stream_case2(entry, rows):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import geometry as G
    g = torch.Generator().manual_seed(rows)
    same16 = lambda a, b: bool(((a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))).all())
    if entry == "inverse_forward":
        from test_inverse_gpu import _well_conditioned
        a64 = _well_conditioned(rows, 3, seed=rows)
        want = torch.linalg.inv(a64)

        def check(o):       # bars of tests/test_inverse_gpu.py
            err = (o[0].double().cpu() - want).abs()
            return err.mean().item() <= 1e-5 and err.max().item() <= 1e-4 * max(1.0, want.abs().max().item())
        return [fmod("inverse")], lambda a: fmod("inverse").inverse(a), dict(a=a64.float().cuda()), (), check
    if entry in ("decode_boxes", "refine_reference_points"):
        from bevformer_tensorrt_amd import bevformer as B
        from test_refine_gpu import _decode_reference
        regs = (torch.randn(1, rows, 10, generator=g) * 3).half().cuda()
        refs = (torch.rand(1, rows, 3, generator=g) * 1.4 - 0.2).half().cuda()
        if entry == "decode_boxes":
            want = _decode_reference(regs, refs)
            return [fmod("refine")], lambda regs, refs: fmod("refine").decode_boxes(regs, refs, B.PC_RANGE), dict(regs=regs, refs=refs), (), \
                lambda o: same16(o[0], want)
        want = G.refine_reference_points(regs, refs)
        return [fmod("refine")], lambda regs, refs: fmod("refine").refine_reference_points(regs, refs), dict(regs=regs, refs=refs), (), \
            lambda o: same16(o[0], want) and same16(o[1].view(rows, 2), o[0][0, :, :2].contiguous())
    if entry == "point_sampling":
        pc = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
        pillars = G.pillar_points(G.reference_points_3d(1, rows, 8, 4, device="cpu"), pc).cuda()
        l2i = G.synthetic_lidar2img((480, 800)).cuda()
        cam, mask = G.project_points(pillars, l2i, (480, 800), projection="fma")
        return [fmod("point_sampling")], lambda pillars, l2i: fmod("point_sampling").point_sampling(pillars, l2i, (480, 800), torch.float16), \
            dict(pillars=pillars, l2i=l2i), (), \
            lambda o: same16(o[0], cam.half().contiguous()) and same16(o[1], mask.half().contiguous())
    if entry == "grid_sampler_3d_forward":
        import oracle
        inp = torch.randn(1, 3, 4, 5, 6, generator=g)
        grid = (torch.rand(1, 3, rows, 1, 1, generator=g) * 2 - 1) * 12
        want = oracle.grid_sampler(inp.numpy(), grid.numpy(), 0, 0, False)
        return [fmod("grid_sampler")], lambda inp, grid: fmod("grid_sampler").grid_sampler(inp, grid, "bilinear", "zeros", False), \
            dict(inp=inp.cuda(), grid=grid.cuda()), (), \
            lambda o: bool(np.allclose(o[0].cpu().numpy(), want, rtol=1e-5, atol=2e-5))
    if entry == "image_normalize_pad":
        from oracle.image_ref import image_normalize_pad as ref
        img = torch.randint(0, 256, (2, 3, rows, 3), generator=g, dtype=torch.uint8)
        want = ref(img.numpy(), std=(58.395, 57.12, 57.375), to_rgb=True)
        return [fmod("image")], lambda img: fmod("image").image_normalize_pad(img, std=(58.395, 57.12, 57.375), to_rgb=True), \
            dict(img=img.cuda()), (), lambda o: torch.equal(o[0].cpu(), torch.from_numpy(want).half())
    if entry == "image_normalize_resize_pad":
        import util_image_scale as U
        img = U.noise(rows, 2, 9, rows)
        size = (7, rows * 4 // 5)
        want = U.normalize_resize_pad(img, size, **U.TINY_NORM)
        return [fmod("image")], lambda img: fmod("image").image_normalize_resize_pad(img, size=size, dtype=torch.float32, **U.TINY_NORM), \
            dict(img=torch.from_numpy(img).cuda()), (), \
            lambda o: np.array_equal(o[0].cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    if entry == "image_resize_crop_normalize":
        import util_image_prepare as U
        raw = U.noise(rows, 2, 20, rows)
        dims, crop = (rows * 3 // 4, 15), (3, 2, rows * 3 // 4 - 2, 14)
        canvas_want = np.stack([U.prepare(im, dims, crop, True) for im in raw])
        plan = bev.image_resize_plan(20, rows, dims, crop, "cuda")
        return [fmod("image")], lambda raw: fmod("image").image_resize_crop_normalize(raw, plan, flip=True, dtype=torch.float32, canvas=True), \
            dict(raw=torch.from_numpy(raw).cuda()), (), \
            lambda o: (np.array_equal(o[1].cpu().numpy(), canvas_want) and
                       np.array_equal(o[0].cpu().numpy().view(np.uint32), U.normalized(canvas_want).view(np.uint32)))
    raise KeyError(entry)


STREAM_ENTRIES2 = ["inverse_forward", "decode_boxes", "refine_reference_points", "point_sampling", "grid_sampler_3d_forward",
                   "image_normalize_pad", "image_normalize_resize_pad", "image_resize_crop_normalize"]


@pytest.mark.parametrize("rows", [255, 257])
@pytest.mark.parametrize("entry", STREAM_ENTRIES2)
def test_streaming_pass_tail_elements_2(ctx, monkeypatch, entry, rows):
    """The remaining one-pass entries (matrices, boxes, points, pixels per row) at counts one below and one above 256:
    their references are bit-exact restatements or the operator's fp64 / oracle bar."""
    modules, call, inputs, inplace, check = stream_case2(entry, rows)
    plain = wrapper_contract(monkeypatch, modules, call, inputs, inplace=inplace)
    assert check(plain)


def test_value_pack_planes(ctx):
    """bevops_value_pack_planes: the re-layout of a projected value tensor into exactly bevops_value_proj_packed_size
    bytes at 128 -- the planes equal, byte for byte, those bevops_value_proj_packed writes from the same GEMM
    (tests/test_sca_fused_gpu.py::test_packed_projection_planes_are_bit_identical_to_repacking_its_own_gemm)."""
    bev, lib, L = ctx
    feats, wgt, bias, sh, ref, off, w, bm, heads = projected_case()
    ncam, nk, embed = feats.shape
    nq, ch, Lv, P = off.shape[1], embed // heads, 4, 8
    need = lib.bevops_value_proj_packed_size(sh.data_ptr(), ncam, nk, heads, ch, Lv, nq, P)
    planes = need - ((ncam * nq * heads + 255) // 256) * 256
    value = bev.tsgemm(feats.view(-1, embed), wgt, bias).view(ncam, nk, heads, ch).contiguous()
    st = L.current_stream_ptr(feats.device)

    def body(arena):
        v, x, wg, b = (arena.place(t, TENSOR_ALIGN, n) for t, n in zip((value, feats, wgt, bias), ("value", "feats", "weight", "bias")))
        a = arena.carve(need, MSDA_WS_ALIGN, "packed", scratch=True)
        c = arena.carve(need, MSDA_WS_ALIGN, "projected", scratch=True)
        assert lib.bevops_value_pack_planes(v.data_ptr(), sh.data_ptr(), a.data_ptr(), need, ncam, nk, heads, ch, Lv, nq, P, st) == 0
        assert lib.bevops_value_proj_packed(x.data_ptr(), wg.data_ptr(), b.data_ptr(), sh.data_ptr(), c.data_ptr(), need,
                                            ncam, nk, heads, ch, Lv, nq, P, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(a[:planes], c[:planes])
        return [a[:planes]]
    both_poisons(4 * need + 2 * feats.numel() * 2 + 64 * MiB, body)


def test_lss_voxel_prepare(ctx, monkeypatch):
    """bevops_lss_voxel_prepare on a fixture of the reference's own view transformer: workspace exactly
    bevops_lss_voxel_prepare_workspace_size bytes at 16, the six index outputs guarded."""
    bev, lib, L = ctx
    mod = fmod("lss_prepare")
    from util_lss import check_arrays, fixture, view_for
    G_, cases = fixture()
    case = cases[0]
    vt = view_for(G_, case)
    calib = torch.from_numpy(G_[case + ".calib"]).cuda()
    frustum = vt.frustum.to("cuda", torch.float32).contiguous()
    plain = wrapper_contract(monkeypatch, [mod], lambda frustum, calib: mod.lss_voxel_prepare(
        frustum, calib, vt.grid_lower_bound, vt.grid_interval, vt.grid_size, padded=True), dict(frustum=frustum, calib=calib),
        capacity=256 * MiB, own_scratch=[lib.bevops_lss_voxel_prepare_workspace_size((calib.numel() - 9) // 24, *frustum.shape[:3])])
    rb, rd, rf, st_, ln, counts = (t.cpu().numpy() for t in plain[:6])
    n_pts, n_int = counts.tolist()
    assert np.array_equal(counts, G_[case + ".counts"])
    check_arrays(G_, case, rb[:n_pts], rd[:n_pts], rf[:n_pts], st_[:n_int], ln[:n_int])


def test_linear_bias_act_with_workspace(ctx, monkeypatch):
    """bevops_linear_bias_act (hipBLASLt) with exactly bevops_linear_workspace_size bytes lent.  NOT run-to-run
    deterministic by design: the wrapper tunes once per problem by timing (bevops_linear_tune) and the winner may be
    another algorithm in another process or after another tuning pass, with another summation order -- so the arena
    result is held to the operator's reference at its bar (tests/test_model_gpu.py: fp32 evaluation, 4e-3 relative to
    max(1, |want|), on that module's ragged shape) instead of to the ordinary call's bits; guards and poison independence are checked as everywhere."""
    bev, lib, L = ctx
    mod = fmod("linear")
    M, N, K = 1237, 256, 64
    x, w, b, r = dense_operands(M, N, K, 5)
    need = lib.bevops_linear_workspace_size()
    want = torch.relu(x.float() @ w.float().t() + b.float() + r.float())

    def close(outs):
        assert (outs[0].float() - want).abs().max().item() <= 4e-3 * max(1.0, want.abs().max().item())
    plain = wrapper_contract(monkeypatch, [mod], lambda x, w, b, r: mod.linear_bias_act(x, w, b, r, True), dict(x=x, w=w, b=b, r=r),
                             capacity=4 * need + 64 * MiB, bitwise=False, scratch_sizes=[need], verify=close)
    close(plain)


# ---- DCNv2 -----------------------------------------------------------------------------------------------------------
def not_contiguous(w):
    """The same values behind other strides: the wrapper then converts per call and takes the entry that re-lays the
    weight out inside its workspace (bevops_mdconv_forward), not the packed one."""
    return w.transpose(2, 3).contiguous().transpose(2, 3)


MDCONV_FLOAT = [(torch.float32, v, n) for v in (0, 1) for n in ("stride2", "dilated_groups", "odd_channels")] + \
               [(torch.float16, v, "stride2") for v in (0, 1, 2, 3, 4, 5)] + [(torch.float16, 0, "dilated_groups")]


@pytest.mark.parametrize("packed", [False, True], ids=["forward", "forward_packed"])
@pytest.mark.parametrize("dtype,variant,name", MDCONV_FLOAT, ids=lambda v: str(v).replace("torch.", ""))
def test_mdconv_float(ctx, monkeypatch, oracle_mod, dtype, variant, name, packed):
    """bevops_mdconv_forward / _packed, fp32 (variants 0, 1) and fp16 (0 .. 5), with the workspace of exactly
    bevops_mdconv_workspace_size bytes and the packed weight of exactly bevops_mdconv_packed_weight_size bytes the
    wrapper allocates (here: from the arena, at 16) on the ragged cases of tests/test_mdconv_gpu.py: a stride, odd
    image sizes, dilation with groups, 6 -> 10 channels."""
    bev, lib, L = ctx
    mod = fmod("modulated_deformable_conv2d")
    from test_mdconv_gpu import CASES, make
    c = CASES[name]
    x, off, mask, w, b = (t.to(dtype).cuda() for t in make(**c))
    as_given = (lambda t: t) if packed else not_contiguous
    geo = (c["stride"], c["pad"], c["dil"], c["g"], c["dg"])
    dt = L.torch_dtype_code(x)
    own = [lib.bevops_mdconv_workspace_size(dt, c["B"], c["Cin"], c["H"], c["W"], c["Cout"], c["K"], c["K"], c["stride"], c["stride"],
                                            c["pad"], c["pad"], c["dil"], c["dil"], c["g"], c["dg"])]
    if packed:
        own.append(lib.bevops_mdconv_packed_weight_size(dt, c["Cout"], c["Cin"] // c["g"], c["K"], c["K"]))
    route = ["bevops_mdconv_forward_packed", "bevops_mdconv_forward"]
    lib.bevops_mdconv_set_variant(variant)
    try:
        plain = wrapper_contract(monkeypatch, [mod], lambda x, off, mask, w, b: mod.modulated_deformable_conv2d(
            x, off, mask, as_given(w), b, *geo), dict(x=x, off=off, mask=mask, w=w, b=b), own_scratch=own,
            entries=route[:1] if packed else route[1:], not_entries=route[1:] if packed else route[:1])[0]
    finally:
        lib.bevops_mdconv_set_variant(0)
    want = oracle_mod.mdconv(*(t.float().cpu().numpy() for t in (x, off, mask, w, b)), (c["stride"],) * 2, (c["pad"],) * 2,
                             (c["dil"],) * 2, c["g"], c["dg"])
    got = plain.float().cpu().numpy()       # bars of tests/test_mdconv_gpu.py::test_mdconv_vs_oracle
    scale = max(1.0, float(np.abs(want).max()))
    if dtype == torch.float32:
        assert np.abs(got - want).max() <= 1e-4 * scale
    else:
        assert np.abs(got - want).max() <= 1e-2 * scale and np.abs(got - want).mean() <= 0.05


@pytest.mark.parametrize("packed", [False, True], ids=["forward_int8", "forward_int8_packed"])
@pytest.mark.parametrize("variant", [0, 6, 8, 9])
@pytest.mark.parametrize("name", ["stride2", "dilated_groups"])
def test_mdconv_int8(ctx, monkeypatch, oracle_mod, name, variant, packed):
    bev, lib, L = ctx
    mod = fmod("modulated_deformable_conv2d")
    from test_mdconv_gpu import CASES, _q, make
    c = CASES[name]
    x, off, mask, w, b = make(**c)
    (qx, s_x), (qo, s_o), (qm, s_m), (qw, s_w) = _q(x), _q(off), _q(mask), _q(w)
    geo = (c["stride"], c["pad"], c["dil"], c["g"], c["dg"])
    ref = oracle_mod.mdconv(x.numpy(), off.numpy(), mask.numpy(), w.numpy(), b.numpy(), (c["stride"],) * 2, (c["pad"],) * 2,
                            (c["dil"],) * 2, c["g"], c["dg"])
    s_out = float(np.abs(ref).max()) / 127.0
    wq = qw.cuda()
    own = [lib.bevops_mdconv_workspace_size(L.I8, c["B"], c["Cin"], c["H"], c["W"], c["Cout"], c["K"], c["K"], c["stride"], c["stride"],
                                            c["pad"], c["pad"], c["dil"], c["dil"], c["g"], c["dg"])]
    if packed:
        own.append(lib.bevops_mdconv_packed_weight_size(L.I8, c["Cout"], c["Cin"] // c["g"], c["K"], c["K"]))
    route = ["bevops_mdconv_forward_int8_packed", "bevops_mdconv_forward_int8"]
    if not packed:                           # a first sighting under "capture" takes the per-call entry
        monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    lib.bevops_mdconv_set_variant(variant)
    try:
        plain = wrapper_contract(monkeypatch, [mod], lambda qx, qo, qm, wq, b: mod.modulated_deformable_conv2d_int8(
            qx, qo, qm, wq, b, s_x, s_o, s_m, s_w, s_out, *geo), dict(qx=qx.cuda(), qo=qo.cuda(), qm=qm.cuda(), wq=wq, b=b.cuda()),
            own_scratch=own, entries=route[:1] if packed else route[1:], not_entries=route[1:] if packed else route[:1])[0]
    finally:
        lib.bevops_mdconv_set_variant(0)
        monkeypatch.undo()
    want = oracle_mod.mdconv_s8(qx.numpy(), s_x, qo.numpy(), s_o, qm.numpy(), s_m, qw.numpy(), s_w, b.numpy(), s_out,
                                (c["stride"],) * 2, (c["pad"],) * 2, (c["dil"],) * 2, c["g"], c["dg"]).astype(np.int32)
    d = np.abs(plain.cpu().numpy().astype(np.int32) - want)      # bar of tests/test_mdconv_gpu.py::test_mdconv_int8_vs_oracle
    assert d.max() <= 1 and (d > 0).mean() <= 0.01, (d.max(), (d > 0).mean())


@pytest.mark.parametrize("form", ["planar", "offset_mask_nhwc"])
def test_mdconv_nhwc(ctx, monkeypatch, form):
    """bevops_mdconv_forward_nhwc with bevops_mdconv_pack_weight on the smallest case of tests/test_mdconv_nhwc_gpu.py
    (17 x 19 pixels: 323, no multiple of a pixel tile), planar offsets and the raw 32-channel offset convolution output."""
    import util_dcn as U
    mod = fmod("modulated_deformable_conv2d")
    from test_mdconv_gpu import make
    from test_mdconv_nhwc_gpu import _fp16_bound, _random_om
    Bn, Cin, Cout, Hn, Wn, stride = 2, 64, 64, 17, 19, 1
    x, off, mask, w, b = (t.half() for t in make(Bn, Cin, Cout, Hn, Wn, 3, stride, 1, 1, 1, 1, seed=3, off_std=2.5))
    xc = x.cuda().contiguous(memory_format=torch.channels_last)
    bev, lib, L = ctx
    own = [lib.bevops_mdconv_packed_weight_size(L.F16, Cout, Cin, 3, 3),
           lib.bevops_mdconv_workspace_size(L.F16, Bn, Cin, Hn, Wn, Cout, 3, 3, stride, stride, 1, 1, 1, 1, 1, 1)]
    sure = dict(own_scratch=own, entries=["bevops_mdconv_pack_weight", "bevops_mdconv_forward_nhwc"])
    if form == "planar":
        plain = wrapper_contract(monkeypatch, [mod], lambda xc, off, mask, w, b: mod.modulated_deformable_conv2d_nhwc(
            xc, off, mask, w, b, stride, 1, 1, 1, 1), dict(xc=xc, off=off.cuda(), mask=mask.cuda(), w=w.cuda(), b=b.cuda()), **sure)[0]
        _fp16_bound(plain, U.dcn_ref(x, off, mask, w, b, stride, 1, 1, 1, 1))
    else:
        om = _random_om(off, Bn, Hn, Wn, torch.Generator().manual_seed(4))
        omc = om.cuda().contiguous(memory_format=torch.channels_last)
        plain = wrapper_contract(monkeypatch, [mod], lambda xc, omc, w, b: mod.modulated_deformable_conv2d_nhwc(
            xc, None, None, w, b, stride, 1, 1, 1, 1, relu=True, offset_mask_nhwc=omc), dict(xc=xc, omc=omc, w=w.cuda(), b=b.cuda()), **sure)[0]
        om_off, om_mask = U.unpack_offset_mask(om)
        _fp16_bound(plain, U.dcn_ref(x, om_off, om_mask, w, b, stride, 1, 1, 1, 1, relu=True))


@pytest.mark.parametrize("exact", [True, False])
def test_mdconv_int8_nhwc(ctx, monkeypatch, exact):
    """bevops_mdconv_forward_int8_nhwc (workspace exactly bevops_mdconv_int8_nhwc_workspace_size bytes, lent) on the
    smallest case of tests/test_int8_chain_gpu.py, against the INT8 plugin entry on the operands it quantises itself."""
    bev, lib, L = ctx
    chain = fmod("int8_chain")
    from test_int8_chain_gpu import _q
    B, Ch, H, W = 2, 128, 20, 30
    g = torch.Generator().manual_seed(B * Ch + H)
    x = torch.randint(-127, 128, (B, Ch, H, W), generator=g, dtype=torch.int8).cuda().contiguous(memory_format=torch.channels_last)
    w = torch.randint(-127, 128, (Ch, Ch, 3, 3), generator=g, dtype=torch.int8).cuda()
    bias = torch.randn(Ch, generator=g).cuda()
    om = torch.zeros(B, 32, H, W)
    om[:, :18] = torch.randn(B, 18, H, W, generator=g) * 2.0
    om[:, 18:27] = torch.randn(B, 9, H, W, generator=g) * 1.5
    om = om.half().cuda().contiguous(memory_format=torch.channels_last)
    s_in, s_off, s_mask, s_w, s_out = 0.02, 6.0 / 127, 1.0 / 127, 0.01 / (Ch * 9) ** 0.5, 0.06
    need = lib.bevops_mdconv_int8_nhwc_workspace_size()
    plain = wrapper_contract(monkeypatch, [chain], lambda x, om, w, bias: chain.modulated_deformable_conv2d_int8_nhwc(
        x, s_in, om, s_off, s_mask, w, s_w, bias, s_out, False, exact=exact), dict(x=x, om=om, w=w, bias=bias),
        scratch_sizes=[need], capacity=4 * need + 64 * MiB, own_scratch=[lib.bevops_mdconv_packed_weight_size(L.I8, Ch, Ch, 3, 3)],
        entries=["bevops_mdconv_pack_weight", "bevops_mdconv_forward_int8_nhwc"])[0]
    off_q = _q(om[:, :18].cpu(), s_off).contiguous().cuda()
    mask_q = _q(torch.sigmoid(om[:, 18:27]).cpu(), s_mask).contiguous().cuda()
    want = bev.modulated_deformable_conv2d_int8(x.contiguous(), off_q, mask_q, w, bias, s_in, s_off, s_mask, s_w, s_out, 1, 1, 1, 1, 1)
    d = (plain.float() - want.float()).abs()       # bars of test_dcn_int8_nhwc_is_the_int8_plugin_on_channels_last
    if exact:
        assert (d > 0).float().mean().item() <= 2e-3 and d.max().item() <= 3
    else:
        assert d.mean().item() <= 0.6 and d.max().item() <= 8
