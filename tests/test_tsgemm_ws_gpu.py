"""GPU tests of the weight-stationary tall-skinny GEMM (csrc/tsgemm.hip: tsgemm_ws_kernel, K <= 256) behind
bevops_tsgemm_f16, bevops_tsgemm_f16_ln and bevops_value_proj_packed: parity with the fp32 evaluation of the same fp16
operands (the bar of test_tsgemm_gpu.py), row invariance bit for bit (an output row depends on its own operands only:
what catches prefetch, buffer-ring and tile-indexing mistakes), the LayerNorm epilogue, the sampler's planes, the A/B
switch and the domain borders.  Operands are drawn once per module (same distributions as test_tsgemm_gpu.py) and
sliced; the CU count comes from the device, the tile height from the build."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

KMAX, NMAX = 256, 1024


def fp32_bar(want):
    return 1e-3 * want.abs() + 2e-3          # fp16 rounding of the result + fp32 summation-order noise


@pytest.fixture(scope="module")
def env():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    assert handle.bevops_tsgemm_set_variant(0) in (0, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tile = handle.bevops_tsgemm_tile_rows(256)
    assert tile > 0 and tile % 32 == 0
    big = cus * tile * 2 + cus * 32 + 7      # every block: three tiles, the last one a single unit; a ragged last unit
    g = torch.Generator().manual_seed(big + NMAX + KMAX)
    ops = dict(
        x=(torch.randn(big, KMAX, generator=g) * 0.5).half().cuda(),
        w=torch.randn(NMAX, KMAX, generator=g).half().cuda(),
        b=torch.randn(NMAX, generator=g).half().cuda(),
        r=torch.randn(big, NMAX, generator=g).half().cuda(),
        gam=(1 + 0.2 * torch.randn(256, generator=g)).half().cuda(),
        bet=(0.1 * torch.randn(256, generator=g)).half().cuda(),
    )
    return dict(bev=bev, L=L, handle=handle, cus=cus, tile=tile, big=big, ops=ops, cache={})


def operands(env, M, N, K):
    """x [M, K], w [N, K] (scaled 1 / sqrt(K)), bias [N], residual [M, N]: slices of the module's operands."""
    key = (N, K)
    if key not in env["cache"]:
        o = env["ops"]
        env["cache"][key] = (o["x"][:, :K].contiguous(), (o["w"][:N, :K].float() / K ** 0.5).half().contiguous(), o["b"][:N].contiguous(),
                             o["r"][:, :N].contiguous())
    x, w, b, r = env["cache"][key]
    return x[:M], w, b, r[:M]


def reference(x, w, b, r, relu):
    want = x.float() @ w.float().t()
    if b is not None:
        want = want + b.float()
    if r is not None:
        want = want + r.float()
    return torch.relu(want) if relu else want


def check_fp32(got, want, what):
    err = (got.float() - want).abs()
    assert bool((err <= fp32_bar(want)).all()), (what, err.max().item(), (err / (want.abs() + 1e-3)).max().item())


KN = [(K, N) for K in (64, 128, 192, 256) for N in (256, 512)] + [(256, 1024)]


@pytest.mark.parametrize("K,N", KN)
def test_parity_with_fp32(env, K, N):
    bev, tile = env["bev"], env["tile"]
    flags = list(itertools.product((True, False), repeat=3))
    for M in (1, 31, 32, 33, tile - 1, tile, tile + 1):
        x, w, b, r = operands(env, M, N, K)
        for has_b, has_r, relu in flags:
            got = bev.tsgemm(x, w, b if has_b else None, r if has_r else None, relu)
            check_fp32(got, reference(x, w, b if has_b else None, r if has_r else None, relu), (M, N, K, has_b, has_r, relu))
    M = env["big"]
    x, w, b, r = operands(env, M, N, K)
    base = x.float() @ w.float().t()
    for has_b, has_r, relu in ((True, True, True), (False, False, False), (True, False, True), (False, True, False)):
        want = base
        if has_b:
            want = want + b.float()
        if has_r:
            want = want + r.float()
        if relu:
            want = torch.relu(want)
        got = bev.tsgemm(x, w, b if has_b else None, r if has_r else None, relu)
        assert got.shape == (M, N)
        check_fp32(got, want, (M, N, K, has_b, has_r, relu))


def row_ranges(env, chunks):
    """(first, last + 1) row ranges around the seams of the launch on `big` rows: the first and last row of a block's
    range, the rows around a tile boundary inside it, the ragged end."""
    big, tile = env["big"], env["tile"]
    units = (big + 31) // 32
    parts = min(units, max(1, env["cus"] // chunks))
    per, extra = divmod(units, parts)
    out = {(0, 1), (big - 7, big), (big - 40, big - 30)}
    for p in (0, 1, parts // 2, parts - 1):
        ub = p * per + min(p, extra)
        ue = ub + per + (1 if p < extra else 0)
        r0, r1 = ub * 32, min(ue * 32, big)
        out.add((r0, r0 + 1))                                 # first row of the block
        out.add((r1 - 1, r1))                                 # last row of the block
        out.add((max(r1 - 2, 0), min(r1 + 3, big)))           # across the seam to the next block
        for t in (1, 2):                                      # around its tile boundaries
            if r0 + t * tile + 2 <= r1:
                out.add((r0 + t * tile - 1, r0 + t * tile + 2))
        out.add((r0 + 5, min(r0 + 5 + 2 * tile + 9, r1)))     # a run that starts inside a unit and spans tiles
    return sorted(out)


@pytest.mark.parametrize("K,N", [(256, 256), (64, 256), (256, 512), (128, 1024)])
def test_rows_do_not_depend_on_the_launch_epi0(env, K, N):
    bev = env["bev"]
    x, w, b, r = operands(env, env["big"], N, K)
    full = bev.tsgemm(x, w, b, r, True)
    for a, e in row_ranges(env, N // 256):
        part = bev.tsgemm(x[a:e], w, b, r[a:e], True)
        assert torch.equal(part, full[a:e]), (K, N, a, e, (part.float() - full[a:e].float()).abs().max().item())


@pytest.mark.parametrize("K", [64, 256])
def test_rows_do_not_depend_on_the_launch_epi2(env, K):
    bev, o = env["bev"], env["ops"]
    x, w, b, r = operands(env, env["big"], 256, K)
    full = bev.tsgemm_ln(x, w, b, r, o["gam"], o["bet"], 1e-5)
    for a, e in row_ranges(env, 1):
        part = bev.tsgemm_ln(x[a:e], w, b, r[a:e], o["gam"], o["bet"], 1e-5)
        assert torch.equal(part, full[a:e]), (K, a, e)


@pytest.mark.parametrize("K", [64, 256])
def test_layer_norm_epilogue(env, K):
    """Against the unfused pair and against fp32, with the bars of test_tsgemm_with_layer_norm_epilogue."""
    import torch.nn.functional as F
    bev, o = env["bev"], env["ops"]
    for M in (32, 37, 900, env["big"]):
        x, w, b, r = operands(env, M, 256, K)
        r = (r.float() * 2 + 0.3).half()
        got = bev.tsgemm_ln(x, w, b, r, o["gam"], o["bet"], 1e-5)
        assert got.shape == (M, 256) and got.dtype == torch.float16
        pair = bev.layer_norm(bev.tsgemm(x, w, b, r, False), o["gam"], o["bet"], 1e-5)
        d = (got.float() - pair.float()).abs()
        assert d.max().item() <= 4e-3 and d.mean().item() <= 1e-4, (M, K, d.max().item(), d.mean().item())
        y = x.float() @ w.float().t() + b.float() + r.float()
        want = F.layer_norm(y.half().float(), (256,), o["gam"].float(), o["bet"].float(), 1e-5)
        err = (got.float() - want).abs()
        assert err.max().item() <= 2e-2 and err.mean().item() <= 6e-4, (M, K, err.max().item(), err.mean().item())


def test_planes_equal_repacking_the_same_gemm(env):
    """bevops_value_proj_packed into a poisoned buffer against bevops_value_pack_planes(tsgemm(...)) on the smallest
    ragged pyramid of the sampler's tests: every byte of the planes, pads included."""
    from test_buffer_contract_gpu import HM5_SHAPES, projected_case
    bev, L, handle = env["bev"], env["L"], env["handle"]
    feats, wgt, bias, sh, _ref, _off, _w, _bm, heads = projected_case()
    ncam, nk, embed = feats.shape
    nq, P = HM5_SHAPES["other_level_sizes"]["nq"], 8
    st = L.current_stream_ptr(feats.device)
    nbytes = handle.bevops_value_proj_packed_size(sh.data_ptr(), ncam, nk, heads, 32, 4, nq, P)
    assert nbytes > 0
    a = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    b = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device="cuda")
    L.check(handle.bevops_value_proj_packed(feats.data_ptr(), wgt.data_ptr(), bias.data_ptr(), sh.data_ptr(), a.data_ptr(),
                                            nbytes, ncam, nk, heads, 32, 4, nq, P, st), "bevops_value_proj_packed")
    value = bev.tsgemm(feats.view(-1, embed), wgt, bias).view(ncam, nk, heads, 32).contiguous()
    L.check(handle.bevops_value_pack_planes(value.data_ptr(), sh.data_ptr(), b.data_ptr(), nbytes, ncam, nk, heads, 32, 4,
                                            nq, P, st), "bevops_value_pack_planes")
    torch.cuda.synchronize()
    planes = nbytes - ((ncam * nq * heads + 255) // 256) * 256
    diff = a[:planes] != b[:planes]
    assert int(diff.sum()) == 0, (int(diff.sum()), int(diff.nonzero()[0]))
    check_fp32(value.view(-1, embed), reference(feats.view(-1, embed), wgt, bias, None, False), "value_proj")


def test_old_and_new_kernel_agree_and_the_switch_restores(env):
    bev, handle = env["bev"], env["handle"]
    x, w, b, r = operands(env, env["big"], 512, 256)
    want = reference(x, w, b, r, True)
    new = bev.tsgemm(x, w, b, r, True)
    assert handle.bevops_tsgemm_tile_rows(256) == env["tile"]
    prev = handle.bevops_tsgemm_set_variant(1)
    try:
        assert prev == 0
        old_tile = handle.bevops_tsgemm_tile_rows(256)
        old = bev.tsgemm(x, w, b, r, True)
    finally:
        assert handle.bevops_tsgemm_set_variant(prev) == 1
    assert handle.bevops_tsgemm_set_variant(0) == 0
    assert old_tile != env["tile"] and handle.bevops_tsgemm_tile_rows(256) == env["tile"]
    check_fp32(new, want, "new")
    check_fp32(old, want, "old")
    assert torch.equal(bev.tsgemm(x, w, b, r, True), new)     # back on the default, and deterministic


def test_two_calls_are_bit_equal(env):
    bev, o = env["bev"], env["ops"]
    for K, N in ((256, 256), (192, 512)):
        x, w, b, r = operands(env, env["big"], N, K)
        assert torch.equal(bev.tsgemm(x, w, b, r, False), bev.tsgemm(x, w, b, r, False))
    x, w, b, r = operands(env, env["big"], 256, 256)
    assert torch.equal(bev.tsgemm_ln(x, w, b, r, o["gam"], o["bet"]), bev.tsgemm_ln(x, w, b, r, o["gam"], o["bet"]))


def test_domain_borders(env):
    bev, L = env["bev"], env["L"]
    g = torch.Generator().manual_seed(11)
    for K in (320, 512):                     # stays on the original kernel
        assert env["handle"].bevops_tsgemm_tile_rows(K) != env["tile"]
        x = (torch.randn(333, K, generator=g) * 0.5).half().cuda()
        w = (torch.randn(256, K, generator=g) / K ** 0.5).half().cuda()
        b = torch.randn(256, generator=g).half().cuda()
        check_fp32(bev.tsgemm(x, w, b, None, True), reference(x, w, b, None, True), K)
    for n, k in ((100, 128), (256, 96)):
        with pytest.raises(L.BevopsError) as e:
            bev.tsgemm(torch.zeros(64, k, dtype=torch.half, device="cuda"), torch.zeros(n, k, dtype=torch.half, device="cuda"))
        assert e.value.status == L.NOT_SUPPORTED
