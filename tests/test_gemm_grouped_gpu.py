"""GPU tests of the grouped launch of the weight-stationary tall-skinny GEMM (bevops_tsgemm_f16_grouped, csrc/tsgemm.hip):
G dense layers of 256 columns over the same rows in one launch.  The bar is bit identity (torch.equal on the fp16 bits)
with G separate calls of bevops_tsgemm_f16, for ragged row counts around the 64-row tile, every K of the kernel's domain,
with and without bias; every destination lies inside a poisoned buffer whose other bytes must stay untouched; the domain
borders are rejected without a launch.  Operands are drawn once per module and sliced."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GMAX, KMAX, MMAX = 6, 256, 200
POISON = 0x7BCD       # a finite fp16 pattern (57 760) no sum of these operands reaches


@pytest.fixture(scope="module")
def env():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    g = torch.Generator().manual_seed(GMAX * 1000 + KMAX)
    ops = dict(x=(torch.randn(MMAX, KMAX, generator=g) * 0.5).half().cuda(),
               w=(torch.randn(GMAX * 256, KMAX, generator=g) / KMAX ** 0.5).half().cuda(),
               b=torch.randn(GMAX * 256, generator=g).half().cuda())
    return dict(bev=bev, L=L, handle=handle, ops=ops, separate={})


def operands(env, M, K, G):
    o = env["ops"]
    return o["x"][:M, :K].contiguous(), o["w"][:G * 256, :K].contiguous(), o["b"][:G * 256].contiguous()


def separate(env, M, K, g, bias):
    """Layer g of the per-layer route: bevops_tsgemm_f16 on the layer's own 256 weight rows (shared between the cases)."""
    key = (M, K, g, bias)
    if key not in env["separate"]:
        x, w, b = operands(env, M, K, GMAX)
        env["separate"][key] = env["bev"].tsgemm(x, w[g * 256:(g + 1) * 256].contiguous(),
                                                 b[g * 256:(g + 1) * 256].contiguous() if bias else None)
    return env["separate"][key]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("G", [2, 3, 6])
@pytest.mark.parametrize("K", [64, 128, 256])
def test_grouped_launch_equals_the_separate_launches(env, K, G, bias):
    bev = env["bev"]
    for M in (1, 63, 64, 65, 200):
        x, w, b = operands(env, M, K, G)
        got = bev.tsgemm_grouped(x, w, b if bias else None)
        assert got.shape == (G, M, 256) and got.dtype == torch.float16
        for g in range(G):
            assert torch.equal(got[g], separate(env, M, K, g, bias)), (M, K, G, g, bias)


@pytest.mark.parametrize("M", [1, 65, 200])
def test_grouped_launch_writes_its_destinations_only(env, M):
    """Destinations group_stride apart inside a poisoned buffer: the gap between two groups, the words in front of the
    first and behind the last row stay as they were."""
    L, handle = env["L"], env["handle"]
    K, G, front, gap = 256, 3, 64, 4096 + 8
    x, w, b = operands(env, M, K, G)
    stride = M * 256 + gap
    buf = torch.full((front + G * stride,), POISON, dtype=torch.int16, device="cuda")
    st = handle.bevops_tsgemm_f16_grouped(x.data_ptr(), w.data_ptr(), b.data_ptr(), buf.data_ptr() + 2 * front, stride, M, G, K,
                                          L.current_stream_ptr(x.device))
    assert st == 0
    torch.cuda.synchronize()
    assert bool((buf[:front] == POISON).all())
    for g in range(G):
        lo = front + g * stride
        assert torch.equal(buf[lo:lo + M * 256].view(torch.float16).view(M, 256), separate(env, M, K, g, True)), g
        assert bool((buf[lo + M * 256:lo + stride] == POISON).all()), g


def test_grouped_launch_follows_the_kernel_switch(env):
    """Under the A/B variant (the original kernel for every K) the grouped entry gives that kernel's bits."""
    bev, handle = env["bev"], env["handle"]
    x, w, b = operands(env, 200, 256, 2)
    prev = handle.bevops_tsgemm_set_variant(1)
    try:
        got = bev.tsgemm_grouped(x, w, b)
        want = [bev.tsgemm(x, w[g * 256:(g + 1) * 256].contiguous(), b[g * 256:(g + 1) * 256].contiguous()) for g in range(2)]
    finally:
        handle.bevops_tsgemm_set_variant(prev)
    for g in range(2):
        assert torch.equal(got[g], want[g])


def test_rejections_return_before_any_launch(env):
    L, handle = env["L"], env["handle"]
    x, w, b = operands(env, 64, 256, 2)
    out = torch.full((2 * 64 * 256 + 16,), POISON, dtype=torch.int16, device="cuda")
    st_ptr = L.current_stream_ptr(x.device)
    ll = ctypes.c_longlong

    def call(xp=x.data_ptr(), wp=w.data_ptr(), op=out.data_ptr(), stride=64 * 256, m=64, groups=2, k=256):
        return handle.bevops_tsgemm_f16_grouped(xp, wp, b.data_ptr(), op, ll(stride), ll(m), groups, k, st_ptr)

    assert call(k=320) == L.NOT_SUPPORTED           # K > 256: outside the weight-stationary kernel
    assert call(k=512) == L.NOT_SUPPORTED
    assert call(k=96) == L.NOT_SUPPORTED            # K % 64
    assert call(stride=64 * 256 - 8) == L.BAD_PARAM       # overlapping destinations
    assert call(stride=64 * 256 + 4) == L.BAD_PARAM       # a destination off the 16-byte grid
    assert call(op=out.data_ptr() + 2) == L.BAD_PARAM     # unaligned output
    assert call(xp=None) == L.BAD_PARAM and call(wp=None) == L.BAD_PARAM and call(op=None) == L.BAD_PARAM
    assert call(m=0) == L.BAD_PARAM and call(groups=0) == L.BAD_PARAM
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- the tiled GEMM with a destination table (bevops_tile_gemm_f16_dst)
DST_N = 1152          # 64 | 192 | 256 | 512 | (128 unused) and 6 x 192


@pytest.fixture(scope="module")
def denv(env):
    g = torch.Generator().manual_seed(DST_N)
    ops = dict(x=(torch.randn(300, 256, generator=g) * 0.5).half().cuda(),
               w=(torch.randn(DST_N, 256, generator=g) / 16).half().cuda(),
               b=torch.randn(DST_N, generator=g).half().cuda(),
               r=torch.randn(300, DST_N, generator=g).half().cuda())
    return dict(env, dops=ops, want={})


def dst_want(denv, M, c0, c1, bias, res, relu=False):
    """The separate launch: bevops_tile_gemm_f16 on the range's own weight rows, dense operands."""
    key = (M, c0, c1, bias, res, relu)
    if key not in denv["want"]:
        o = denv["dops"]
        denv["want"][key] = denv["bev"].tile_gemm(o["x"][:M], o["w"][c0:c1].contiguous(), o["b"][c0:c1].contiguous() if bias else None,
                                                  o["r"][:M, c0:c1].contiguous() if res else None, relu)
    return denv["want"][key]


def run_dst(denv, M, ranges, bias=True, res=(), relu=False, n=DST_N):
    """One launch; range i = (c0, c1, out pitch, res pitch) lands in a poisoned int16 buffer with 64 words of margin on
    both sides.  Returns the buffers."""
    from bevformer_tensorrt_amd.functions.linear import _GemmDst
    L, handle, o = denv["L"], denv["handle"], denv["dops"]
    tab = (_GemmDst * len(ranges))()
    bufs, keep = [], []
    for i, (c0, c1, op, rp) in enumerate(ranges):
        buf = torch.full((64 + M * op + 64,), POISON, dtype=torch.int16, device="cuda")
        bufs.append(buf)
        tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = c0, c1, buf.data_ptr() + 128, op
        if i in res:
            r = torch.zeros(M, rp, dtype=torch.float16, device="cuda")
            r[:, :c1 - c0] = o["r"][:M, c0:c1]
            keep.append(r)
            tab[i].res, tab[i].res_pitch = r.data_ptr(), rp
    x = o["x"][:M].contiguous()
    st = handle.bevops_tile_gemm_f16_dst(x.data_ptr(), o["w"][:n].data_ptr(), o["b"].data_ptr() if bias else None,
                                         ctypes.addressof(tab), len(ranges), M, n, 256, int(relu), L.current_stream_ptr(x.device))
    assert st == 0, st
    torch.cuda.synchronize()
    return bufs


def check_dst(denv, M, ranges, bufs, bias=True, res=(), relu=False):
    for i, ((c0, c1, op, _), buf) in enumerate(zip(ranges, bufs)):
        assert bool((buf[:64] == POISON).all()) and bool((buf[64 + M * op:] == POISON).all()), (M, i)
        body = buf[64:64 + M * op].view(M, op)
        assert torch.equal(body[:, :c1 - c0].contiguous().view(torch.float16), dst_want(denv, M, c0, c1, bias, i in res, relu)), (M, i)
        assert bool((body[:, c1 - c0:] == POISON).all()), (M, i)      # between the pitched rows


@pytest.mark.parametrize("M", [1, 127, 128, 129, 300])
def test_destination_table_equals_the_separate_launches(denv, M):
    # widths 64 / 192 / 256 / 512 in one launch, columns 1024 .. 1151 in no range; dense and pitched destinations,
    # identities (ranges 1 and 3) with a pitch different from the output's
    ranges = [(0, 64, 64, 0), (64, 256, 200, 192), (256, 512, 256, 0), (512, 1024, 520, 640)]
    check_dst(denv, M, ranges, run_dst(denv, M, ranges, res=(1, 3)), res=(1, 3))
    # six layers of 192 columns, each with an identity, no bias (TSA's prev_bev @ Wa of the six encoder layers)
    ranges = [(192 * i, 192 * i + 192, 192 if i % 2 else 208, 192 + 8 * i) for i in range(6)]
    check_dst(denv, M, ranges, run_dst(denv, M, ranges, bias=False, res=range(6)), bias=False, res=range(6))


def test_destination_table_other_orders(denv):
    """Ranges listed out of column order, ReLU, and a launch whose N ends inside the last 128-column tile."""
    M = 129
    ranges = [(512, 768, 256, 0), (0, 512, 512, 0)]        # SCA: attention_weights listed first
    check_dst(denv, M, ranges, run_dst(denv, M, ranges, relu=True, n=768), relu=True)
    ranges = [(0, 128, 136, 128), (128, 192, 64, 0)]
    check_dst(denv, M, ranges, run_dst(denv, M, ranges, res=(0,), n=192), res=(0,))


def test_wrapper_returns_dense_results(denv):
    bev, o = denv["bev"], denv["dops"]
    M = 300
    outs = bev.tile_gemm_dst(o["x"], o["w"][:768].contiguous(), o["b"][:768].contiguous(), [512, 256])
    assert torch.equal(outs[0], dst_want(denv, M, 0, 512, True, False)) and torch.equal(outs[1], dst_want(denv, M, 512, 768, True, False))
    res = [o["r"][:, 192 * i:192 * i + 192] for i in range(6)]          # views with pitch 1152
    outs = bev.tile_gemm_dst(o["x"], o["w"], None, [192] * 6, res)
    for i in range(6):
        assert torch.equal(outs[i], dst_want(denv, M, 192 * i, 192 * i + 192, False, True)), i


def test_destination_table_rejections(denv):
    from bevformer_tensorrt_amd.functions.linear import _GemmDst
    L, handle, o = denv["L"], denv["handle"], denv["dops"]
    out = torch.full((2, 64 * 256 + 16), POISON, dtype=torch.int16, device="cuda")

    def call(ranges, n=512, k=256, count=None):
        tab = (_GemmDst * max(len(ranges), 1))()
        for i, (c0, c1, off, pitch) in enumerate(ranges):
            tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = c0, c1, out[i % 2].data_ptr() + off, pitch
        return handle.bevops_tile_gemm_f16_dst(o["x"].data_ptr(), o["w"].data_ptr(), None, ctypes.addressof(tab),
                                               len(ranges) if count is None else count, 64, n, k, 0, L.current_stream_ptr(out.device))

    assert call([(0, 256, 0, 256), (256, 512, 0, 256)]) == 0
    torch.cuda.synchronize()
    out.fill_(POISON)
    assert call([(0, 96, 0, 256)]) == L.BAD_PARAM                          # bound off the 64-column grid
    assert call([(32, 96, 0, 256)]) == L.BAD_PARAM
    assert call([(0, 256, 0, 256), (192, 512, 0, 320)]) == L.BAD_PARAM     # overlapping ranges
    assert call([(0, 576, 0, 576)]) == L.BAD_PARAM                         # past N
    assert call([(256, 256, 0, 256)]) == L.BAD_PARAM                       # empty
    assert call([(0, 256, 0, 192)]) == L.BAD_PARAM                         # pitch below the width
    assert call([(0, 256, 0, 260)]) == L.BAD_PARAM                         # rows off the 16-byte grid
    assert call([(0, 256, 2, 256)]) == L.BAD_PARAM                         # unaligned destination
    assert call([], count=0) == L.BAD_PARAM
    assert call([(0, 64, 0, 64)] * 1, count=9) == L.NOT_SUPPORTED          # more than 8 destinations
    assert call([(0, 64, 0, 64)], n=64) == L.NOT_SUPPORTED                 # the 64-column flavour's domain
    assert call([(0, 256, 0, 256)], k=100) == L.NOT_SUPPORTED              # K % 8
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


def test_tile_gemm_and_tsgemm_give_the_same_bits(env):
    """The model's merged launches replace per-layer GEMMs that the dispatch runs on either of the two kernels: same
    matrix instruction, k ascending, fp32 epilogue in the same order, one rounding -- the same bits, with bias and / or
    identity and ReLU, for K <= 256 (the weight-stationary tsgemm; the K > 256 kernel rotates its k order per block and
    is not part of any merged route: every merged layer has K = 256)."""
    bev = env["bev"]
    g = torch.Generator().manual_seed(7)
    for K in (64, 128, 192, 256):
        x = (torch.randn(333, K, generator=g) * 0.5).half().cuda()
        w = (torch.randn(512, K, generator=g) / K ** 0.5).half().cuda()
        b, r = torch.randn(512, generator=g).half().cuda(), torch.randn(333, 512, generator=g).half().cuda()
        for bias, res, relu in ((b, None, False), (None, r, False), (b, r, True), (None, None, False)):
            assert torch.equal(bev.tile_gemm(x, w, bias, res, relu), bev.tsgemm(x, w, bias, res, relu)), (K, bias is not None, res is not None)


# ---- the few-row GEMM with a destination table (bevops_small_gemm_f16_dst)
@pytest.mark.parametrize("M", [1, 7, 900])
def test_small_gemm_destination_table_equals_the_separate_launches(env, M):
    """Ranges 64 + 32 (the decoder's sampling_offsets | attention_weights), each with an identity whose pitch differs from
    the output's, inside poisoned buffers; then the same without identities and with a bias."""
    from bevformer_tensorrt_amd.functions.linear import _GemmDst
    bev, L, handle = env["bev"], env["L"], env["handle"]
    g = torch.Generator().manual_seed(900 + M)
    x = (torch.randn(M, 256, generator=g) * 0.5).half().cuda()
    w = (torch.randn(96, 256, generator=g) / 16).half().cuda()
    b = torch.randn(96, generator=g).half().cuda()
    r = torch.randn(M, 96, generator=g).half().cuda()
    for bias, res in ((False, True), (True, False)):
        ranges = [(0, 64, 72, 80), (64, 96, 32, 40)]
        tab = (_GemmDst * 2)()
        bufs, keep = [], []
        for i, (c0, c1, op, rp) in enumerate(ranges):
            buf = torch.full((64 + M * op + 64,), POISON, dtype=torch.int16, device="cuda")
            bufs.append(buf)
            tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = c0, c1, buf.data_ptr() + 128, op
            if res:
                ri = torch.zeros(M, rp, dtype=torch.float16, device="cuda")
                ri[:, :c1 - c0] = r[:, c0:c1]
                keep.append(ri)
                tab[i].res, tab[i].res_pitch = ri.data_ptr(), rp
        st = handle.bevops_small_gemm_f16_dst(x.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None, ctypes.addressof(tab), 2,
                                              M, 96, 256, 0, L.current_stream_ptr(x.device))
        assert st == 0, st
        torch.cuda.synchronize()
        for (c0, c1, op, _), buf in zip(ranges, bufs):
            want = bev.small_gemm(x, w[c0:c1].contiguous(), b[c0:c1].contiguous() if bias else None,
                                  r[:, c0:c1].contiguous() if res else None)
            assert bool((buf[:64] == POISON).all()) and bool((buf[64 + M * op:] == POISON).all()), (M, c0)
            body = buf[64:64 + M * op].view(M, op)
            assert torch.equal(body[:, :c1 - c0].contiguous().view(torch.float16), want), (M, c0, bias, res)
            assert bool((body[:, c1 - c0:] == POISON).all()), (M, c0)
    outs = bev.small_gemm_dst(x, w, None, [64, 32], [r[:, :64], r[:, 64:]])          # the wrapper, identities as views
    assert torch.equal(outs[0], bev.small_gemm(x, w[:64].contiguous(), None, r[:, :64].contiguous()))
    assert torch.equal(outs[1], bev.small_gemm(x, w[64:].contiguous(), None, r[:, 64:].contiguous()))


def test_small_gemm_destination_table_rejections(env):
    from bevformer_tensorrt_amd.functions.linear import _GemmDst
    L, handle = env["L"], env["handle"]
    x, w, _ = operands(env, 64, 256, 1)
    out = torch.full((2, 64 * 128 + 16), POISON, dtype=torch.int16, device="cuda")

    def call(ranges, n=96, k=256):
        tab = (_GemmDst * len(ranges))()
        for i, (c0, c1, off, pitch) in enumerate(ranges):
            tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = c0, c1, out[i % 2].data_ptr() + off, pitch
        return handle.bevops_small_gemm_f16_dst(x.data_ptr(), w.data_ptr(), None, ctypes.addressof(tab), len(ranges), 64, n, k, 0,
                                                L.current_stream_ptr(out.device))

    assert call([(32, 96, 0, 64)]) == L.BAD_PARAM                          # begins off the 64-column grid
    assert call([(0, 60, 0, 64)]) == L.BAD_PARAM                           # ends off the 8-column grid
    assert call([(0, 64, 0, 64), (0, 32, 0, 32)]) == L.BAD_PARAM           # overlapping ranges
    assert call([(0, 32, 0, 32), (0, 64, 0, 64)]) == L.BAD_PARAM
    assert call([(0, 128, 0, 128)]) == L.BAD_PARAM                         # past N
    assert call([(0, 64, 0, 48)]) == L.BAD_PARAM                           # pitch below the width
    assert call([(0, 64, 2, 64)]) == L.BAD_PARAM                           # unaligned destination
    assert call([(0, 64, 0, 64)], k=96) == L.NOT_SUPPORTED                 # K % 64
    assert call([(0, 64, 0, 64)], k=2048) == L.NOT_SUPPORTED               # K > 1024
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
