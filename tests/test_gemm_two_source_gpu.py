"""GPU tests of the two-source GEMM (bevops_gemm2_f16: conv3 and the downsample convolution of a ResNet stage's first
bottleneck as one accumulation; csrc/tsgemm.hip tsgemm_ws2_kernel for K1 + K2 <= 256, csrc/tile_gemm.hip
tile_gemm_src2_kernel above).

  * definition, bit for bit: the call equals the single-source entry of the same kernel family (bevops_tsgemm_f16 for
    K1 + K2 <= 256, bevops_tile_gemm_f16 above) on the materialised [a1 | rows of a2] with the same stacked weight; every
    operand and the output sit between poisoned guard bands that must stay untouched;
  * predicted bits: dyadic operands (tests/util_exact_dense.py) on which every output bit follows from float64;
  * row independence, rejections without a launch, graph capture.

Operands are drawn once per module and sliced; the CU-derived row counts are those of util_exact_dense.ts_large_m."""
import itertools

import numpy as np
import pytest
import torch

import util_exact_dense as X

pytestmark = pytest.mark.gpu

KK = [(64, 64), (64, 192), (128, 256), (256, 512)]
NN = [256, 512, 1024]
GEO2 = [(2, 5, 7), (2, 6, 8), (2, 1, 1)]          # stride 2: B, H, W (odd sizes, even sizes, a one-pixel image)
K1MAX, K2MAX, NMAX = 256, 512, 1024
GUARD = 512                                        # bytes of poison on each side of every operand
POISON = 0xA5


@pytest.fixture(scope="module")
def env():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    assert handle.bevops_tsgemm_set_variant(0) in (0, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    large = X.ts_large_m(cus)
    big = max(large)
    g = torch.Generator().manual_seed(20 + big)
    ops = dict(
        a1=(torch.randn(big, K1MAX, generator=g) * 0.5).half().cuda(),
        a2=(torch.randn(big, K2MAX, generator=g) * 0.5).half().cuda(),
        w=(torch.randn(NMAX, K1MAX + K2MAX, generator=g) / 16).half().cuda(),
        b=torch.randn(NMAX, generator=g).half().cuda(),
    )
    return dict(bev=bev, L=L, handle=handle, cus=cus, large=large, big=big, ops=ops)


class Bands:
    """fp16 tensors carved out of ONE poisoned byte buffer with GUARD bytes of poison around each."""

    def __init__(self, shapes):
        self.spans, off = [], GUARD
        for shape in shapes:
            n = 2 * int(np.prod(shape))
            self.spans.append((off, n, shape))
            off += (n + GUARD + 255) // 256 * 256
        self.raw = torch.full((off + GUARD,), POISON, dtype=torch.uint8, device="cuda")

    def tensor(self, i):
        off, n, shape = self.spans[i]
        return self.raw[off:off + n].view(torch.float16).view(shape)

    def outside_untouched(self):
        mask = torch.ones(self.raw.numel(), dtype=torch.bool, device="cuda")
        for off, n, _ in self.spans:
            mask[off:off + n] = False
        return bool((self.raw[mask] == POISON).all())


def rows_of(a2, stride):
    """[B, K2, H, W] channels-last -> the [M, K2] rows the entry reads."""
    return a2.permute(0, 2, 3, 1)[:, ::stride, ::stride, :].reshape(-1, a2.shape[1]).contiguous()


def single_source(env, cat, w, b, relu):
    fn = env["bev"].tsgemm if cat.shape[1] <= 256 else env["bev"].tile_gemm
    return fn(cat, w, b, None, relu)


def run_case(env, a1, a2_rows_full, geo, stride, w, b, relu):
    """One call inside guard bands -> (got, want): a1 [M, K1]; a2_rows_full [B * H * W, K2] the pixels of the second
    source in channels-last order."""
    B, H, W = geo
    K1, K2, N = a1.shape[1], a2_rows_full.shape[1], w.shape[0]
    M = a1.shape[0]
    bands = Bands([(M, K1), (B, H, W, K2), (N, K1 + K2), (N,), (M, N)])
    t1, t2, tw, tb, out = (bands.tensor(i) for i in range(5))
    t1.copy_(a1); t2.copy_(a2_rows_full.view(B, H, W, K2)); tw.copy_(w); tb.copy_(b if b is not None else torch.zeros_like(tb))
    keep = [t.clone() for t in (t1, t2, tw, tb)]
    a2 = t2.permute(0, 3, 1, 2)
    got = env["bev"].gemm2(t1, a2, tw, tb if b is not None else None, stride, relu, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bands.outside_untouched(), ("bytes outside the operands changed", M, N, K1, K2, geo, stride)
    for t, k in zip((t1, t2, tw, tb), keep):
        assert torch.equal(t, k), "an input operand changed"
    cat = torch.cat([a1, rows_of(a2, stride)], dim=1).contiguous()
    assert cat.shape[0] == M
    return out.clone(), single_source(env, cat, w.contiguous(), b, relu)


def slices(env, M, K1, K2, N, pixels):
    o = env["ops"]
    w = torch.cat([o["w"][:N, :K1], o["w"][:N, K1MAX:K1MAX + K2]], dim=1).contiguous()
    return o["a1"][:M, :K1].contiguous(), o["a2"][:pixels, :K2].contiguous(), w, o["b"][:N].contiguous()


@pytest.mark.parametrize("N", NN)
@pytest.mark.parametrize("K1,K2", KK)
def test_definition_bit_for_bit(env, K1, K2, N):
    flags = list(itertools.product((True, False), repeat=2))
    i = 0
    for M in [1, 31, 33, 160, 161] + env["large"]:
        a1, a2r, w, b = slices(env, M, K1, K2, N, M)
        for relu, has_b in (flags if M <= 161 else [flags[i % 4]]):
            got, want = run_case(env, a1, a2r, (1, 1, M), 1, w, b if has_b else None, relu)
            assert torch.equal(got, want), ("stride 1", M, N, K1, K2, relu, has_b, (got.float() - want.float()).abs().max().item())
        i += 1
    for B, H, W in GEO2:
        M = B * ((H + 1) // 2) * ((W + 1) // 2)
        a1, a2r, w, b = slices(env, M, K1, K2, N, B * H * W)
        for relu, has_b in flags:
            got, want = run_case(env, a1, a2r, (B, H, W), 2, w, b if has_b else None, relu)
            assert torch.equal(got, want), ("stride 2", (B, H, W), N, K1, K2, relu, has_b)
    # stride 1 on a real image: the rows are the pixels
    B, H, W = 2, 5, 7
    a1, a2r, w, b = slices(env, B * H * W, K1, K2, N, B * H * W)
    got, want = run_case(env, a1, a2r, (B, H, W), 1, w, b, True)
    assert torch.equal(got, want)


@pytest.mark.parametrize("K1,K2,N", [(64, 64, 256), (64, 192, 512), (128, 256, 512), (256, 512, 1024)])
def test_predicted_bits(env, K1, K2, N):
    """Dyadic operands: every product and partial sum is exact in fp32 in any order, so float64 predicts the bits."""
    bev = env["bev"]
    for stride, (B, H, W) in ((1, (1, 1, 161)), (2, (2, 5, 7)), (2, (3, 12, 17))):
        r = X._rng("gemm2", K1, K2, N, stride, B, H, W)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        M = B * Ho * Wo
        a1 = X.gen_f16_small(r, (M, K1))
        x2 = X.gen_f16_small(r, (B, H, W, K2))
        w = X.gen_f16_small(r, (N, K1 + K2))
        bias = X.gen_bias(r, N, X.F16)
        cat = np.concatenate([a1, x2[:, ::stride, ::stride, :].reshape(M, K2)], axis=1)
        acc = X.int_matmul(cat, w)
        for relu, has_b in ((True, True), (False, False)):
            want = X.ref_epilogue(acc, 1.0, bias if has_b else None, None, relu, "fp16")
            got = bev.gemm2(torch.from_numpy(a1).cuda(), torch.from_numpy(x2).cuda().permute(0, 3, 1, 2), torch.from_numpy(w).cuda(),
                            torch.from_numpy(bias).cuda() if has_b else None, stride, relu)
            assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16)), (K1, K2, N, stride, (B, H, W), relu)


@pytest.mark.parametrize("K1,K2,N", [(64, 64, 256), (64, 192, 1024), (128, 256, 512)])
def test_rows_do_not_depend_on_the_launch(env, K1, K2, N):
    bev = env["bev"]
    M = env["large"][3]
    a1, a2r, w, b = slices(env, M, K1, K2, N, M)
    full = bev.gemm2(a1, a2r.view(1, 1, M, K2).permute(0, 3, 1, 2), w, b, 1, True)
    for a, e in ((0, 1), (5, 5 + 161), (M // 2 - 33, M // 2 + 64), (M - 17, M)):
        part = bev.gemm2(a1[a:e].contiguous(), a2r[a:e].contiguous().view(1, 1, e - a, K2).permute(0, 3, 1, 2), w, b, 1, True)
        assert torch.equal(part, full[a:e]), (K1, K2, N, a, e)
    assert torch.equal(bev.gemm2(a1, a2r.view(1, 1, M, K2).permute(0, 3, 1, 2), w, b, 1, True), full)


def test_rejections_queue_nothing(env):
    L, handle = env["L"], env["handle"]
    M, N = 70, 256
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
    a1 = torch.zeros(M, 128, dtype=torch.float16, device="cuda")
    a2 = torch.zeros(M, 128, dtype=torch.float16, device="cuda")
    w = torch.zeros(N, 256, dtype=torch.float16, device="cuda")
    st = L.current_stream_ptr(out.device)

    def call(K1=64, K2=64, B=1, H=1, W=M, s=1, p2=a2.data_ptr(), m=M):
        return handle.bevops_gemm2_f16(a1.data_ptr(), p2, w.data_ptr(), None, out.data_ptr(), m, N, K1, K2, B, H, W, s, 1, st)
    assert call() == L.SUCCESS
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    out.fill_(float("nan"))
    for kw in (dict(K1=96), dict(K2=32), dict(K2=72), dict(s=3)):
        assert call(**kw) == L.NOT_SUPPORTED, kw
    for kw in (dict(W=M + 1), dict(B=2), dict(H=2, W=M, s=2), dict(m=M - 1), dict(p2=None), dict(s=0), dict(p2=a2.data_ptr() + 2)):
        assert call(**kw) == L.BAD_PARAM, kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a rejected call wrote its output"


@pytest.mark.parametrize("K1,K2,N,stride", [(64, 64, 256, 1), (128, 256, 512, 2)])
def test_graph_capture_replays_the_eager_result(env, K1, K2, N, stride):
    bev = env["bev"]
    B, H, W = 2, 9, 13
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a1, a2r, w, b = slices(env, B * Ho * Wo, K1, K2, N, B * H * W)
    a2 = a2r.view(B, H, W, K2).permute(0, 3, 1, 2)
    eager = bev.gemm2(a1, a2, w, b, stride, True)
    out = torch.zeros_like(eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bev.gemm2(a1, a2, w, b, stride, True, out=out)      # warm-up outside capture (sets the kernel's LDS attribute)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bev.gemm2(a1, a2, w, b, stride, True, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
