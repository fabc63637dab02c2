"""bevops_tsgemm_s8_ln (tsgemm_s8_kernel<2> of csrc/tsgemm.hip: the persistent int8 GEMM with the block's LayerNorm in its
epilogue) against the float64 reference of tests/util_int8_ln.py -- pre-norm binary16 bits predicted exactly on dyadic
operands, the norm in float64, the two conditions of util_int8_ln.check -- on every k-step count, every kloop<G>, a second
pass of a block's unit loop and ragged last units; against the unfused pair on ordinary scales; its rejections; the
buffer contract; graph capture."""
import numpy as np
import pytest
import torch

import util_exact_dense as X
import util_int8_ln as U
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

MiB = 1 << 20


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(c, o, g, b):
    from bevformer_tensorrt_amd.functions import linear_int8_ln
    sw = o["s_w"] if np.isscalar(o["s_w"]) else _dev(o["s_w"])
    out = linear_int8_ln(_dev(o["a"]), o["s_a"], _dev(o["w"]), sw, _dev(o["bias"]), _dev(o["res"]), o["s_res"], _dev(g),
                         _dev(b), U.EPS)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(c):
    o = X.make_ops(c)
    g, b = U.ln_params(c)
    want = U.reference(U.pre_norm(c, o), g, b)
    U.check(_run(c, o, g, b), want, c["id"])


@pytest.mark.parametrize("c", U.small_cases(), ids=lambda c: c["id"])
def test_small_row_counts(c):
    _check(c)


@pytest.mark.parametrize("j", range(X.TS_LARGE))
def test_every_unit_count_and_a_second_pass(j):
    """Row counts computed from the CU count, the partition asserted BEFORE the launch (as test_tsgemm_s8_exact_gpu.py):
    every kloop<G>, a second pass of a block's unit loop -- the values a thread kept from half 0 of pass 1 must not reach
    pass 2 -- and a ragged last unit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = U.large_case(j, cus)
    assert c["M"] % 32 != 0
    passes = X.ts_block_passes(c["M"], cus)
    assert passes == X.ts_expected_partition(cus)[j], (cus, c["M"], sorted(passes))
    _check(c)


def _ordinary(M, K, seed, res_kind):
    """Operands with ordinary (non-dyadic) scales, as tests/test_buffer_contract_gpu.py builds them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(256, K, generator=g) / K ** 0.5
    s_x, s_w = float(x.abs().max()) / 127, float(w.abs().max()) / 127
    q = torch.clamp(torch.round(x / s_x), -127, 127).to(torch.int8).cuda()
    wq = torch.clamp(torch.round(w / s_w), -127, 127).to(torch.int8).cuda()
    b = torch.randn(256, generator=g).cuda()
    r, s_r = None, 1.0
    if res_kind == "fp16":
        r = (torch.randn(M, 256, generator=g) * 2 + 0.3).half().cuda()
    elif res_kind == "int8":
        r, s_r = torch.randint(-127, 128, (M, 256), generator=g, dtype=torch.int8).cuda(), 0.021
    gam = (1 + 0.2 * torch.randn(256, generator=g)).half().cuda()
    bet = (0.1 * torch.randn(256, generator=g)).half().cuda()
    return q, s_x, wq, s_w, b, r, s_r, gam, bet


PAIR_SHAPES = [(161, 256, "fp16"), (900, 512, "int8"), (None, 128, "fp16")]


@pytest.mark.parametrize("M,K,res_kind", PAIR_SHAPES)
def test_against_the_unfused_pair(monkeypatch, M, K, res_kind):
    """linear_int8_ln against layer_norm(linear_int8_chain(..., out fp16)) on bevops_tsgemm_s8: the same binary16 sums,
    so only the last bit of the normalisation may differ -- the bars of test_tsgemm_with_layer_norm_epilogue."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import int8_chain as C
    if M is None:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        M = 32 * (5 * cus + cus // 2) - 15
    q, s_x, wq, s_w, b, r, s_r, gam, bet = _ordinary(M, K, M + K, res_kind)
    monkeypatch.setitem(C._TS_S8, "enabled", True)
    got = C.linear_int8_ln(q, s_x, wq, s_w, b, r, s_r, gam, bet, 1e-5)
    assert got.shape == (M, 256) and got.dtype == torch.float16
    pre = C.linear_int8_chain(q, s_x, wq, s_w, b, r, s_r, False, torch.float16)
    pair = bev.layer_norm(pre, gam, bet, 1e-5)
    d = (got.float() - pair.float()).abs()
    print(f"{M} x 256 x {K}: max {d.max().item():.3e}, mean {d.mean().item():.3e}")
    assert d.max().item() <= 4e-3 and d.mean().item() <= 1e-4, (d.max().item(), d.mean().item())
    if M % 4 == 0:      # 3-d operands keep their leading dimensions
        got3 = C.linear_int8_ln(q.view(4, M // 4, K), s_x, wq, s_w, b, r.view(4, M // 4, 256), s_r, gam, bet, 1e-5)
        assert got3.shape == (4, M // 4, 256) and torch.equal(got3.view(M, 256), got)


def test_rejections_on_the_device():
    from bevformer_tensorrt_amd.functions import linear_int8_ln
    from bevformer_tensorrt_amd.utils import lib as L
    lib = L.load_library()
    dev = "cuda"
    a = torch.zeros(64, 512, dtype=torch.int8, device=dev)
    gam, bet = torch.ones(512, dtype=torch.half, device=dev), torch.zeros(512, dtype=torch.half, device=dev)
    for n, k in ((512, 128), (256, 192), (256, 64)):
        w = torch.zeros(n, k, dtype=torch.int8, device=dev)
        with pytest.raises(L.BevopsError) as e:
            linear_int8_ln(a[:, :k].contiguous(), 0.1, w, 0.1, None, None, 1.0, gam[:n], bet[:n])
        assert e.value.status == L.NOT_SUPPORTED, (n, k)
    w = torch.zeros(256, 128, dtype=torch.int8, device=dev)
    a = a[:, :128].contiguous()
    out = torch.empty(64 * 256 + 8, dtype=torch.half, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    import ctypes
    f = ctypes.c_float

    def call(ln_w=gam.data_ptr(), eps=1e-5, o=out.data_ptr()):
        return lib.bevops_tsgemm_s8_ln(a.data_ptr(), f(0.1), w.data_ptr(), None, f(0.1), None, None, L.F16, f(1.0), ln_w,
                                       bet.data_ptr(), f(eps), o, 64, 256, 128, st)
    assert call(ln_w=None) == L.BAD_PARAM
    assert call(eps=-1.0) == L.BAD_PARAM
    assert call(o=out.data_ptr() + 8) == L.BAD_PARAM
    assert call() == L.SUCCESS
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", [33, 161])
def test_buffer_contract(M):
    """Operands and output in a guarded arena at exactly their sizes and alignments: guards intact, equal bits under the
    NaN poison and the finite poison, equal to the ordinary call.  The entry takes no workspace."""
    from bevformer_tensorrt_amd.functions import int8_chain as C
    from bevformer_tensorrt_amd.utils import lib as L
    import ctypes
    lib = L.load_library()
    K = 256
    q, s_x, wq, s_w, b, r, s_r, gam, bet = _ordinary(M, K, 7 * M, "fp16")
    plain = C.linear_int8_ln(q, s_x, wq, s_w, b, r, s_r, gam, bet, 1e-5)
    torch.cuda.synchronize()
    f = ctypes.c_float
    runs = []
    for poison in POISONS:
        arena = Arena(8 * MiB, poison)
        pq, pw, pr = arena.place(q, 16, "a_q"), arena.place(wq, 16, "w_q"), arena.place(r, 16, "identity")
        pb = arena.place(b, 4, "bias")
        pg, pbe = arena.place(gam, 16, "ln_weight"), arena.place(bet, 16, "ln_bias")
        out = arena.empty((M, 256), torch.float16, 16, "out")
        st = lib.bevops_tsgemm_s8_ln(pq.data_ptr(), f(s_x), pw.data_ptr(), None, f(s_w), pb.data_ptr(), pr.data_ptr(), L.F16,
                                     f(1.0), pg.data_ptr(), pbe.data_ptr(), f(1e-5), out.data_ptr(), M, 256, K,
                                     torch.cuda.current_stream().cuda_stream)
        assert st == L.SUCCESS
        arena.check()
        for name, t, src in (("a_q", pq, q), ("w_q", pw, wq), ("identity", pr, r), ("ln_weight", pg, gam)):
            assert torch.equal(t, src), f"{name} was written"
        runs.append(out.clone())
        del arena
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16)), "the result depends on bytes never written"
    assert torch.equal(runs[0].view(torch.int16), plain.view(torch.int16))
    assert bool(torch.isfinite(runs[0]).all())


def test_graph_capture():
    """One call at M = 161 captured on one stream and replayed twice: equal bits, equal to the eager call."""
    from bevformer_tensorrt_amd.functions import int8_chain as C
    M, K = 161, 384
    q, s_x, wq, s_w, b, r, s_r, gam, bet = _ordinary(M, K, 99, "int8")
    eager = C.linear_int8_ln(q, s_x, wq, s_w, b, r, s_r, gam, bet, 1e-5)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C.linear_int8_ln(q, s_x, wq, s_w, b, r, s_r, gam, bet, 1e-5)      # warm-up on the capture stream
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = C.linear_int8_ln(q, s_x, wq, s_w, b, r, s_r, gam, bet, 1e-5)
    torch.cuda.current_stream().wait_stream(s)
    replays = []
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert torch.equal(replays[0].view(torch.int16), replays[1].view(torch.int16))
    assert torch.equal(replays[0].view(torch.int16), eager.view(torch.int16))
