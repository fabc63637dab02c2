"""GPU: layout handling of the dense wrappers that share one operand preparation (functions/linear.py: _operands).  A
call on a strided x (a [:, ::2] slice), a strided residual and a caller-provided `out` must return, bit for bit, what
the same call on contiguous copies returns -- at the smallest shapes with a ragged last tile -- and M == 0 must return an
empty tensor of the right shape without reaching the library.  The values themselves are checked against float64 by the
exact tests of each kernel (test_tsgemm_gpu, test_tile_gemm_exact_gpu, test_small_gemm_gpu, ...); this pins the layout."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    import bevformer_tensorrt_amd.functions as f
    return f


def _half(shape, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 0.5).half().to(dev)


def _strided(t):
    """t's values as a [:, ::2] slice of a matrix twice as wide (not contiguous)"""
    wide = torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=t.device)
    wide[:, ::2] = t
    v = wide[:, ::2]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def _pitched(t):
    """t's values as the left half of a matrix twice as wide (unit column stride, row pitch 2 * width)"""
    wide = torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


F16_CASES = [("tsgemm", 33, 256, 64), ("tsgemm", 65, 256, 320), ("tile_gemm", 129, 72, 8), ("small_gemm", 33, 72, 64),
             ("linear_bias_act", 33, 256, 64)]


@pytest.mark.parametrize("name,M,N,K", F16_CASES)
def test_f16_wrappers_strided_equals_contiguous(name, M, N, K, monkeypatch):
    monkeypatch.setenv("BEVOPS_LINEAR_TUNE", "0")     # linear_bias_act: no blocking algorithm search for one call
    fn = getattr(_ops(), name)
    x, w, b, r = _half((M, K), 1), _half((N, K), 2), _half((N,), 3), _half((M, N), 4)
    want = fn(x, w, b, r, True)
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
    got = fn(_strided(x), w, b, _strided(r), True, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == want.shape == (M, N)
    assert torch.equal(got, want)
    # leading dimensions come back, and a transposed (non-contiguous) weight is the same weight
    got3 = fn(_strided(x).unsqueeze(0), w.t().contiguous().t(), b, r.unsqueeze(0), True)
    assert got3.shape == (1, M, N) and torch.equal(got3[0], want)


def test_tsgemm_ln_strided_equals_contiguous():
    f = _ops()
    M, N, K = 33, 256, 64
    x, w, b, r = _half((M, K), 1), _half((N, K), 2), _half((N,), 3), _half((M, N), 4)
    g, be = _half((N,), 5), _half((N,), 6)
    want = f.tsgemm_ln(x, w, b, r, g, be, 1e-5)
    got = f.tsgemm_ln(_strided(x), w, b, _strided(r), g, be, 1e-5)
    assert got.shape == (M, N) and torch.equal(got, want)


def test_tsgemm_grouped_strided_equals_contiguous():
    f = _ops()
    M, G, K = 33, 2, 64
    x, w, b = _half((M, K), 1), _half((G * 256, K), 2), _half((G * 256,), 3)
    want = f.tsgemm_grouped(x, w, b)
    out = torch.full((G, M, 256), float("nan"), dtype=torch.float16, device="cuda")
    got = f.tsgemm_grouped(_strided(x), w, b, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, want)


@pytest.mark.parametrize("name,M,widths,K", [("tile_gemm_dst", 129, [64, 64], 64), ("small_gemm_dst", 33, [64, 8], 64)])
def test_dst_wrappers_strided_equals_contiguous(name, M, widths, K):
    fn = getattr(_ops(), name)
    N = sum(widths)
    x, w, b = _half((M, K), 1), _half((N, K), 2), _half((N,), 3)
    res = [_half((M, n), 4 + i) for i, n in enumerate(widths)]
    want = fn(x, w, b, widths, res, True)
    outs = [_pitched(torch.full((M, n), float("nan"), dtype=torch.float16, device="cuda")) for n in widths]
    got = fn(_strided(x), w, b, widths, [_pitched(r) for r in res], True, outs=outs)
    assert len(got) == len(want) == len(widths)
    for g, o, wnt in zip(got, outs, want):
        assert g.data_ptr() == o.data_ptr() and torch.equal(g, wnt)


def _int8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-127, 128, shape, generator=g, dtype=torch.int8).cuda()


def test_int8_wrappers_strided_equals_contiguous():
    f = _ops()
    M, N, K = 33, 256, 128
    a, w, r = _int8((M, K), 1), _int8((N, K), 2), _half((M, N), 4)
    b = _half((N,), 3).float()
    ws = (torch.rand(N, generator=torch.Generator().manual_seed(5)) * 0.01 + 0.001).cuda()
    g, be = _half((N,), 6), _half((N,), 7)
    ah = a.half()
    calls = [
        ("linear_int8", a, lambda a_, r_: f.linear_int8(a_, 0.02, w, ws, b, r_, True)),
        ("linear_int8_fused", ah, lambda a_, r_: f.linear_int8(a_, 0.02, w, 0.01, b, r_, True)),
        ("linear_int8_chain", a, lambda a_, r_: f.linear_int8_chain(a_, 0.02, w, ws, b, r_, 1.0, True)),
        ("linear_int8_chain_f16", ah, lambda a_, r_: f.linear_int8_chain(a_, 0.02, w, ws, b, r_, 1.0, True)),
        ("linear_int8_chain_out8", a, lambda a_, r_: f.linear_int8_chain(a_, 0.02, w, 0.01, b, r_, 1.0, True, torch.int8, 0.05)),
        ("linear_int8_ln", a, lambda a_, r_: f.linear_int8_ln(a_, 0.02, w, ws, b, r_, 1.0, g, be, 1e-5)),
    ]
    for name, operand, fn in calls:
        want = fn(operand, r)
        got = fn(_strided(operand), _strided(r))
        assert got.shape == (M, N) and got.dtype == want.dtype, name
        assert torch.equal(got, want), name


def test_empty_rows_return_without_a_launch(monkeypatch):
    f = _ops()
    from bevformer_tensorrt_amd.utils import lib as _lib

    def no_library():
        raise AssertionError("M == 0 reached the library")

    monkeypatch.setattr(_lib, "load_library", no_library)
    N, K = 256, 128
    x, w, b = _half((2, 0, K), 1), _half((N, K), 2), _half((N,), 3)
    r = _half((2, 0, N), 4)
    for name in ("tsgemm", "tile_gemm", "small_gemm", "linear_bias_act"):
        out = getattr(f, name)(x, w, b, r, True)
        assert out.shape == (2, 0, N) and out.dtype == torch.float16 and out.is_cuda, name
    assert f.tsgemm_ln(x, w, b, r, b, b).shape == (2, 0, N)
    assert f.tsgemm_grouped(x, w, b).shape == (1, 0, 256)
    for name, widths in (("tile_gemm_dst", [128, 128]), ("small_gemm_dst", [192, 64])):
        outs = getattr(f, name)(x, w, b, widths)
        assert [tuple(o.shape) for o in outs] == [(0, n) for n in widths], name
    a, wq = _int8((2, 0, K), 1), _int8((N, K), 2)
    assert f.linear_int8(a, 0.02, wq, 0.01, b.float(), r).shape == (2, 0, N)
    assert f.linear_int8_chain(a, 0.02, wq, 0.01, b.float(), r, out_dtype=torch.int8).dtype == torch.int8
    assert f.linear_int8_chain(a, 0.02, wq, 0.01, b.float(), r).shape == (2, 0, N)
    assert f.linear_int8_ln(a, 0.02, wq, 0.01, b.float(), r, 1.0, b, b).shape == (2, 0, N)
