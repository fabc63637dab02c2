"""Exact routing and counting tests of the attention kernels (csrc/qkv.hip: qkv / qkv2 in fp32 and fp16, all eight head
widths, 4 and 8 waves, with and without the key split; csrc/attention.hip: self_attention_qkv) on the operands of
util_exact_attention.py: every softmax weight is exactly 0 or 1/n, n in {1, 2, 4}, so the result is the mean of named V
rows, bit for bit -- torch.equal, no tolerance.  A key that is dropped, counted twice, given to the wrong query, batch,
head or channel, or a wave / split whose share is weighed wrongly, changes an output by at least 1/8.
test_attention_exact_cpu.py proves on the CPU that exact equality is a fair demand.  The uniform-weight groups
(q = 0, one-hot V) count the keys of every channel instead: count / Lkv within 1 ulp (fp16) or 2 ulp (fp32); with a
power of two of keys (all_keys_tie) that too is exact.  q = 0 is what shows a zero K row staged past the last key: the
class codes score such a row below every class."""
import numpy as np
import pytest
import torch

import util_exact_attention as X

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s)) for s in X.QKV_SHAPES]


def _assert_equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).reshape(-1, got.shape[-1]).any(-1).nonzero().flatten()
        diff = (got.double() - want.double()).abs().max().item()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel() // got.shape[-1]} rows differ, "
                             f"first {bad[:8].tolist()}; max |diff| {diff}")


@pytest.mark.parametrize("E", X.QKV_DIMS)
@pytest.mark.parametrize("shape", X.QKV_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("dtype", X.QKV_DTYPES)
def test_qkv_routing_and_counting(dtype, shape, E):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    B, Lq, Lkv = shape
    tdt = getattr(torch, dtype)
    d = X.cached_inputs(dtype, B, Lq, Lkv, E)
    q, k, v = (torch.tensor(d[n]).to("cuda", tdt) for n in "qkv")
    want = torch.tensor(d["want"]).to(tdt).cuda()
    if shape == X.QKV_SPLIT_SHAPE:                           # the key split must not leave this test unnoticed
        nsplit = d["plan"]["nsplit"]
        assert nsplit == (3 if d["plan"]["NW"] == 8 else 6)
        need = L.load_library().bevops_qkv_workspace_size(L.torch_dtype_code(q), B, Lq, Lkv, E)
        assert need > 0 and need == nsplit * B * Lq * (E + 2) * 4
    got = bev.qkv(q, k, v)
    assert got.shape == (B, Lq, E) and got.dtype == tdt
    _assert_equal(got, want, "qkv")
    _assert_equal(bev.qkv2(q, k, v), want, "qkv2")
    # permuted, non-contiguous operands, as the module layout produces them
    qp, kp, vp = (t.transpose(0, 1).contiguous().transpose(0, 1) for t in (q, k, v))
    assert B == 1 or Lkv == 1 or not kp.is_contiguous()
    _assert_equal(bev.qkv(qp, kp, vp), want, "qkv of permuted operands")


@pytest.mark.parametrize("E", X.QKV_DIMS)
@pytest.mark.parametrize("Lkv", X.UNIFORM_LKV)
@pytest.mark.parametrize("dtype", X.QKV_DTYPES)
def test_qkv_uniform_weights_count_every_key_once(dtype, Lkv, E):
    import bevformer_tensorrt_amd as bev
    tdt = getattr(torch, dtype)
    B, Lq = X.UNIFORM_B, X.UNIFORM_LQ
    q, k, v, want, count = X.uniform_inputs(B, Lq, Lkv, E)
    if Lkv == 1541:
        assert X.plan(dtype, B, Lq, Lkv, E)["nsplit"] > 1
    got = bev.qkv(*(torch.from_numpy(t).to("cuda", tdt) for t in (q, k, v))).double().cpu().numpy()
    err = np.abs(got - want)
    bar = (1 if X.is_half(dtype) else 2) * X.ulp(want, dtype)
    # a miscounted key moves its channel by 1 / count_ch >= 1 / 97 of its value, the bar allows 2^-9 at the most
    assert count.max() <= 97 and (bar[want > 0] <= want[want > 0] * 2.0 ** -9).all()
    assert (err <= bar).all(), (np.argwhere(err > bar)[:8].tolist(), (err / np.maximum(bar, 1e-300)).max())


@pytest.fixture(scope="module")
def self_attention_cases():
    cache = {}

    def get(n, heads):
        if (n, heads) not in cache:
            d = X.cached_inputs("float16", heads, n, n, X.SELF_ATTN_DIM, "self_attention")
            qkv, want = X.pack_self_attention(d)
            cache[n, heads] = (torch.from_numpy(qkv).half().cuda(), torch.from_numpy(want).half().cuda())
        return cache[n, heads]
    return get


@pytest.mark.parametrize("heads", X.SELF_ATTN_HEADS)
@pytest.mark.parametrize("n", X.SELF_ATTN_N)
def test_self_attention_routing_and_counting(self_attention_cases, n, heads):
    import bevformer_tensorrt_amd as bev
    packed, want = self_attention_cases(n, heads)
    got = bev.self_attention_qkv(packed)
    assert got.shape == (n, heads * 32) and got.dtype == torch.float16
    _assert_equal(got, want, "self_attention_qkv")


@pytest.mark.parametrize("heads", X.SELF_ATTN_HEADS)
@pytest.mark.parametrize("n", X.SELF_ATTN_TIE_N)
def test_self_attention_all_keys_tie(n, heads):
    """q = 0: the zero K rows that attention.hip stages past n tie with the real keys, and only its `key < n` mask keeps
    them out.  n a power of two: the mean of all V rows, exactly."""
    import bevformer_tensorrt_amd as bev
    packed, want = X.pack_self_attention(X.tie_inputs(heads, n, X.SELF_ATTN_DIM))
    packed = torch.from_numpy(packed).half().cuda()
    _assert_equal(bev.self_attention_qkv(packed), torch.from_numpy(want).half().cuda(), "self_attention_qkv")
    q, k, v = (packed[:, i].transpose(0, 1) for i in range(3))
    _assert_equal(bev.qkv(q, k, v).transpose(0, 1).reshape(n, heads * 32), torch.from_numpy(want).half().cuda(), "qkv")


@pytest.mark.parametrize("heads", X.SELF_ATTN_HEADS)
@pytest.mark.parametrize("n", X.SELF_ATTN_UNIFORM_N)
def test_self_attention_uniform_weights_count_every_key_once(n, heads):
    import bevformer_tensorrt_amd as bev
    q, k, v, want, count = X.uniform_inputs(heads, n, n, X.SELF_ATTN_DIM)
    packed = np.ascontiguousarray(np.stack([q, k, v], 0).transpose(2, 0, 1, 3))          # [n, 3, heads, 32]
    got = bev.self_attention_qkv(torch.from_numpy(packed).half().cuda()).double().cpu().numpy()
    want = want.transpose(1, 0, 2).reshape(n, heads * 32)
    err, bar = np.abs(got - want), X.ulp(want, "float16")                                # 1 ulp of binary16
    # one key more or less moves a channel by 1 / (n + 1) of its value or more: at least twice the bar
    assert (bar[want > 0] <= want[want > 0] * 2.0 ** -10).all() and 2 * (n + 1) <= 2 ** 10
    assert (err <= bar).all(), (np.argwhere(err > bar)[:8].tolist(), (err / np.maximum(bar, 1e-300)).max())


@pytest.mark.parametrize("heads", X.SELF_ATTN_HEADS)
@pytest.mark.parametrize("n", X.SELF_ATTN_N)
def test_qkv_equals_self_attention_bit_for_bit(self_attention_cases, n, heads):
    import bevformer_tensorrt_amd as bev
    packed, _ = self_attention_cases(n, heads)
    q, k, v = (packed[:, i].transpose(0, 1) for i in range(3))          # [head, n, 32], permuted views
    got = bev.qkv(q, k, v).transpose(0, 1).reshape(n, heads * 32)
    _assert_equal(got, bev.self_attention_qkv(packed), "qkv on the self-attention operands")
