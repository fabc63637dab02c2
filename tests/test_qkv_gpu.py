"""GPU parity of qkv / qkv2 (csrc/qkv.hip): fp32 against the reference's own outputs (tests/golden/qkv.npz) and an fp64
evaluation, fp16 against the evaluation of the same fp16 operands, the call contract (qkv2 == qkv, determinism, graph
capture, permuted inputs), the domain, the reference test's Transformer module and a cross-check with the decoder's
self-attention kernel."""
import math

import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

# (B, Lq, Lkv, E, logit gain): the reference test's q / k / v after its head split (test_multi_head_attn.py:7-51), the
# decoder's 900 queries, BEV-sized keys, more keys than attention.hip stages (a key split across blocks), wide heads,
# single elements, ragged tiles, sharp softmax
SHAPES = [(64, 960, 960, 32, 1.0), (8, 900, 900, 32, 1.0), (8, 900, 2500, 32, 1.0), (2, 64, 40000, 32, 1.0),
          (16, 1024, 1024, 64, 1.0), (8, 512, 777, 128, 1.0), (3, 1, 1, 16, 1.0), (5, 31, 33, 48, 1.0),
          (4, 100, 300, 32, 6.0), (3, 45, 77, 80, 1.0), (2, 33, 130, 96, 1.0), (2, 64, 95, 112, 1.0)]
IDS = ["x".join(map(str, s[:4])) + ("_gain%g" % s[4] if s[4] != 1.0 else "") for s in SHAPES]


def _inputs(B, Lq, Lkv, E, gain, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + B * 7 + Lq * 3 + Lkv + E)
    q = torch.randn(B, Lq, E, generator=g) * gain
    k = torch.randn(B, Lkv, E, generator=g)
    v = torch.randn(B, Lkv, E, generator=g)
    return [t.to("cuda", dtype) for t in (q, k, v)]


def _attention64(q, k, v):
    q, k, v = (t.double() for t in (q, k, v))
    return torch.softmax(q @ k.transpose(1, 2) / math.sqrt(q.shape[-1]), -1) @ v


def test_qkv_fp32_matches_reference_fixtures():
    import bevformer_tensorrt_amd as bev
    g = golden("qkv")
    for i in range(len(g["shapes"])):
        q, k, v = (torch.from_numpy(g[f"{n}{i}"]).cuda() for n in "qkv")
        want = torch.from_numpy(g[f"out{i}"]).cuda()
        got = bev.qkv(q, k, v)
        err = (got - want).abs()
        assert err.mean().item() <= 1e-5 and err.max().item() <= 1e-4 * max(1.0, want.abs().max().item()), \
            (i, err.mean().item(), err.max().item())


@pytest.mark.parametrize("B,Lq,Lkv,E,gain", SHAPES, ids=IDS)
def test_qkv_fp32_matches_fp64(B, Lq, Lkv, E, gain):
    import bevformer_tensorrt_amd as bev
    q, k, v = _inputs(B, Lq, Lkv, E, gain, torch.float32)
    got = bev.qkv(q, k, v)
    assert got.shape == (B, Lq, E) and got.dtype == torch.float32
    want = _attention64(q, k, v)
    err = (got.double() - want).abs()
    assert err.mean().item() <= 1e-5 and err.max().item() <= 1e-4 * max(1.0, want.abs().max().item()), \
        (err.mean().item(), err.max().item())


@pytest.mark.parametrize("B,Lq,Lkv,E,gain", SHAPES, ids=IDS)
def test_qkv_fp16_matches_evaluation_of_its_operands(B, Lq, Lkv, E, gain):
    import bevformer_tensorrt_amd as bev
    q, k, v = _inputs(B, Lq, Lkv, E, gain, torch.float16)
    got = bev.qkv(q, k, v)
    assert got.shape == (B, Lq, E) and got.dtype == torch.float16
    want = _attention64(q, k, v)
    err = (got.double() - want).abs()
    assert torch.isfinite(got).all()
    assert err.max().item() <= 4e-3 * max(1.0, want.abs().max().item()), err.max().item()
    assert err.mean().item() <= 3e-4 * max(1.0, want.abs().mean().item()), err.mean().item()
    if (B, Lq, Lkv, E) == (64, 960, 960, 32):        # the reference test's fp16 bar (test_multi_head_attn.py:132)
        assert err.mean().item() <= 1e-4, err.mean().item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,Lq,Lkv,E", [(8, 900, 900, 32), (2, 64, 40000, 32), (5, 31, 33, 48)])
def test_qkv_call_contract(B, Lq, Lkv, E, dtype):
    import bevformer_tensorrt_amd as bev
    q, k, v = _inputs(B, Lq, Lkv, E, 1.0, dtype, seed=1)
    a = bev.qkv(q, k, v)
    assert torch.equal(bev.qkv2(q, k, v), a)                 # the half2 plugin name: same operation
    assert torch.equal(bev.qkv(q, k, v), a)                  # run to run
    # permuted operands, as the module layout produces them: view(-1, B, E).permute(1, 0, 2)
    qp, kp, vp = (t.transpose(0, 1).contiguous().transpose(0, 1) for t in (q, k, v))
    assert not qp.is_contiguous()
    assert torch.equal(bev.qkv(qp, kp, vp), a)
    # capture + replay == eager
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bev.qkv(q, k, v)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = bev.qkv(q, k, v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)


def test_qkv_domain():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt, device="cuda")   # noqa: E731
    for E in (24, 256, 8):
        with pytest.raises(L.BevopsError) as e:
            bev.qkv(z(2, 8, E), z(2, 8, E), z(2, 8, E))
        assert e.value.status == L.NOT_SUPPORTED
    with pytest.raises(L.BevopsError) as e:
        bev.qkv(z(2, 8, 32, dt=torch.int8), z(2, 8, 32, dt=torch.int8), z(2, 8, 32, dt=torch.int8))
    assert e.value.status == L.NOT_SUPPORTED
    assert bev.qkv(z(0, 8, 32), z(0, 5, 32), z(0, 5, 32)).shape == (0, 8, 32)
    assert bev.qkv2(z(2, 0, 32), z(2, 5, 32), z(2, 5, 32)).shape == (2, 0, 32)
    with pytest.raises(ValueError):
        bev.qkv(z(2, 8, 32), z(2, 0, 32), z(2, 0, 32))


class _Transformer(torch.nn.Module):
    """The reference test's module (test_multi_head_attn.py:15-51): q / k / v / out projections around `attn`."""

    def __init__(self, attn, embed_dim=256, num_heads=8):
        super().__init__()
        self.embed_dim, self.num_heads, self.attn = embed_dim, num_heads, attn
        self.q_proj = torch.nn.Linear(embed_dim, embed_dim)
        self.k_proj = torch.nn.Linear(embed_dim, embed_dim)
        self.v_proj = torch.nn.Linear(embed_dim, embed_dim)
        self.out_proj = torch.nn.Linear(embed_dim, embed_dim)

    def forward(self, query, key, value):
        bs, hd = query.shape[1], self.embed_dim // self.num_heads
        q, k, v = (p(x).view(-1, bs * self.num_heads, hd).permute(1, 0, 2)
                   for p, x in ((self.q_proj, query), (self.k_proj, key), (self.v_proj, value)))
        out = self.attn(q, k, v).permute(1, 0, 2).reshape(-1, self.embed_dim)
        return self.out_proj(out).view(-1, bs, self.embed_dim)


def _torch_attention(q, k, v):          # functions/multi_head_attn.py:13-15
    q = q / math.sqrt(q.shape[-1])
    return torch.matmul(q, k.permute(0, 2, 1)).softmax(-1) @ v


@pytest.mark.parametrize("dtype,bar", [(torch.float32, 1e-5), (torch.float16, 1e-4)])
def test_transformer_module_matches_torch_attention(dtype, bar):
    import bevformer_tensorrt_amd as bev
    torch.manual_seed(0)
    ours = _Transformer(bev.TRT_FUNCTIONS.get("qkv")).cuda().to(dtype).eval()
    ref = _Transformer(_torch_attention).cuda().to(dtype).eval()
    ref.load_state_dict(ours.state_dict())
    x = [torch.randn(960, 8, 256, device="cuda", dtype=dtype) for _ in range(3)]   # test_multi_head_attn.py:7-10
    with torch.no_grad():
        a, b = ours(*x), ref(*x)
    assert a.shape == (960, 8, 256)
    assert (a.float() - b.float()).abs().mean().item() <= bar


def test_qkv_agrees_with_decoder_self_attention():
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(3)
    packed = torch.randn(900, 3, 8, 32, generator=g).half().cuda()     # [query, q/k/v, head, 32]
    want = bev.self_attention_qkv(packed)                                # [900, 8 * 32]
    q, k, v = (packed[:, i].transpose(0, 1) for i in range(3))          # [head, query, 32], permuted views
    got = bev.qkv(q, k, v).transpose(0, 1).reshape(900, 256)
    err = (got.float() - want.float()).abs()
    assert err.max().item() <= 4e-3 * max(1.0, want.float().abs().max().item()) and err.mean().item() <= 3e-4
