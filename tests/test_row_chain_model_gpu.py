"""The row-chain launches of the BEVFormer decoder (bevformer._ROW_CHAIN: a layer's tail with its regression branch and
the next layer's in-projection, the six levels' classification branches) inside the model."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _count_row_chains(hip_ops):
    calls = {"n": 0}
    saved = hip_ops.row_chain

    def counted(*a, **k):
        calls["n"] += 1
        return saved(*a, **k)
    hip_ops.row_chain = counted
    return calls, saved


def test_decoder_layer_tail_as_a_chain_against_the_per_layer_launches():
    """One DecoderLayer at 900 queries on a 50 x 50 BEV with its regression branch and the next layer's in-projection:
    chain on against chain off, within the bars tests/test_attention_gpu.py holds a route change to."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    dev, dtype = torch.device("cuda"), torch.float16
    torch.manual_seed(4)
    layer, nxt = (B.DecoderLayer(hip_ops).to(dev, dtype).eval() for _ in range(2))
    reg = torch.nn.Sequential(torch.nn.Linear(256, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU(),
                              torch.nn.Linear(256, 10)).to(dev, dtype).eval()
    query = torch.randn(900, 1, 256, device=dev, dtype=dtype)
    qpos = torch.randn(900, 1, 256, device=dev, dtype=dtype)
    bev_embed = torch.randn(2500, 1, 256, device=dev, dtype=dtype)
    ref = torch.rand(1, 900, 1, 2, device=dev, dtype=dtype)
    shapes = torch.tensor([[50, 50]])

    def run():
        out, reg_out = torch.empty(900, 256, device=dev, dtype=dtype), torch.empty(900, 10, device=dev, dtype=dtype)
        o, r, qkv = layer(query, bev_embed, qpos, ref, shapes, tail=(reg, nxt, out, reg_out))
        if r is None:      # the per-layer route leaves the branch and the next in-projection to the caller
            r = B._mlp(hip_ops, reg, o).view(1, -1, 10)
            qkv = hip_ops.dense_auto(o.view(900, 256), nxt.self_attn.in_proj_weight, None, nxt._qkv_term(hip_ops, o, qpos), False)
        return o, r, qkv

    from bevformer_tensorrt_amd.functions.dispatch import using
    with torch.no_grad(), using(own=True):      # (the own-kernel dispatch, as inside the model's frame)
        calls, saved = _count_row_chains(hip_ops)
        try:
            on = run()
        finally:
            hip_ops.row_chain = saved
        assert calls["n"] == 1
        assert B._ROW_CHAIN["enabled"]
        B._ROW_CHAIN["enabled"] = False
        try:
            off = run()
        finally:
            B._ROW_CHAIN["enabled"] = True
    for a, b in zip(on, off):
        d = (a.float() - b.float()).abs()
        print(tuple(a.shape), "max", d.max().item(), "mean", d.mean().item())
        assert a.shape == b.shape and d.max().item() <= 2e-2 and d.mean().item() <= 1e-3


def _tiny_frames(B, G, model, dev, dtype, graph, frames=3):
    H, W = B.CONFIGS["tiny"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randn(1, 6, 3, H, W, generator=g).to(dev, dtype) for _ in range(frames)]
    r = B.FrameRunner(model, dev, dtype, graph=graph)
    got = []
    for i, img in enumerate(imgs):
        can = torch.zeros(18)
        can[0], can[1], can[-2], can[-1] = 0.4 * i, -0.15 * i, 0.02 * i, 1.1 * i
        cls, crd = r.step(img, can, l2i, "scene")
        got.append((r.prev_bev.clone(), cls.clone(), crd.clone()))
    return got


def test_tiny_frames_eager_and_graph_give_the_same_bits_with_the_chain_on():
    """BEVFormer-tiny over three frames: every layer's tail and the class head run as row chains (7 launches per frame),
    eagerly and replayed from a HIP graph with the same bits."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev, dtype = torch.device("cuda"), torch.float16
    model = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    assert B._ROW_CHAIN["enabled"]
    with torch.no_grad():
        calls, saved = _count_row_chains(hip_ops)
        try:
            eager = _tiny_frames(B, G, model, dev, dtype, False)
        finally:
            hip_ops.row_chain = saved
        assert calls["n"] == 3 * 7, calls
        graph = _tiny_frames(B, G, model, dev, dtype, True)
    for f, (a, b) in enumerate(zip(eager, graph)):
        for x, y in zip(a, b):
            assert torch.isfinite(x.float()).all() and torch.equal(x, y), f


def test_a_frame_with_the_chain_on_is_bit_reproducible():
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev, dtype = torch.device("cuda"), torch.float16
    model = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    H, W = B.CONFIGS["tiny"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    img = torch.randn(1, 6, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev, dtype)
    nq = model.bev_h * model.bev_w
    prev = (torch.randn(nq, 1, B.EMBED, generator=torch.Generator().manual_seed(2)) * 0.5).to(dev, dtype)
    can = torch.zeros(18, device=dev)
    assert B._ROW_CHAIN["enabled"]
    with torch.no_grad():
        runs = [[t.clone() for t in model(img, prev, torch.tensor(1.0, device=dev), can, l2i)] for _ in range(4)]
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert torch.equal(x, y)
