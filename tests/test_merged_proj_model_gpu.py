"""The merged projection launches of the BEVFormer frame (bevformer._MERGED_PROJ: one grouped launch for the six decoder
value projections of bev_embed, one destination-table launch for the six prev_bev @ Wa terms of TSA, one per layer for
SCA's sampling_offsets | attention_weights, one per decoder layer for its pair on the few-row kernel) against the per-layer
launches: BEV features, class scores and box coordinates bit for bit (torch.equal), frame by frame.

Row counts: a merged launch replaces a per-layer GEMM only where the dispatch runs that GEMM on tile_gemm / tsgemm
(M * N > 1024 * 512; below that the few-row kernel with its own summation order runs, and the merge stays off).  The
layer-level cases therefore use 56 x 56 = 3 136 queries, the smallest square grid at which every merged route -- the
192-column one included -- is taken, not a few hundred."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _count_calls(hip_ops, names):
    calls = {n: 0 for n in names}
    saved = {n: getattr(hip_ops, n) for n in names}
    for n in names:
        def counted(*a, _n=n, _f=saved[n], **k):
            calls[_n] += 1
            return _f(*a, **k)
        setattr(hip_ops, n, counted)
    return calls, saved


def _ab(fn):
    """fn() with the merged launches off, then on; the number of merged launches of the second run."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    assert B._MERGED_PROJ["enabled"]
    B._MERGED_PROJ["enabled"] = False
    try:
        off = fn()
    finally:
        B._MERGED_PROJ["enabled"] = True
    calls, saved = _count_calls(hip_ops, ("tsgemm_grouped", "tile_gemm_dst", "small_gemm_dst"))
    try:
        on = fn()
    finally:
        for n, f in saved.items():
            setattr(hip_ops, n, f)
    return off, on, calls


@pytest.mark.parametrize("graph", [False, True])
def test_tiny_frames_are_bit_identical_with_and_without_the_merged_launches(graph):
    """Three frames of one scene: the first (no history) runs the per-layer launches either way, frames two and three
    the merged ones."""
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev, dtype = torch.device("cuda"), torch.float16
    model = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    H, W = B.CONFIGS["tiny"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(0)
    imgs = [torch.randn(1, 6, 3, H, W, generator=g).to(dev, dtype) for _ in range(3)]

    def run():
        r = B.FrameRunner(model, dev, dtype, graph=graph)
        got = []
        for i, img in enumerate(imgs):
            can = torch.zeros(18)
            can[0], can[1], can[-2], can[-1] = 0.4 * i, -0.15 * i, 0.02 * i, 1.1 * i
            cls, crd = r.step(img, can, l2i, "scene")
            got.append((r.prev_bev.clone(), cls.clone(), crd.clone()))
        return got

    with torch.no_grad():
        off, on, calls = _ab(run)
    # tiny (2 500 queries): the shipped table runs the encoder's layers and the decoder's value_proj on the few-row
    # kernel, so of the merged routes only the decoder's pair is taken here (frames two and three; the base frame and
    # the layer cases below take the others)
    assert calls["tsgemm_grouped"] == 0 and calls["tile_gemm_dst"] == 0 and calls["small_gemm_dst"] >= 2 * len(model.decoder), calls
    for f, ((ba, ca, da), (bb, cb, db)) in enumerate(zip(off, on)):
        assert torch.equal(ba, bb), f
        assert torch.equal(ca, cb) and torch.equal(da, db), f


def test_base_frame_with_history_is_bit_identical():
    """Two base frames of one scene; the second runs all four merged routes (40 000 queries)."""
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev, dtype = torch.device("cuda"), torch.float16
    model = B.BEVFormer("base", seed=0).to(dev, dtype)
    H, W = B.CONFIGS["base"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    img = torch.randn(1, 6, 3, H, W, generator=torch.Generator().manual_seed(2)).to(dev, dtype)

    def run():
        r = B.FrameRunner(model, dev, dtype)
        got = []
        for i in range(2):
            can = torch.zeros(18)
            can[0], can[-1] = 0.4 * i, 1.1 * i
            cls, crd = r.step(img, can, l2i, "scene")
            got.append((r.prev_bev.clone(), cls.clone(), crd.clone()))
        return got

    with torch.no_grad():
        off, on, calls = _ab(run)
    assert calls == {"tsgemm_grouped": 1, "tile_gemm_dst": 1 + len(model.encoder), "small_gemm_dst": len(model.decoder)}, calls
    for f, ((ba, ca, da), (bb, cb, db)) in enumerate(zip(off, on)):
        assert torch.equal(ba, bb) and torch.equal(ca, cb) and torch.equal(da, db), f


NQ_SIDE = 56


def _own_kernels():
    from bevformer_tensorrt_amd.functions.linear import OWN_KERNELS

    class Ctx:
        def __enter__(self):
            self.was, OWN_KERNELS["enabled"] = OWN_KERNELS["enabled"], True

        def __exit__(self, *a):
            OWN_KERNELS["enabled"] = self.was
    return Ctx()


def test_encoder_layer_at_base_widths():
    """One BEVFormerLayer (8 heads x 32, 4 levels x 8 points, six cameras) over 3 136 queries with history: TSA's
    prev_bev term evaluated in front of the layer as the frame does, SCA's pair inside it."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    dev, dtype, nq = torch.device("cuda"), torch.float16, NQ_SIDE * NQ_SIDE
    torch.manual_seed(11)
    layer = B.BEVFormerLayer(hip_ops, 4).to(dev, dtype).eval()
    levels = [[12, 20], [6, 10], [3, 5], [2, 3]]
    nk = sum(h * w for h, w in levels)
    q, pos = (torch.randn(1, nq, 256, device=dev, dtype=dtype) for _ in range(2))
    prev = torch.randn(2, nq, 256, device=dev, dtype=dtype)
    feat = torch.randn(6, nk, 256, device=dev, dtype=dtype)
    ref_2d = torch.rand(2, nq, 1, 2, device=dev, dtype=dtype)
    ref_cam = torch.rand(6, nq, 4, 2, device=dev, dtype=dtype)
    mask = (torch.rand(6, nq, 1, device=dev) < 0.4).to(dtype)
    shapes, bev_shapes = torch.tensor(levels), torch.tensor([[NQ_SIDE, NQ_SIDE]])
    holder = torch.nn.Module()

    def run():
        terms = B._merged_prev_terms(hip_ops, holder, "_t", [layer.tsa], q, prev[0], pos)
        assert (terms is None) == (not B._MERGED_PROJ["enabled"])
        return layer(q, feat, pos, ref_2d, ref_cam, mask, shapes, bev_shapes, prev, True, None, None, None, None,
                     None if terms is None else terms[0], B._MERGED_PROJ["enabled"])

    with torch.no_grad(), _own_kernels():
        off, on, calls = _ab(run)
    assert calls == {"tsgemm_grouped": 0, "tile_gemm_dst": 2, "small_gemm_dst": 0}, calls
    assert torch.equal(off, on)


def test_decoder_layer_at_base_widths():
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    dev, dtype, nq = torch.device("cuda"), torch.float16, NQ_SIDE * NQ_SIDE
    torch.manual_seed(12)
    layer = B.DecoderLayer(hip_ops).to(dev, dtype).eval()
    query, qpos = (torch.randn(900, 1, 256, device=dev, dtype=dtype) for _ in range(2))
    bev = torch.randn(nq, 1, 256, device=dev, dtype=dtype)
    ref = torch.rand(1, 900, 1, 2, device=dev, dtype=dtype)
    shapes = torch.tensor([[NQ_SIDE, NQ_SIDE]])
    holder = torch.nn.Module()

    def run():
        values = B._merged_value_proj(hip_ops, holder, "_v", [layer.cross_attn.value_proj], bev)
        assert (values is None) == (not B._MERGED_PROJ["enabled"])
        return layer(query, bev, qpos, ref, shapes, None if values is None else values[0], B._MERGED_PROJ["enabled"])

    with torch.no_grad(), _own_kernels():
        off, on, calls = _ab(run)
    assert calls == {"tsgemm_grouped": 1, "tile_gemm_dst": 0, "small_gemm_dst": 1}, calls
    assert torch.equal(off, on)


def test_few_row_layers_keep_their_own_launches():
    """Below the few-row kernel's threshold the per-layer GEMM has another summation order: no merged launch."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    dev, dtype = torch.device("cuda"), torch.float16
    lins = [torch.nn.Linear(256, 256).to(dev, dtype) for _ in range(2)]
    x = torch.randn(300, 256, device=dev, dtype=dtype)
    with torch.no_grad(), _own_kernels():
        assert B._merged_value_proj(hip_ops, torch.nn.Module(), "_v", lins, x) is None
        assert B._merged_pair(hip_ops, torch.nn.Module(), "_p", lins[0], lins[1], x) is None
    with torch.no_grad():      # ... and not without the own-kernel dispatch either (the library's order)
        assert B._merged_value_proj(hip_ops, torch.nn.Module(), "_v", lins, torch.randn(4096, 256, device=dev, dtype=dtype)) is None
