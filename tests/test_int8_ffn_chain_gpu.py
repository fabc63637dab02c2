"""The INT8 engine's FFN as an int8 chain with the block's LayerNorm in fc2's epilogue (bevformer._INT8_LN_FUSED, off by
default): fc1 writes its hidden tensor as int8 at fc2's input scale, fc2 + identity + norm is one bevops_tsgemm_s8_ln.
Module level: the exact hidden tensor, the pair bars of the fp16 fused norm, no bit changed in the float / calibrate
phases or with the switch off.  Engine level (BEVFormer-tiny, two frames): switch off is bit for bit the engine of
today, three layer_norm launches fewer per encoder layer with it on (the FFN and the two output_proj sites), and the
error against the fp16 model stays within 1.25 x the switched-off engine's."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ffn(seed, cal):
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.quantization import quantize_dense_layers
    torch.manual_seed(seed)
    ffn = B.FFN().cuda().half()
    norm = torch.nn.LayerNorm(256).cuda().half()
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(256))
        norm.bias.copy_(0.1 * torch.randn(256))
    q = quantize_dense_layers(ffn, cal)
    assert len(q) == 2 and ffn.fc1 in q and ffn.fc2 in q
    return ffn, norm, q


def test_ffn_module(monkeypatch):
    import bevformer_tensorrt_amd.functions as ops
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.functions import int8_chain as C
    from bevformer_tensorrt_amd.quantization import MinMaxCalibrator
    assert B._INT8_LN_FUSED["enabled"] is False, "the switch is off by default"
    g = torch.Generator().manual_seed(3)
    x = torch.randn(900, 256, generator=g).half().cuda()
    with torch.no_grad():
        cal = MinMaxCalibrator()
        ffn, norm, q = _ffn(5, cal)
        # float and calibrate phases: the switch changes no bit, the calibrator sees fc2's input
        for phase in ("float", "calibrate"):
            if phase == "calibrate":
                for m in q:
                    m.calibrate()
            off = ffn(x, ops, norm)
            monkeypatch.setitem(B._INT8_LN_FUSED, "enabled", True)
            on = ffn(x, ops, norm)
            monkeypatch.setitem(B._INT8_LN_FUSED, "enabled", False)
            assert torch.equal(on, off), phase
        assert cal.has(ffn.fc1.site) and cal.has(ffn.fc2.site)
        for m in q:
            m.freeze()
        assert ffn.fc1.mode == ffn.fc2.mode == "int8"

        # a second module, frozen without the switch ever touched while it exists in the int8 phase
        cal2 = MinMaxCalibrator()
        ffn2, norm2, q2 = _ffn(5, cal2)
        for m in q2:
            m.calibrate()
        ffn2(x, ops, norm2)
        for m in q2:
            m.freeze()
        before = ffn2(x, ops, norm2)
        assert torch.equal(before, ffn(x, ops, norm)), "same seed, same calibration: the two modules agree"

        seen = {}
        real_q = ffn2.fc1.forward_q
        monkeypatch.setattr(ffn2.fc1, "forward_q", lambda *a, **k: seen.setdefault("hidden", real_q(*a, **k)))
        calls = []
        monkeypatch.setattr(ops, "layer_norm", lambda *a, **k: calls.append(1) or torch.zeros(0))
        monkeypatch.setitem(B._INT8_LN_FUSED, "enabled", True)
        on = ffn2(x, ops, norm2)
        monkeypatch.undo()
        assert not calls, "the fused path launches no separate layer_norm"
        fc1, fc2 = ffn2.fc1, ffn2.fc2
        hidden = C.linear_int8_chain(x, fc1.scale_in, fc1.weight_q, fc1.scale_w, fc1.bias_f32, None, 1.0, True, torch.int8,
                                     fc2.scale_in)
        assert seen["hidden"].dtype == torch.int8 and seen["hidden"].shape == (900, 512)
        assert torch.equal(seen["hidden"], hidden)
        assert int(hidden.min()) >= 0 and int(hidden.max()) > 0                     # ReLU in fc1's epilogue
        pair = ops.layer_norm(C.linear_int8_chain(hidden, fc2.scale_in, fc2.weight_q, fc2.scale_w, fc2.bias_f32, x, 1.0,
                                                  False, torch.float16), norm2.weight, norm2.bias, norm2.eps)
        d = (on.float() - pair.float()).abs()
        print(f"fused FFN against the pair: max {d.max().item():.3e}, mean {d.mean().item():.3e}")
        assert on.shape == (900, 256) and on.dtype == torch.float16
        assert d.max().item() <= 4e-3 and d.mean().item() <= 1e-4, (d.max().item(), d.mean().item())
        # leading dimensions survive
        monkeypatch.setitem(B._INT8_LN_FUSED, "enabled", True)
        on3 = ffn2(x.view(1, 900, 256), ops, norm2)
        monkeypatch.undo()
        assert on3.shape == (1, 900, 256) and torch.equal(on3.view(900, 256), on)
        # switch off again: bit for bit the run before it was ever touched
        assert B._INT8_LN_FUSED["enabled"] is False
        assert torch.equal(ffn2(x, ops, norm2), before)


class _Count:
    def __init__(self, fn):
        self.fn, self.n = fn, 0

    def __call__(self, *a, **k):
        self.n += 1
        return self.fn(*a, **k)


def test_engine_tiny():
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    from bevformer_tensorrt_amd.quantization import build_int8_engine
    assert B._INT8_LN_FUSED["enabled"] is False
    dev, dtype = torch.device("cuda"), torch.float16
    H, W = B.CONFIGS["tiny"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(1)

    def frame(i):
        can = torch.zeros(18)
        can[0], can[1], can[-1] = 0.4 * i, -0.1 * i, 1.0 * i
        return torch.randn(1, 6, 3, H, W, generator=g).to(dev, dtype), can, l2i

    model, qops, note = build_int8_engine(B, "tiny", dev, [frame(i) for i in range(3)], calibrator="entropy_device")
    assert qops.int8_ln_fused is None, "block_norm_fused=None: the switch's value"
    layers = sum(1 for m in model.modules() if isinstance(m, B.BEVFormerLayer))
    assert layers > 0
    frames = [frame(10), frame(11)]

    def run(m, count=None):
        """Two frames on a fresh runner -> ([head outputs per frame], bev_embed of the last frame)."""
        if count is not None:
            qops.layer_norm = count
        try:
            r = B.FrameRunner(m, dev, dtype)
            outs = [tuple(t.clone() for t in r.step(*f, "s")) for f in frames]
            torch.cuda.synchronize()
            return outs, r.prev_bev.clone()
        finally:
            if count is not None:
                del qops.layer_norm

    ref = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    _, bev_ref = run(ref)
    n_off = _Count(qops.layer_norm)
    heads_off, bev_off = run(model, n_off)
    qops.int8_ln_fused = True
    n_on = _Count(qops.layer_norm)
    heads_on, bev_on = run(model, n_on)
    qops.int8_ln_fused = None
    heads_off2, bev_off2 = run(model)
    # switch off: bit for bit before and after a switched-on run
    assert torch.equal(bev_off, bev_off2)
    for a, b in zip(heads_off, heads_off2):
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    # three layer_norm launches fewer per encoder layer and frame: the FFN site and the two output_proj sites
    assert n_off.n - n_on.n == 3 * layers * len(frames), (n_off.n, n_on.n, layers)
    assert torch.isfinite(bev_on.float()).all() and all(torch.isfinite(t.float()).all() for t in heads_on[-1])
    assert not torch.equal(bev_on, bev_off), "the fused path ran"
    # the error bar: against the fp16 model, at most 1.25 x the switched-off engine's error on the same frames
    err_on = (bev_on.float() - bev_ref.float()).abs().mean().item()
    err_off = (bev_off.float() - bev_ref.float()).abs().mean().item()
    print(f"bev_embed mean |engine - fp16|: fused {err_on:.5f}, unfused {err_off:.5f}, ratio {err_on / err_off:.4f}")
    assert err_on <= 1.25 * err_off, (err_on, err_off)
    assert B._INT8_LN_FUSED["enabled"] is False
