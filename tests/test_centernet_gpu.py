"""centernet.CenterNet on the GPU: the fast path (channels-last fp16 on this package's kernels) against the fp32 plain
path (library statements) on the same state dict, run-to-run and eager-to-replay reproducibility, the absence of library
convolutions / pooling / interpolation from the fast path, the packed head output under `get_bboxes`, and the rebuild of
the packed / merged operands when a weight changes -- never inside a capture.

Images: [1, 3, 32, 32] (every stage goes down to 1 x 1; the neck's DCN packs see 1 x 1, 2 x 2 and 4 x 4 maps) and
[2, 3, 64, 96]."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = ((1, 3, 32, 32), (2, 3, 64, 96))
NAMES = ("center_heatmap_preds", "wh_preds", "offset_preds")


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def nets():
    """One state dict in three models: fp16 (fast path), fp32 and fp16 on an operator set WITHOUT the fast entries (plain
    path); the images; the plain fp32 outputs, computed once."""
    import types
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.centernet import CenterNet
    fast = CenterNet(seed=0).cuda().half()
    plain_ops = types.SimpleNamespace(modulated_deformable_conv2d=fn.modulated_deformable_conv2d)
    ref32, plain16 = CenterNet(seed=1, ops=plain_ops).cuda(), CenterNet(seed=2, ops=plain_ops).cuda().half()
    sd = {k: v.float() for k, v in fast.state_dict().items()}       # the fp16 weights, exactly, in every model
    ref32.load_state_dict(sd)
    plain16.load_state_dict(sd)
    g = torch.Generator().manual_seed(11)
    images = {s: torch.randn(s, generator=g).cuda() for s in SHAPES}
    ref = {s: tuple(o.clone() for o in ref32(images[s])) for s in SHAPES}
    return dict(fast=fast, ref32=ref32, plain16=plain16, images=images, ref=ref)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fast_path_against_the_fp32_plain_path(nets, shape):
    img = nets["images"][shape]
    B, _, H, W = shape
    got = nets["fast"](img.half())
    p16 = nets["plain16"](img.half())
    for name, c, g, p, r in zip(NAMES, (80, 2, 2), got, p16, nets["ref"][shape]):
        assert g.shape == (B, c, H // 4, W // 4) and g.dtype == torch.float16 and r.dtype == torch.float32
        scale = max(1.0, float(r.abs().max()))
        err, err16 = float((g.float() - r).abs().max()), float((p.float() - r).abs().max())
        print(f"{shape} {name}: |ref|max {float(r.abs().max()):.4f}, fast path err {err:.3e}, "
              f"plain fp16 path err {err16:.3e} (bar {3e-2 * scale:.3e})")
        assert float(r.max() - r.min()) > 1e-3, f"{name} is a constant"
        assert err <= 3e-2 * scale, name
    assert float(got[0].min()) >= 0.0 and float(got[0].max()) <= 1.0        # the heat map is returned after the sigmoid


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_two_runs_and_the_replay_give_equal_bits(nets, shape):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    from bevformer_tensorrt_amd.functions.decode2d import centernet_decode
    model, img = nets["fast"], nets["images"][shape].half()
    a = [o.clone() for o in model(img)]
    b = model(img)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    cfg = model.cfg["test_cfg"]
    dec = centernet_decode(*b, cfg["topk"], shape[2:], cfg["local_maximum_kernel"], padded=True)
    runner = CenterNetRunner(model, *shape[:1], *shape[2:])
    for _ in range(2):
        out = runner.step(img)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, runner.head_outputs):
        assert torch.equal(_bits(x), _bits(y)), name
    assert len(out) == 4 and out[0].shape == (shape[0], cfg["topk"], 4) and out[3].dtype == torch.int32
    for name, x, y in zip(("boxes", "scores", "labels", "count"), dec, out):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert int(out[3].min()) == min(cfg["topk"], 80 * (shape[2] // 4) * (shape[3] // 4))


class _Counter:
    """Monkey-patch probes: counts the calls of torch.nn.functional's convolution, pooling and interpolation entries."""
    NAMES = ("conv2d", "conv_transpose2d", "max_pool2d", "interpolate")

    def __init__(self, monkeypatch):
        self.counts = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(F, name, self._wrap(name, getattr(F, name)))

    def _wrap(self, name, inner):
        def probe(*args, **kwargs):
            self.counts[name] += 1
            return inner(*args, **kwargs)
        return probe


def test_no_library_convolution_on_the_fast_path(nets, monkeypatch):
    from bevformer_tensorrt_amd.functions import conv as C
    shape = SHAPES[1]
    img = nets["images"][shape]
    nets["fast"](img.half())                          # (warm: packed and merged operands built)
    misses = list(C.CONV_MISSES)
    counter = _Counter(monkeypatch)
    nets["fast"](img.half())
    torch.cuda.synchronize()
    print("fast :", counter.counts)
    assert counter.counts == dict(conv2d=0, conv_transpose2d=0, max_pool2d=0, interpolate=0)
    assert C.CONV_MISSES == misses
    nets["plain16"](img.half())
    torch.cuda.synchronize()
    print("plain:", counter.counts)
    # 1 stem + 16 block convolutions + 3 downsamples + 3 offset convolutions + 6 head convolutions; 3 deconvolutions; 1 pool
    assert counter.counts["conv2d"] >= 29 and counter.counts["conv_transpose2d"] == 3 and counter.counts["max_pool2d"] == 1


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_packed_head_outputs_decode_in_place(nets, shape):
    from bevformer_tensorrt_amd.postprocess import centernet_get_bboxes
    model = nets["fast"]
    outs = model(nets["images"][shape].half())
    ptr = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == ptr for o in outs)          # three slices of one packed tensor
    assert outs[0].stride(1) == 1 and outs[0].stride(3) == 88 and outs[1].data_ptr() == outs[0].data_ptr() + 2 * 80
    B, _, H, W = shape
    metas = [dict(batch_input_shape=(H, W), border=(1.0, H - 1.0, 2.0, W - 2.0), scale_factor=[0.5, 0.5, 0.5, 0.5])
             for _ in range(B)]
    got = model.get_bboxes(outs, metas, rescale=True)
    want = centernet_get_bboxes(*(o.contiguous() for o in outs), metas, rescale=True, topk=100, local_maximum_kernel=3)
    assert len(got) == B
    for (gb, gl), (wb, wl) in zip(got, want):
        assert gb.shape == (100, 5) and gl.dtype == torch.int64
        assert torch.equal(gb.view(torch.int32), wb.view(torch.int32)) and torch.equal(gl, wl)


def test_capture_guard_and_weight_reload():
    from bevformer_tensorrt_amd.centernet import CenterNet
    from bevformer_tensorrt_amd.functions.deconv import deconv_packed_weight
    model = CenterNet(seed=3).cuda().half()
    img = torch.randn(SHAPES[0], generator=torch.Generator().manual_seed(5)).cuda().half()
    scratch = torch.zeros(8, device="cuda")
    ups = [u.weight for u in model.neck.deconv]
    assert model.heads_merged(build=False) is None and all(deconv_packed_weight(w, build=False) is None for w in ups)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)                                               # raises before it launches anything
        with pytest.raises(RuntimeError):
            model.prepare()
    del graph
    assert model.heads_merged(build=False) is None and all(deconv_packed_weight(w, build=False) is None for w in ups)
    # after an eager call the capture succeeds and replays the eager bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [o.clone() for o in model(img)]
    torch.cuda.current_stream().wait_stream(s)
    merged0, packed0 = model.heads_merged(build=False), [deconv_packed_weight(w, build=False) for w in ups]
    assert merged0 is not None and all(p is not None for p in packed0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = model(img)
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, outs, eager):
        assert torch.equal(_bits(a), _bits(b)), n
    del graph, outs
    # new weights: the wh branch's final convolution becomes the constant 0.5; every other operand keeps its cached copy
    with torch.no_grad():
        model.heads["wh"][1].weight.zero_()
        model.heads["wh"][1].bias.fill_(0.5)
    assert model.heads_merged(build=False) is None                   # stale
    assert all(deconv_packed_weight(w, build=False) is p for w, p in zip(ups, packed0))
    new = model(img)
    assert model.heads_merged(build=False) is not merged0
    assert bool((new[1] == 0.5).all())
    for i in (0, 2):
        assert torch.equal(_bits(new[i]), _bits(eager[i])), NAMES[i]
    new = [o.clone() for o in new]
    # the last deconvolution's weight doubles: its packed copy is rebuilt (a stale one would give the old bits)
    with torch.no_grad():
        model.neck.deconv[2].weight.mul_(2.0)
    assert deconv_packed_weight(ups[2], build=False) is None
    assert deconv_packed_weight(ups[0], build=False) is packed0[0] and model.heads_merged(build=False) is not None
    doubled = model(img)
    assert deconv_packed_weight(ups[2], build=False) is not packed0[2]
    assert not torch.equal(_bits(doubled[2]), _bits(new[2])) and not torch.equal(_bits(doubled[0]), _bits(new[0]))
