"""yolox.YOLOX on the GPU: the fast path (channel slices of channels-last fp16 buffers on csrc/conv_slice.hip and
csrc/yolox.hip) against the fp32 plain path (library statements) on the same state dict, run-to-run and eager-to-replay
reproducibility, the absence of library calls and concatenations from the fast path, the packed head output under
`get_bboxes`, and the rebuild of the merged / padded operands when a weight changes -- never inside a capture.

YOLOX_X at [1, 3, 64, 64] (the deepest map is 2 x 2: every SPP window is larger than the map) and [2, 3, 96, 128];
YOLOX_S (no padded layer, 64-column tiles) at [1, 3, 64, 96]."""
import copy
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES = (("x", (1, 3, 64, 64)), ("x", (2, 3, 96, 128)), ("s", (1, 3, 64, 96)))
NAMES = tuple(f"{n}_{l}" for n in ("cls_score", "bbox_pred", "objectness") for l in (1, 2, 3))
BAR = 3e-2      # the project's model bar: 3e-2 * max(1, |ref|max) (tests/test_centernet_gpu.py)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def nets():
    """Per architecture one state dict in three models: fp16 (fast path), fp32 and fp16 on an operator set WITHOUT the
    fast entries (plain path); the images; the plain fp32 outputs, computed once."""
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S, YOLOX_X
    plain_ops = types.SimpleNamespace()
    out = {}
    g = torch.Generator().manual_seed(11)
    for key, cfg in (("x", YOLOX_X), ("s", YOLOX_S)):
        base = YOLOX(cfg, seed=0, ops=plain_ops)                       # built once (its initialisation runs a forward), copied
        ref32, plain16 = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda().half()
        fast = base.cuda().half()
        fast.ops = fn
        sd = {k: v.float() for k, v in fast.state_dict().items()}       # the fp16 weights, exactly, in every model
        ref32.load_state_dict(sd)
        plain16.load_state_dict(sd)
        out[key] = dict(fast=fast, ref32=ref32, plain16=plain16)
    out["images"] = {c: torch.randn(c[1], generator=g).cuda() for c in CASES}
    out["ref"] = {c: tuple(o.clone() for o in out[c[0]]["ref32"](out["images"][c])) for c in CASES}
    return out


@pytest.mark.parametrize("case", CASES, ids=str)
def test_fast_path_against_the_fp32_plain_path(nets, case):
    key, shape = case
    img = nets["images"][case]
    B, _, H, W = shape
    got = nets[key]["fast"](img.half())
    p16 = nets[key]["plain16"](img.half())
    assert len(got) == 9
    for i, (name, g, p, r) in enumerate(zip(NAMES, got, p16, nets["ref"][case])):
        s = (8, 16, 32)[i % 3]
        assert g.shape == (B, (80, 4, 1)[i // 3], H // s, W // s) and g.dtype == torch.float16 and r.dtype == torch.float32
        scale = max(1.0, float(r.abs().max()))
        err, err16 = float((g.float() - r).abs().max()), float((p.float() - r).abs().max())
        print(f"{case} {name}: |ref|max {float(r.abs().max()):.4f}, fast path err {err:.3e}, "
              f"plain fp16 path err {err16:.3e} (bar {BAR * scale:.3e})")
        assert float(r.max() - r.min()) > 1e-3, f"{name} is a constant"
        assert err16 <= BAR * scale, f"{name}: the plain fp16 path misses the bar, which would make it meaningless"
        assert err <= BAR * scale, name


@pytest.mark.parametrize("case", CASES, ids=str)
def test_two_runs_and_the_replay_give_equal_bits(nets, case):
    from bevformer_tensorrt_amd.functions.decode2d import box_nms, yolox_decode
    from bevformer_tensorrt_amd.yolox import YOLOXRunner, num_priors
    key, shape = case
    model, img = nets[key]["fast"], nets["images"][case].half()
    a = [o.clone() for o in model(img)]
    b = model(img)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    cfg = model.cfg
    boxes, scores, labels = yolox_decode(list(b[:3]), list(b[3:6]), list(b[6:]), cfg["strides"])
    dec = box_nms(boxes, scores, labels, score_threshold=cfg["test_cfg"]["score_thr"],
                  iou_threshold=cfg["test_cfg"]["nms"]["iou_threshold"], class_aware=True, padded=True)
    runner = YOLOXRunner(model, shape[0], *shape[2:])
    for _ in range(2):
        out = runner.step(img)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, runner.head_outputs):
        assert torch.equal(_bits(x), _bits(y)), name
    P = num_priors(*shape[2:])
    assert len(out) == 4 and out[0].shape == (shape[0], P, 4) and out[3].dtype == torch.int32
    for name, x, y in zip(("boxes", "scores", "labels", "count"), dec, out):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert int(out[3].max()) > 0


class _Counter:
    """Monkey-patch probes: counts the calls of the library entries the plain path is made of."""
    NAMES = (("conv2d", F), ("max_pool2d", F), ("interpolate", F), ("silu", F), ("sigmoid", torch), ("cat", torch))

    def __init__(self, monkeypatch):
        self.counts = {n: 0 for n, _ in self.NAMES}
        for name, mod in self.NAMES:
            monkeypatch.setattr(mod, name, self._wrap(name, getattr(mod, name)))

    def _wrap(self, name, inner):
        def probe(*args, **kwargs):
            self.counts[name] += 1
            return inner(*args, **kwargs)
        return probe


@pytest.mark.parametrize("case", CASES[1:], ids=str)
def test_no_library_call_and_no_concatenation_on_the_fast_path(nets, monkeypatch, case):
    from bevformer_tensorrt_amd.functions import conv as C
    from bevformer_tensorrt_amd.yolox import ConvAct, CSPLayer
    key, _ = case
    img = nets["images"][case]
    fast = nets[key]["fast"]
    fast(img.half())                                  # (warm: merged and padded operands built)
    misses = list(C.CONV_MISSES)
    counter = _Counter(monkeypatch)
    outs = fast(img.half())
    torch.cuda.synchronize()
    print("fast :", counter.counts)
    assert counter.counts == dict(conv2d=0, max_pool2d=0, interpolate=0, silu=0, sigmoid=0, cat=0)
    assert C.CONV_MISSES == misses and len(outs) == 9
    nets[key]["plain16"](img.half())
    torch.cuda.synchronize()
    print("plain:", counter.counts)
    # from the layer list: every convolution module once; a sigmoid per ConvModule; the three SPP pools; the two PAFPN
    # up-samplings; concatenations: Focus, SPP, one per CSP layer, four in the PAFPN
    convs = sum(1 for m in fast.modules() if isinstance(m, nn.Conv2d))
    acts = sum(1 for m in fast.modules() if isinstance(m, ConvAct))
    csp = sum(1 for m in fast.modules() if isinstance(m, CSPLayer))
    assert convs == {"x": 155, "s": 83}[key] and acts == convs - 9 and csp == 8
    assert counter.counts == dict(conv2d=convs, max_pool2d=3, interpolate=2, silu=0, sigmoid=acts, cat=1 + 1 + csp + 4)


@pytest.mark.parametrize("case", CASES[1:], ids=str)
def test_packed_head_outputs_decode_in_place(nets, case):
    key, shape = case
    model = nets[key]["fast"]
    outs = model(nets["images"][case].half())
    for l in range(3):
        level = (outs[l], outs[3 + l], outs[6 + l])
        ptr = level[0].untyped_storage().data_ptr()
        assert all(o.untyped_storage().data_ptr() == ptr for o in level)      # three slices of one packed tensor
        assert level[0].stride(1) == 1 and level[0].stride(3) == 88
        assert level[1].data_ptr() == level[0].data_ptr() + 2 * 80 and level[2].data_ptr() == level[0].data_ptr() + 2 * 84
    assert outs[0].untyped_storage().data_ptr() != outs[1].untyped_storage().data_ptr()
    B, _, H, W = shape
    metas = [dict(scale_factor=[0.5, 0.5, 0.5, 0.5]) for _ in range(B)]
    got = model.get_bboxes(outs, metas, rescale=True)
    want = model.get_bboxes([o.contiguous() for o in outs], metas, rescale=True)
    assert len(got) == B
    for (gb, gl), (wb, wl) in zip(got, want):
        assert gb.shape[1] == 5 and gl.dtype == torch.int64 and gb.shape[0] > 0
        assert torch.equal(gb.view(torch.int32), wb.view(torch.int32)) and torch.equal(gl, wl)


def test_capture_guard_and_weight_reload():
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    model = YOLOX(YOLOX_S, seed=3).cuda().half()
    img = torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda().half()
    scratch = torch.zeros(8, device="cuda")
    assert model.operands(build=False) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)                                               # raises before it launches anything
        with pytest.raises(RuntimeError):
            model.prepare()
    del graph
    assert model.operands(build=False) is None
    # after prepare() the capture succeeds and replays the eager bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.prepare()
        eager = [o.clone() for o in model(img)]
    torch.cuda.current_stream().wait_stream(s)
    ops0 = model.operands(build=False)
    assert ops0 is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = model(img)
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, outs, eager):
        assert torch.equal(_bits(a), _bits(b)), n
    del graph, outs
    # new weights: level 2's objectness predictor becomes the constant 0.5; the operands are stale and rebuilt
    with torch.no_grad():
        model.bbox_head.conv_obj[1].weight.zero_()
        model.bbox_head.conv_obj[1].bias.fill_(0.5)
    assert model.operands(build=False) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)
    del graph
    new = model(img)
    assert model.operands(build=False) is not ops0
    assert bool((new[7] == 0.5).all())
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        assert torch.equal(_bits(new[i]), _bits(eager[i])), NAMES[i]
    new = [o.clone() for o in new]
    # a backbone weight doubles: different bits everywhere
    with torch.no_grad():
        model.backbone.stages[0][0].weight.mul_(2.0)
    doubled = model(img)
    assert not torch.equal(_bits(doubled[0]), _bits(new[0])) and not torch.equal(_bits(doubled[5]), _bits(new[5]))
