"""yolox.YOLOX(YOLOX_NANO) -- use_depthwise -- on the GPU: the fast path (one csrc/dwsep_conv.hip launch per
depthwise-separable layer) against the fp32 plain path with the statistic and the bar of tests/test_yolox_gpu.py, every
launch of one forward against its own float64 statement, no library call, replay through YOLOXRunner (`step`,
`step_raw`), the capture guard, the INT8 refusal, and the dense YOLOX_S left as it was."""
import copy
import types

import pytest
import torch

from test_yolox_gpu import BAR, NAMES, _bits, _Counter
from util_dwsep import bound, statement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    """One state dict in two models (fp16 fast path with dwsep_conv_taps recorded, fp32 plain path) and the image."""
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    base = YOLOX(YOLOX_NANO, seed=0, ops=types.SimpleNamespace())
    ref32, fast = copy.deepcopy(base).cuda(), base.cuda().half()
    ref32.load_state_dict({k: v.float() for k, v in fast.state_dict().items()})
    calls = []

    def probe(x, *args):
        out = fn.dwsep_conv_taps(x, *args)
        calls.append((x.clone(), args, out.clone()))
        return out

    fast.ops = types.SimpleNamespace(**{n: getattr(fn, n) for n in fn.__all__})
    fast.ops.dwsep_conv_taps = probe
    image = torch.randn((2, 3, 96, 128), generator=torch.Generator().manual_seed(11)).cuda()
    return dict(fast=fast, ref32=ref32, image=image, calls=calls)


def test_fast_path_against_fp32_every_launch_against_its_statement_and_no_library_call(net, monkeypatch):
    from bevformer_tensorrt_amd.yolox import DWSepConvAct
    fast, calls, image = net["fast"], net["calls"], net["image"]
    fast(image.half())                                               # (warm: operands built)
    del calls[:]
    ref = net["ref32"](image)
    counter = _Counter(monkeypatch)
    got = fast(image.half())
    torch.cuda.synchronize()
    assert counter.counts == dict(conv2d=0, max_pool2d=0, interpolate=0, silu=0, sigmoid=0, cat=0)
    monkeypatch.undo()
    for name, g, r in zip(NAMES, got, ref):
        scale, err = max(1.0, float(r.abs().max())), float((g.float() - r).abs().max())
        print(f"{name}: |ref|max {float(r.abs().max()):.4f}, fast path err {err:.3e} (bar {BAR * scale:.3e})")
        assert g.shape == r.shape and float(r.max() - r.min()) > 1e-3 and err <= BAR * scale, name
    assert len(calls) == sum(isinstance(m, DWSepConvAct) for m in fast.modules()) == 30        # one launch per layer
    for i, (x, (wd, bd, wp, bp, act_dw, act_pw, res, stride, _), out) in enumerate(calls):
        C, Co = x.shape[1], wp.shape[0]
        wp4 = wp.view(Co, C, 1, 1)
        e, s, t, mag = statement(x, wd.permute(2, 0, 1).reshape(C, 1, 3, 3), bd, wp4, bp, act_dw, act_pw, res, stride)
        err, lim = (out.double().cpu() - e).abs(), bound(e, s, t, mag, wp4)
        assert bool((err <= lim).all()), f"launch {i} {tuple(x.shape)} -> {Co}: worst err / bound {float((err / lim).max()):.3f}"


@pytest.mark.parametrize("batch", [1, 2])
def test_runner_replays_the_eager_bits_from_images_and_raw_frames(net, batch):
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    fast = net["fast"]
    image = net["image"][:batch, :, :, :96].half().contiguous()
    eager = [o.clone() for o in fast(image)]
    runner = YOLOXRunner(fast, batch, 96, 96, raw_size=(60, 80), img_scale=(96, 96))
    for _ in range(2):
        out = runner.step(image)
    assert len(out) == 4 and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, runner.head_outputs))
    raw = torch.randint(0, 256, (batch, 60, 80, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).cuda()
    for _ in range(2):
        runner.step_raw(raw)
    heads = [o.clone() for o in runner.head_outputs]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(fast(runner.image_buffer), heads))


def test_capture_guard_weight_reload_and_int8_refusal():
    from bevformer_tensorrt_amd.quantization import build_int8_yolox
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    model = YOLOX(YOLOX_NANO, seed=3).cuda().half()
    img = torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(5)).cuda().half()
    with pytest.raises(NotImplementedError, match="use_depthwise"):
        build_int8_yolox(model, "cuda", iter(()))
    scratch = torch.zeros(8, device="cuda")
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)                                               # raises before it launches anything
    assert model.operands(build=False) is None
    first = [o.clone() for o in model(img)]
    ops0 = model.operands(build=False)
    with torch.no_grad():
        model.backbone.stages[0][0].depthwise_conv.weight.mul_(2.0)
    assert model.operands(build=False) is None
    second = model(img)
    assert model.operands(build=False) is not ops0 and not torch.equal(_bits(second[0]), _bits(first[0]))


def test_a_dense_model_keeps_its_operands_and_launches():
    """YOLOX_S: no depthwise entry in the operand list, the stacked first tower convolutions still there, no
    dwsep_conv_taps launch; its bits are conv_slice.hip's, which tests/test_yolox_gpu.py holds to the fp32 path."""
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S, DWSepConvAct
    model = YOLOX(YOLOX_S, seed=0).cuda().half()
    model.ops = types.SimpleNamespace(**{n: getattr(fn, n) for n in fn.__all__ if n != "dwsep_conv_taps"})
    out = model(torch.randn((1, 3, 64, 96), generator=torch.Generator().manual_seed(11)).cuda().half())
    table = model.operands(build=False)
    assert len(out) == 9 and out[0].stride(3) == 88                              # (the fast path ran)
    assert all(len(v) == 2 for k, v in table.items() if k != "slices") and ("first", 0) in table
    assert not any(isinstance(k, DWSepConvAct) for k in table) and len(table) == 83 - 9 + 3 + 3 + 1
