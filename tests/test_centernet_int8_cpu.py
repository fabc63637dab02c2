"""CPU-only: the plan of the INT8 CenterNet (bevformer_tensorrt_amd/centernet_int8.py) -- its layer and site counts
derived from the layer list, every tensor written and read with one scale (the plan run on a stand-in operator set
that computes nothing), the quantised operands' shapes, and a calibration-cache round trip."""
import pytest
import torch

import util_centernet_int8 as U


@pytest.fixture(scope="module")
def fp():
    from bevformer_tensorrt_amd.centernet import CenterNet
    return CenterNet(seed=0)


def test_layer_and_site_counts_follow_from_the_layer_list(fp):
    """ResNet-18 = 4 stages of 2 BasicBlocks: 8 conv1 + 8 conv2 + 3 downsamples (the first blocks of stages 1 .. 3) = 19
    int8 convolutions; the int8 neck adds 3 levels x (offset convolution, DCN, deconvolution) = 9; the head 2.
    Sites, one per int8 tensor: the stem's output 1; per block t1 and out, plus idt behind a downsample = 8 + 8 + 3 = 19;
    per neck level the offsets, the mask, the DCN's output and the deconvolution's output = 12; the head's hidden tensor 1.
    With the fp16 neck the last block's output is fp16 (-1), the neck's four tensors per level are not quantised (-12),
    and the one quantise pass in front of the head writes the tensor the last deconvolution writes otherwise (+1)."""
    from bevformer_tensorrt_amd import centernet_int8 as CI
    blocks = [b for st in fp.backbone.stages for b in st]
    downs = sum(1 for b in blocks if b.downsample is not None)
    levels = len(fp.neck.dcn)
    assert (len(blocks), downs, levels) == (8, 3, 3)
    p8, p16 = CI.build_plan(fp, "int8"), CI.build_plan(fp, "fp16")
    assert p8.int8_layers == 2 * len(blocks) + downs + 3 * levels + 2 == 30
    assert p16.int8_layers == 2 * len(blocks) + downs + 2 == 21
    assert len(p8.sites) == 1 + (2 * len(blocks) + downs) + 4 * levels + 1 == 33
    assert len(p16.sites) == len(p8.sites) - 1 - 4 * levels + 1 == 21
    assert len(set(p8.sites)) == 33 and set(p16.sites) < set(p8.sites) and CI.all_sites(fp) == p8.sites
    assert [l.op for l in p16.layers].count("neck_fp16") == 1 and [l.op for l in p16.layers].count("quantize") == 1
    assert p16.tensors["s3.b1.out"] == "f16" and p8.tensors["s3.b1.out"] == "q"
    # every conv2 adds its block's identity -- the block's input, or the downsample's output -- in front of the ReLU
    for p in (p8, p16):
        conv2 = [l for l in p.layers if l.op == "conv" and l.key.endswith(".conv2")]
        assert len(conv2) == 8 and all(l.res is not None and l.act == "relu" for l in conv2)
        assert sum(1 for l in conv2 if l.res.endswith(".idt")) == 3
    assert CI.dcn_int8_domain(fp) == []
    with pytest.raises(ValueError):
        CI.build_plan(fp, "int4")


@pytest.mark.parametrize("neck", ["int8", "fp16"])
def test_every_tensor_is_read_with_the_scale_it_was_written_with(fp, neck, monkeypatch):
    from bevformer_tensorrt_amd import centernet_int8 as CI
    plan = CI.build_plan(fp, neck)
    monkeypatch.setattr(fp.neck, "forward_nhwc", U.ShapeOps(fp).neck_fp16)      # (the fp16 neck's kernels need a GPU)
    scales = {s: 0.01 * (i + 1) for i, s in enumerate(plan.sites)}           # a different scale per site
    model = CI.Int8CenterNet(fp, scales, ops=None, neck=neck)
    rec = U.ScaleRecorder(U.ShapeOps(fp))
    packed = model.run(torch.zeros(1, 3, 64, 96, dtype=torch.float16), model.operands(), rec)
    assert tuple(packed.shape) == (1, 88, 16, 24) and packed.dtype == torch.float16
    rec.check()
    assert len(rec.written) == len(plan.sites) - (6 if neck == "int8" else 0)  # (offsets and masks are quantised inside the DCN)
    assert sorted(rec.written.values()) == sorted(v for s, v in scales.items() if not s.endswith((".offset", ".mask")))
    assert rec.reads >= len(rec.written)
    with pytest.raises(ValueError):
        CI.Int8CenterNet(fp, {k: v for k, v in scales.items() if not k.endswith("head.hidden")}, neck=neck)
    with pytest.raises(ValueError):
        CI.Int8CenterNet(fp, dict(scales, **{plan.sites[0]: float("inf")}), neck=neck)


def test_quantised_operands(fp):
    from bevformer_tensorrt_amd import centernet_int8 as CI
    plan = CI.build_plan(fp, "int8")
    table = CI.quantize_operands(fp, plan)
    assert table["slices"] == [(0, 80), (80, 82), (82, 84)]
    w, ws, b = table["s1.b0.down"]
    assert w.shape == (128, 1, 1, 64) and w.dtype == torch.int8 and ws.shape == (128,) and b.dtype == torch.float32
    assert table["s3.b1.conv2"][0].shape == (512, 3, 3, 512) and table["head.first"][0].shape == (192, 3, 3, 64)
    assert table["head.final"][0].shape == (88, 1, 1, 192) and not table["head.final"][0][84:].any()
    ow, osc, ob = table["neck0.offset"]
    assert ow.shape == (32, 3, 3, 512) and not ow[27:].any() and not ob[27:].any()
    dw, ds, db = table["neck1.dcn"]
    assert dw.shape == (128, 256, 3, 3) and isinstance(ds, float) and int(dw.abs().max()) == 127
    uw, us, ub = table["neck2.up"]
    assert uw.shape == (64, 64, 4, 4) and us.shape == (64,) and torch.equal(uw.abs().amax(dim=(0, 2, 3)).int(), torch.full((64,), 127).int())
    # the de-quantised weights are within half a step of the model's
    up = fp.neck.deconv[2].weight.detach().float()
    assert float((uw.float() * us[None, :, None, None] - up).abs().max()) <= float(us.max()) / 2 * (1 + 1e-6)
    # cached, and rebuilt when a weight changes
    model = CI.Int8CenterNet(fp, {s: 1.0 for s in plan.sites})
    t0 = model.operands()
    assert model.operands() is t0 and model.operands(build=False) is t0
    with torch.no_grad():
        fp.heads["wh"][1].bias.add_(1.0)
    assert model.operands(build=False) is None and model.operands() is not t0
    with torch.no_grad():
        fp.heads["wh"][1].bias.sub_(1.0)


@pytest.mark.parametrize("calibrator", ["minmax", "entropy"])
def test_calibration_cache_round_trip_gives_equal_scales(fp, calibrator, tmp_path):
    from bevformer_tensorrt_amd import centernet_int8 as CI
    from bevformer_tensorrt_amd.quantization import get_calibrator
    sites = CI.all_sites(fp)
    g = torch.Generator().manual_seed(7)
    cal = get_calibrator(calibrator)()
    for frame in range(2):
        for i, s in enumerate(sites):
            cal.collect(s, torch.randn(4, 16, 8, 8, generator=g) * (1.0 + i))
    path = str(tmp_path / "centernet.calib")
    CI.save_calibration(cal, path, {"model": "centernet", "sites": len(sites), "frames": 2})
    again = get_calibrator(calibrator)()
    extra = CI.load_calibration(again, path)
    assert extra["frames"] == 2 and extra["sites"] == 33
    for neck in ("int8", "fp16"):
        want = CI.scales_from(cal, CI.build_plan(fp, neck).sites)
        assert CI.scales_from(again, CI.build_plan(fp, neck).sites) == want and all(v > 0 for v in want.values())
    with pytest.raises(ValueError):
        CI.scales_from(get_calibrator(calibrator)(), sites)
