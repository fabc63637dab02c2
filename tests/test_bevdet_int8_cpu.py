"""CPU-only: the plan of the INT8 BEV half of BEVDet (bevformer_tensorrt_amd/bevdet_int8.py) -- its layer and site counts
as numbers, writer and reader scales on a stand-in operator set (the two writers of the concatenation buffer included),
the shapes of the merged and quantised operands, the calibration cache round trip, and that the default
build_int8_bevdet(bev_half="fp16") never imports the new module."""
import subprocess
import sys

import pytest
import torch

import util_bevdet_int8 as U


@pytest.fixture(scope="module")
def fp():
    from bevformer_tensorrt_amd.bevdet import BEVDet
    return BEVDet(seed=0)


@pytest.fixture(scope="module")
def plan(fp):
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    return BI.build_plan(fp)


def test_layer_and_site_counts(plan):
    ops = {}
    for l in plan.layers:
        ops[l.op] = ops.get(l.op, 0) + 1
    # depth_net 1 + three stages of (downsample, conv1, conv2, conv1, conv2) 15 + neck 2 + up2 2 + shared 1 + heads 2
    assert ops == dict(quantize=1, conv=23, split=1, pool=1, upsample=2)
    assert len(plan.layers) == 28 and plan.int8_layers == 24
    kinds = list(plan.tensors.values())
    assert kinds.count("f16") == 2 and [n for n, k in plan.tensors.items() if k == "f16"] == ["depth_net", "head.packed"]
    # 27 int8 tensors and the buffer two of them are slices of; 26 scales: the two slices share the buffer's
    assert kinds.count("q") == 28 and len(plan.sites) == 26 and len(set(plan.sites)) == 26
    assert plan.site("s0.b1.out") == plan.site("up4") == plan.site("cat") == "bevdet.cat"
    assert plan.buffers == {"cat": 640}
    into = {l.dst: l.into for l in plan.layers if l.into is not None}
    assert into == {"s0.b1.out": ("cat", 0), "up4": ("cat", 128)}
    assert [l.factor for l in plan.layers if l.op == "upsample"] == [4, 2]
    assert sum(1 for l in plan.layers if l.res is not None and l.op == "conv") == 6      # one identity per BasicBlock
    assert sum(1 for l in plan.layers if l.stride == 2) == 6                             # downsample + conv1 per stage


def test_operand_shapes(fp, plan):
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    table = BI.quantize_operands(fp, plan)
    want = {"depth_net": (128, 1, 256), "s0.b0.down": (128, 3, 64), "s0.b1.conv2": (128, 3, 128), "s2.b0.conv1": (512, 3, 256),
            "neck_conv.0": (512, 3, 640), "neck_conv.1": (512, 3, 512), "up2_conv.0": (256, 3, 512), "up2_conv.1": (256, 1, 256),
            "shared_conv": (64, 3, 256), "head.first": (384, 3, 64), "head.final": (32, 3, 384)}
    for key, (cout, k, cin) in want.items():
        w, ws, b = table[key]
        assert w.dtype == torch.int8 and tuple(w.shape) == (cout, k, k, cin) and w.is_contiguous(), key
        assert ws.dtype == b.dtype == torch.float32 and ws.shape == b.shape == (cout,), key
        assert int(w.abs().max()) == 127
    assert len([k for k in table if k not in ("layout", "slices")]) == 23
    assert table["layout"] == dict(row_stride=128, feat_offset=0, depth_offset=64)
    assert table["slices"] == [(0, 2), (2, 3), (3, 6), (6, 8), (8, 10), (10, 20)]
    # depth_net's pad columns and the packed output's pad channels: zero rows with scale 1
    w, ws, b = table["depth_net"]
    assert not w[123:].any() and bool((ws[123:] == 1).all()) and not b[123:].any()
    w, ws, b = table["head.final"]
    assert not w[20:].any() and bool((ws[20:] == 1).all())
    # the heads' final convolution is block-diagonal: head i reads hidden channels 64 i .. 64 i + 63 only
    for i, (a, z) in enumerate(table["slices"]):
        other = torch.ones(384, dtype=torch.bool)
        other[64 * i:64 * i + 64] = False
        assert not w[a:z][..., other].any()


def test_writer_and_reader_scales_agree(fp, plan):
    """Every int8 tensor is read with the scale it was written with; the concatenation buffer has two writers and one
    reader, all three on the group's scale; only depth_net's logits and the packed output are fp16."""
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    scales = {s: 0.01 * (i + 1) for i, s in enumerate(plan.sites)}
    model = BI.Int8BEVDet(fp, scales)
    table = model.operands()
    assert model.operands() is table and model.operands(build=False) is table
    rec = U.ScaleRecorder(U.ShapeOps())
    x = torch.zeros(6, 16, 44, 256, dtype=torch.float16).permute(0, 3, 1, 2)
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
    live = {}
    packed = model.run(x, pool, table, rec, tensors=live)
    rec.check()
    assert packed.shape == (1, 32, 128, 128) and packed.dtype == torch.float16
    assert rec.reads == 23 + 6 + 2 + 2                    # conv inputs, identities, pooling operands, up-sampler inputs
    f16 = sorted(n for n, t in live.items() if t.dtype == torch.float16)
    assert f16 == ["depth_net", "head.packed", "x.f16"]
    assert live["cat"].shape == (1, 640, 64, 64) and live["up2"].shape == (1, 512, 128, 128)
    assert live["s0.b1.out"].data_ptr() == live["cat"].data_ptr()
    assert live["up4"].data_ptr() == live["cat"][:, 128:].data_ptr()
    # a scale out of place is seen: the up-sampler writing its slice with another scale than stage 1's block
    bad = dict(scales)
    model2 = BI.Int8BEVDet(fp, bad)
    model2.plan.group["up4"] = "up4"
    model2.scales["bevdet.up4"] = 0.5
    rec2 = U.ScaleRecorder(U.ShapeOps())
    pool2 = lambda d, f, s: rec2.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
    with pytest.raises(AssertionError, match="written with 0.5"):
        model2.run(x, pool2, table, rec2)
    with pytest.raises(ValueError, match="no scale"):
        BI.Int8BEVDet(fp, {k: v for k, v in scales.items() if k != "bevdet.cat"})
    with pytest.raises(ValueError, match="positive"):
        BI.Int8BEVDet(fp, {**scales, "bevdet.cat": 0.0})


def test_weight_reload_makes_the_operands_stale(fp, plan):
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    model = BI.Int8BEVDet(fp, {s: 0.05 for s in plan.sites})
    t0 = model.operands()
    with torch.no_grad():
        fp.shared_conv.weight.mul_(0.5)
    assert model.operands(build=False) is None
    assert model.operands() is not t0
    with torch.no_grad():
        fp.shared_conv.weight.mul_(2.0)


def test_calibration_cache_round_trip(plan, tmp_path):
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    from bevformer_tensorrt_amd.quantization import MinMaxCalibrator
    g = torch.Generator().manual_seed(4)
    cal = MinMaxCalibrator()
    for i, s in enumerate(plan.sites):
        cal.collect(s, torch.randn(64, generator=g) * (i + 1))
    path = str(tmp_path / "bevdet.calib")
    BI.save_calibration(cal, path, {"model": "bevdet", "bev_half": "int8", "frames": 1})
    again = MinMaxCalibrator()
    BI.load_calibration(again, path)
    a, b = BI.scales_from(cal, plan.sites), BI.scales_from(again, plan.sites)
    assert a == b and len(a) == 26 and all(v > 0 for v in a.values())
    with pytest.raises(ValueError, match="no calibration data"):
        BI.scales_from(MinMaxCalibrator(), plan.sites)


def test_build_arguments():
    from bevformer_tensorrt_amd import bevdet as D
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    with pytest.raises(ValueError, match="bev_half"):
        build_int8_bevdet(D, "cpu", [], bev_half="int4")
    with pytest.raises(ValueError, match="calibration_cache"):
        build_int8_bevdet(D, "cpu", [], calibration_cache="x.calib")


def test_default_build_never_imports_the_int8_bev_half():
    """bev_half="fp16" reaches the construction of the model (the stand-in raises there) with bevdet_int8 not imported."""
    code = ("import sys, bevformer_tensorrt_amd\n"
            "from bevformer_tensorrt_amd.quantization import build_int8_bevdet\n"
            "class Reached(Exception): pass\n"
            "class D:\n"
            "    @staticmethod\n"
            "    def BEVDet(**kw):\n"
            "        raise Reached()\n"
            "try:\n"
            "    build_int8_bevdet(D, 'cpu', [])\n"
            "except Reached:\n"
            "    pass\n"
            "else:\n"
            "    raise SystemExit('the stand-in was not reached')\n"
            "assert 'bevformer_tensorrt_amd.bevdet_int8' not in sys.modules\n"
            "print('ok')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
