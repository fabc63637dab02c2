"""CPU-only: the plan of the INT8 BEVDepth (bevformer_tensorrt_amd/bevdepth_int8.py) -- layer and site counts as numbers,
the four writers of the ASPP buffer on one scale, writer and reader scales on a stand-in operator set, the shapes of the
quantised operands (the conv1 split, the padded last convolution), the calibration cache round trip, stale operands after a
weight reload, the unchanged default plan, what the default build still refuses, and that the default chain imports
neither bevdepth_int8 nor bevdepth."""
import os
import subprocess
import sys

import pytest
import torch

import util_bevdepth_int8 as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fp():
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDet
    return BEVDet(cfg=BEVDEPTH_R50, seed=0)


@pytest.fixture(scope="module")
def plan(fp):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    return DI.build_plan(fp)


def test_layer_and_site_counts(plan):
    ops = {}
    for l in plan.layers:
        ops[l.op] = ops.get(l.op, 0) + 1
    # bevdet_int8's 23 convolutions without depth_net (22) + the DepthNet's 14: reduce_conv, context_conv, three
    # BasicBlocks of two, aspp1 .. aspp4, conv1, the last 1 x 1.  The gates and the average pool are no matrix-core layers.
    assert ops == dict(quantize=1, conv=36, gate=1, avgpool=1, split=1, pool=1, upsample=2)
    assert len(plan.layers) == 43 and plan.int8_layers == 37              # 36 convolutions + the pooling; 24 without
    assert plan.tail == 17 and plan.layers[plan.tail].op == "split"
    f16 = [n for n, k in plan.tensors.items() if k == "f16"]
    assert f16 == ["dn.feat_cols", "dn.image_bias", "depth_net", "head.packed"]
    # 26 sites of bevdet_int8 + 11: dn.r, dn.depth0, dn.context, six BasicBlock tensors, dn.aspp.cat, dn.aspp.out
    assert len(plan.sites) == 37 and len(set(plan.sites)) == 37
    dn = [s for s in plan.sites if s.startswith("bevdet.dn.")]
    assert dn == ["bevdet.dn.r", "bevdet.dn.context", "bevdet.dn.depth0"] + \
        [f"bevdet.dn.b{i}.{t}" for i in range(3) for t in ("t1", "out")] + ["bevdet.dn.aspp.cat", "bevdet.dn.aspp.out"]
    assert plan.buffers == {"cat": 640, "dn.rows": 128, "dn.aspp.cat": 1024}
    assert [l.dilation for l in plan.layers if l.key and l.key.startswith("dn.aspp") and l.key != "dn.aspp.conv1"] == [1, 6, 12, 18]
    assert sum(1 for l in plan.layers if l.res is not None and l.op == "conv") == 9      # one identity per BasicBlock


def test_the_four_writers_of_the_aspp_buffer_share_one_scale(plan):
    writers = [l for l in plan.layers if l.into is not None and l.into[0] == "dn.aspp.cat"]
    assert [l.into for l in writers] == [("dn.aspp.cat", 256 * i) for i in range(4)]
    assert {plan.site(l.dst) for l in writers} == {plan.site("dn.aspp.cat")} == {"bevdet.dn.aspp.cat"}
    reader = [l for l in plan.layers if l.src == "dn.aspp.cat"]
    assert len(reader) == 1 and reader[0].key == "dn.aspp.conv1" and reader[0].image_bias == "dn.image_bias"


def test_the_default_plan_is_unchanged():
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    from bevformer_tensorrt_amd.bevdet import BEVDet
    p = BI.build_plan(BEVDet(seed=0))
    assert len(p.layers) == 28 and p.int8_layers == 24 and len(p.sites) == 26 and p.buffers == {"cat": 640}
    assert [l.key for l in p.layers if l.op == "conv"][:2] == ["depth_net", "s0.b0.down"]
    assert not hasattr(p, "tail")


def test_operand_shapes(fp, plan):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    table = DI.quantize_operands(fp, plan)
    want = {"dn.reduce_conv": (256, 3, 256), "dn.context_conv": (64, 1, 256), "dn.b0.conv1": (256, 3, 256),
            "dn.b2.conv2": (256, 3, 256), "dn.aspp1": (256, 1, 256), "dn.aspp2": (256, 3, 256), "dn.aspp4": (256, 3, 256),
            "dn.aspp.conv1": (256, 1, 1024), "dn.last": (64, 1, 256), "s0.b0.down": (128, 3, 64), "head.final": (32, 3, 384)}
    for key, (cout, k, cin) in want.items():
        w, ws, b = table[key]
        assert w.dtype == torch.int8 and tuple(w.shape) == (cout, k, k, cin) and w.is_contiguous(), key
        assert ws.dtype == b.dtype == torch.float32 and ws.shape == b.shape == (cout,), key
        assert int(w.abs().max()) == 127
    assert len([k for k in table if k not in ("layout", "slices", "fast")]) == 36 and "depth_net" not in table
    assert table["layout"] == dict(row_stride=128, feat_offset=0, depth_offset=64, depth_padded=64)
    # the last convolution: 59 depth bins padded to 64 with zero rows of scale 1 and zero bias
    w, ws, b = table["dn.last"]
    assert not w[59:].any() and bool((ws[59:] == 1).all()) and not b[59:].any() and w[:59].any()
    # conv1 is split: its first 4 mid columns are the int8 operand (no bias: the per-image bias carries it), the pooled
    # branch's mid columns stay fp16
    a = fp.view.depth_net.aspp
    w, ws, b = table["dn.aspp.conv1"]
    assert not b.any()
    deq = w.float().reshape(256, 1024) * ws[:, None]
    ref = a.conv1.weight.detach().float().flatten(1)
    assert (deq - ref[:, :1024]).abs().max() <= ws.max() * 0.5 + 1e-7
    assert torch.equal(table["fast"]["conv1_pool"].float(), ref[:, 1024:]) and table["fast"]["pool_w"].shape == (256, 256)


def test_writer_and_reader_scales_agree(fp, plan):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    scales = {s: 0.01 * (i + 1) for i, s in enumerate(plan.sites)}
    model = DI.Int8BEVDepth(fp, scales)
    table = model.operands()
    assert model.operands() is table and model.operands(build=False) is table
    rec = U.ScaleRecorder(U.ShapeOps())
    x = torch.zeros(6, 16, 44, 256, dtype=torch.float16).permute(0, 3, 1, 2)
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
    live = {}
    packed = model.run(x, pool, table, rec, tensors=live, mlp_input=torch.zeros(6, 27))
    rec.check()
    assert packed.shape == (1, 32, 128, 128) and packed.dtype == torch.float16
    # conv inputs 36, identities 9, the gate's and the average pool's input, pooling operands 2, up-sampler inputs 2
    assert rec.reads == 36 + 9 + 2 + 2 + 2
    f16 = sorted(n for n, t in live.items() if t.dtype == torch.float16)
    assert f16 == ["depth_net", "dn.feat_cols", "dn.image_bias", "dn.rows", "head.packed", "x.f16"]
    assert live["dn.rows"].shape == (6, 128, 16, 44) and live["dn.aspp.cat"].shape == (6, 1024, 16, 44)
    assert live["dn.aspp.cat"].dtype == torch.int8 and live["depth_net"].data_ptr() == live["dn.rows"].data_ptr()
    for i in range(4):
        assert live[f"dn.aspp.b{i}"].data_ptr() == live["dn.aspp.cat"][:, 256 * i:].data_ptr()
    assert live["dn.feat_cols"].shape[1] == 64 and live["dn.feat_cols"].data_ptr() == live["dn.rows"].data_ptr()
    # a writer of the ASPP buffer with a scale of its own is seen
    model2 = DI.Int8BEVDepth(fp, dict(scales))
    model2.plan.group["dn.aspp.b2"] = "dn.aspp.b2"
    model2.scales["bevdet.dn.aspp.b2"] = 0.5
    rec2 = U.ScaleRecorder(U.ShapeOps())
    pool2 = lambda d, f, s: rec2.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
    with pytest.raises(AssertionError, match="written with 0.5"):
        model2.run(x, pool2, table, rec2, mlp_input=torch.zeros(6, 27))
    with pytest.raises(ValueError, match="no scale"):
        DI.Int8BEVDepth(fp, {k: v for k, v in scales.items() if k != "bevdet.dn.aspp.cat"})
    with pytest.raises(ValueError, match="mlp_input"):
        model.run(x, pool, table, rec)


def test_weight_reload_makes_the_operands_stale(fp, plan):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    model = DI.Int8BEVDepth(fp, {s: 0.05 for s in plan.sites})
    t0 = model.operands()
    a = fp.view.depth_net.aspp
    with torch.no_grad():
        a.aspp3.weight.mul_(0.5)
    assert model.operands(build=False) is None
    t1 = model.operands()
    assert t1 is not t0 and not torch.equal(t1["dn.aspp3"][1], t0["dn.aspp3"][1])
    with torch.no_grad():
        a.aspp3.weight.mul_(2.0)
        fp.view.depth_net.bn.running_mean.add_(1.0)               # a buffer: the packed gate block follows it
    assert model.operands(build=False) is None
    assert not torch.equal(model.operands()["fast"]["gate"], t1["fast"]["gate"])
    with torch.no_grad():
        fp.view.depth_net.bn.running_mean.sub_(1.0)


def test_calibration_cache_round_trip(plan, tmp_path):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd.quantization import MinMaxCalibrator
    g = torch.Generator().manual_seed(4)
    cal = MinMaxCalibrator()
    for i, s in enumerate(plan.sites):
        cal.collect(s, torch.randn(64, generator=g) * (i + 1))
    path = str(tmp_path / "bevdepth.calib")
    DI.save_calibration(cal, path, {"model": "bevdepth", "bev_half": "int8", "frames": 1})
    again = MinMaxCalibrator()
    DI.load_calibration(again, path)
    a, b = DI.scales_from(cal, plan.sites), DI.scales_from(again, plan.sites)
    assert a == b and len(a) == 37 and all(v > 0 for v in a.values())


def test_gates_statement_is_the_modules_gates(fp, plan):
    """gates_statement (the statement's stand-in for lss_camera_gate) against DepthNet.gates in float64."""
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    dn = fp.view.depth_net
    g = torch.Generator().manual_seed(2)
    mlp = torch.randn(6, 27, generator=g) * 100.0
    got = DI.gates_statement(dn, mlp)
    dn64 = dn.double()
    try:
        gd, gc = dn64.gates(mlp.double())
    finally:
        dn.float()
    assert got.shape == (2, 6, 256) and got.dtype == torch.float32
    assert torch.allclose(got[0].double(), gd.flatten(1), atol=1e-6) and torch.allclose(got[1].double(), gc.flatten(1), atol=1e-6)


def test_what_the_default_build_still_refuses():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50

    class _Model(torch.nn.Module):
        cfg = BEVDEPTH_R50

    with pytest.raises(NotImplementedError, match="BEVDepth") as e:
        Q.build_int8_bevdet(_Model(), torch.device("cpu"), [])
    assert 'bev_half="int8"' in str(e.value)
    # with bev_half="int8" the stub gets past that check; whatever stops it later is no NotImplementedError
    with pytest.raises(Exception) as later:
        Q.build_int8_bevdet(_Model(), torch.device("cpu"), [], "minmax", bev_half="int8")
    assert not isinstance(later.value, NotImplementedError)
    # a module asked for BEVDepth through cfg= is refused by the default build in the same way
    with pytest.raises(NotImplementedError, match="BEVDepth"):
        Q.build_int8_bevdet(object(), "cpu", [], cfg=BEVDEPTH_R50)


def test_build_forwards_the_keywords_it_should():
    """D.BEVDet(ops=, seed=0) for a module without cfg=; cfg= is added only when given."""
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    seen = []

    class Reached(Exception):
        pass

    class D:
        @staticmethod
        def BEVDet(**kw):
            seen.append(sorted(kw))
            raise Reached()

    with pytest.raises(Reached):
        build_int8_bevdet(D, "cpu", [])
    with pytest.raises(Reached):
        build_int8_bevdet(D, "cpu", [], bev_half="int8", cfg=BEVDEPTH_R50)
    assert seen == [["ops", "seed"], ["cfg", "ops", "seed"]]


def test_default_chain_imports_neither_new_module():
    code = ("import sys, bevformer_tensorrt_amd\n"
            "from bevformer_tensorrt_amd.quantization import build_int8_bevdet\n"
            "from bevformer_tensorrt_amd.bevdet import BEVDet\n"
            "class Reached(Exception): pass\n"
            "class D:\n"
            "    @staticmethod\n"
            "    def BEVDet(**kw):\n"
            "        assert sorted(kw) == ['ops', 'seed'], kw\n"
            "        raise Reached()\n"
            "try:\n"
            "    build_int8_bevdet(D, 'cpu', [])\n"
            "except Reached:\n"
            "    pass\n"
            "else:\n"
            "    raise SystemExit('the stand-in was not reached')\n"
            "BEVDet()\n"
            "for m in ('bevdepth_int8', 'bevdepth', 'bevdet_int8'):\n"
            "    assert 'bevformer_tensorrt_amd.' + m not in sys.modules, m\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
