"""CPU-only: the plan of the INT8 BEVDepth WITH the DepthNet's DCN layer (bevdepth_int8.py on a use_dcn=True DepthNet;
quantization.build_int8_bevdet(depthnet_dcn="int8")) -- exactly two more layers, two more int8 layers and one more site
than the use_dcn=False plan of the same widths, which stays layer for layer what it was; writer and reader scales of the
two new layers on a stand-in operator set; the operand shapes (the 24-row offset weight, pad rows zero with scale 1);
the statement of the layer; the cache round trip with the new site; the keyword's error cases; and that the default
build still imports nothing new for a model without the layer."""
import os
import subprocess
import sys

import pytest
import torch

import util_bevdepth_int8 as U
import util_bevdet_int8 as UB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ShapeOps(U.ShapeOps):
    def deform_conv2d_q_nhwc(self, x_q, scale_x, offset_nhwc, w, ws, bias, groups, out=None, scale_out=None,
                             out_dtype=torch.int8, relu=False):
        B, cin, H, W = x_q.shape
        assert x_q.dtype == torch.int8 and w.dtype == torch.int8 and tuple(w.shape[1:]) == (3, 3, cin // groups)
        assert offset_nhwc.dtype == torch.float16 and offset_nhwc.shape[1] >= 18 and offset_nhwc.shape[1] % 2 == 0
        assert (offset_nhwc.shape[0], offset_nhwc.shape[2], offset_nhwc.shape[3]) == (B, H, W)
        assert bias is None and not relu and ws.shape == (w.shape[0],) and out is None
        return UB._nhwc(B, w.shape[0], H, W, out_dtype, x_q.device)


class ScaleRecorder(U.ScaleRecorder):
    def deform_conv2d_q_nhwc(self, x_q, scale_x, offset_nhwc, w, ws, bias, groups, out=None, scale_out=None,
                             out_dtype=torch.int8, relu=False):
        self._read(x_q, scale_x, "deformable conv input")
        y = self._call("deform_conv2d_q_nhwc", (x_q, scale_x, offset_nhwc, w, ws, bias, groups, out, scale_out), {})
        return self._wrote(y, scale_out, "deformable conv output")


@pytest.fixture(scope="module")
def models():
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDEPTH_R50_DCN, BEVDet
    return BEVDet(cfg=BEVDEPTH_R50, seed=0), BEVDet(cfg=BEVDEPTH_R50_DCN, seed=0)


@pytest.fixture(scope="module")
def plans(models):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    return DI.build_plan(models[0]), DI.build_plan(models[1])


def _row(l):
    return (l.op, l.key, l.src, l.dst, l.res, l.act, l.stride, l.into, l.extra, l.factor, l.dilation, l.image_bias)


def test_two_more_layers_two_more_int8_layers_one_more_site(plans):
    plain, dcn = plans
    # the plan rule: the layer adds an int8 convolution with fp16 out (no site) and the int8 deformable convolution
    # (its own site) between dn.aspp.out and dn.last
    assert len(dcn.layers) == len(plain.layers) + 2
    assert dcn.int8_layers == plain.int8_layers + 2 and len(dcn.sites) == len(plain.sites) + 1
    assert (len(plain.layers), plain.int8_layers, len(plain.sites)) == (43, 37, 37)          # what it was
    assert (len(dcn.layers), dcn.int8_layers, len(dcn.sites)) == (45, 39, 38)
    assert dcn.tail == plain.tail + 2 and dcn.layers[dcn.tail].op == "split"
    assert "dcn" in dcn.int8_ops and "dcn" not in plain.int8_ops and plain.int8_ops == ("conv", "pool")
    assert set(dcn.sites) - set(plain.sites) == {"bevdet.dn.dcn"} and not set(plain.sites) - set(dcn.sites)
    keys = [l.key for l in dcn.layers]
    i = keys.index("dn.dcn.offset")
    off, d, last = dcn.layers[i], dcn.layers[i + 1], dcn.layers[i + 2]
    assert keys[i - 1] == "dn.aspp.conv1" and (d.op, d.key) == ("dcn", "dn.dcn") and last.key == "dn.last"
    assert _row(off) == ("conv", "dn.dcn.offset", "dn.aspp.out", "dn.dcn.om", None, "none", 1, None, (), 1, 1, None)
    assert _row(d) == ("dcn", "dn.dcn", "dn.aspp.out", "dn.dcn", "dn.dcn.om", "none", 1, None, (), 1, 1, None)
    assert last.src == "dn.dcn" and plain.layers[i].src == "dn.aspp.out" and plain.layers[i].key == "dn.last"
    assert dcn.tensors["dn.dcn.om"] == "f16" and dcn.tensors["dn.dcn"] == "q" and dcn.site("dn.dcn") == "bevdet.dn.dcn"
    assert [n for n, k in dcn.tensors.items() if k == "f16"] == \
        ["dn.feat_cols", "dn.image_bias", "dn.dcn.om", "depth_net", "head.packed"]
    # every other layer is the plain plan's, in its order
    rest = [_row(l) for l in dcn.layers if l.key not in ("dn.dcn.offset", "dn.dcn")]
    want = [_row(l) for l in plain.layers]
    want[i] = want[i][:2] + ("dn.dcn",) + want[i][3:]
    assert rest == want


def test_without_aspp_the_layer_follows_the_last_basic_block():
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.int8_plan import Plan
    for use_dcn in (False, True):
        P = Plan("t.", ("conv", "dcn"))
        DI.depthnet_layers(P, DepthNet(128, 128, 16, 8, use_aspp=False, use_dcn=use_dcn), "x")
        keys = [l.key for l in P.layers if l.key]
        assert keys[-1] == "dn.last" and ("dn.dcn" in keys) == use_dcn
        if use_dcn:
            assert keys[-3:] == ["dn.dcn.offset", "dn.dcn", "dn.last"] and P.layers[-3].src == "dn.b2.out"


def test_operand_shapes(models, plans):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    fp, plan = models[1], plans[1]
    dcn = fp.view.depth_net.dcn
    with torch.no_grad():
        dcn.conv_offset.weight.normal_(0, 0.02, generator=torch.Generator().manual_seed(3))
        dcn.conv_offset.bias.normal_(0, 0.3, generator=torch.Generator().manual_seed(4))
    try:
        table = DI.quantize_operands(fp, plan)
        assert len([k for k in table if k not in ("layout", "slices", "fast")]) == 38
        w, ws, b = table["dn.dcn.offset"]                  # 18 rows padded to 24: zero rows of scale 1 and zero bias
        assert w.dtype == torch.int8 and tuple(w.shape) == (24, 3, 3, 256) and w.is_contiguous()
        assert ws.dtype == b.dtype == torch.float32 and ws.shape == b.shape == (24,)
        assert not w[18:].any() and bool((ws[18:] == 1).all()) and not b[18:].any() and w[:18].any()
        assert int(w.abs().max()) == 127 and torch.equal(b[:18], dcn.conv_offset.bias.detach().float())
        w, ws, b = table["dn.dcn"]                         # [Cout, 3, 3, Cin / groups], per-output-channel scales, no bias
        assert w.dtype == torch.int8 and tuple(w.shape) == (256, 3, 3, 64) and w.is_contiguous() and not b.any()
        assert ws.shape == (256,) and int(w.abs().max()) == 127 and bool((w.abs().amax(dim=(1, 2, 3)) == 127).all())
        deq = w.float().permute(0, 3, 1, 2) * ws[:, None, None, None]
        assert (deq - dcn.weight.detach().float()).abs().max() <= ws.max() * 0.5 + 1e-7
        # the un-quantised operands of the fp32 plain path: the same layouts, unit scales
        fl = DI._float_operands(fp, plan)
        assert tuple(fl["dn.dcn"][0].shape) == (256, 3, 3, 64) and bool((fl["dn.dcn"][1] == 1).all())
        assert tuple(fl["dn.dcn.offset"][0].shape) == (18, 3, 3, 256)
        # the plain model's table has neither
        plain = DI.quantize_operands(models[0], plans[0])
        assert "dn.dcn" not in plain and "dn.dcn.offset" not in plain
    finally:
        with torch.no_grad():
            dcn.conv_offset.weight.zero_()
            dcn.conv_offset.bias.zero_()


def test_writer_and_reader_scales_of_the_new_layers(models, plans):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    fp, plan = models[1], plans[1]
    scales = {s: 0.01 * (i + 1) for i, s in enumerate(plan.sites)}
    model = DI.Int8BEVDepth(fp, scales)
    assert model.num_int8_layers == 39
    table = model.operands()
    rec = ScaleRecorder(ShapeOps(), keep_calls=True)
    x = torch.zeros(6, 16, 44, 256, dtype=torch.float16).permute(0, 3, 1, 2)
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
    live = {}
    packed = model.run(x, pool, table, rec, tensors=live, mlp_input=torch.zeros(6, 27))
    rec.check()
    assert packed.shape == (1, 32, 128, 128)
    assert rec.reads == 37 + 9 + 2 + 2 + 2 + 1             # one more convolution input, the deformable convolution's
    assert live["dn.dcn.om"].dtype == torch.float16 and tuple(live["dn.dcn.om"].shape) == (6, 24, 16, 44)
    assert live["dn.dcn"].dtype == torch.int8 and tuple(live["dn.dcn"].shape) == (6, 256, 16, 44)
    names = [c[0] for c in rec.calls]
    i = names.index("deform_conv2d_q_nhwc")
    assert names.count("deform_conv2d_q_nhwc") == 1 and names[i - 1] == names[i + 1] == "conv_slice_q_taps"
    _, a, _, out = rec.calls[i]
    s_in, s_out = scales["bevdet.dn.aspp.out"], scales["bevdet.dn.dcn"]
    assert a[0] is live["dn.aspp.out"] and a[1] == s_in and a[2] is live["dn.dcn.om"] and a[6] == 4 and a[8] == s_out
    assert a[3] is table["dn.dcn"][0] and a[4] is table["dn.dcn"][1] and a[5] is None and out is live["dn.dcn"]
    off = rec.calls[i - 1][1]                              # the offset convolution: the same input and scale, fp16 out
    assert off[0] is live["dn.aspp.out"] and off[1] == s_in and off[10] is None and off[11] == torch.float16
    assert off[2] is table["dn.dcn.offset"][0] and off[5] == "none" and off[6] is None
    last = rec.calls[i + 1][1]                             # the last convolution reads the layer's output with its scale
    assert last[0] is live["dn.dcn"] and last[1] == s_out
    with pytest.raises(ValueError, match="no scale"):
        DI.Int8BEVDepth(fp, {k: v for k, v in scales.items() if k != "bevdet.dn.dcn"})


@torch.no_grad()
def test_the_statement_of_the_layer():
    """emulate's `other` hook on a small DepthNet: with scales None the layer is deform_conv2d on the fp32 weights; with
    scales the offsets are rounded to binary16, the column is fake-quantised with the SOURCE tensor's scale and the
    result with the layer's own."""
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.functions.deform_conv import _deform_conv2d_cpu, deform_conv2d
    from bevformer_tensorrt_amd.functions.yolox_ops import quantize_weight_taps
    from bevformer_tensorrt_amd.int8_plan import Plan, fake_quant, float_operands
    torch.manual_seed(0)
    dn = DepthNet(128, 128, 16, 8, use_dcn=True).eval()
    with torch.no_grad():
        dn.dcn.conv_offset.weight.normal_(0, 0.03)
        dn.dcn.conv_offset.bias.normal_(0, 0.3)
    P = Plan("t.", ("conv", "dcn"))
    DI.depthnet_layers(P, dn, "x")
    P.tail = len(P.layers)
    off_l, dcn_l = [l for l in P.layers if l.key in ("dn.dcn.offset", "dn.dcn")]
    assert (off_l.op, dcn_l.op) == ("conv", "dcn")

    class _View:
        depth_net = dn

    class _Model:
        view = _View()

    x = torch.randn(2, 128, 5, 6)
    mlp = torch.randn(2, 27)
    captured = {}

    def fake_emulate(model, plan, x_, ranks, table, scales, live, layers=None, other=None):
        if other is not None:
            captured["other"] = other
        live[DI.ROWS] = None

    real = DI._bi.emulate
    DI._bi.emulate = fake_emulate
    try:
        # fp32 plain path
        tf = float_operands({"dn.dcn": (dn.dcn.weight, None)})
        DI.emulate(_Model(), P, x, None, dict(tf, fast={}), None, {}, mlp)
        off = dn.dcn.conv_offset(x)
        got = captured["other"](dcn_l, x, {"dn.dcn.om": off})
        assert torch.allclose(got, deform_conv2d(x, off, dn.dcn.weight, 1, 1, 1, 4, 1), atol=1e-6)
        # quantised: source scale 0.05, the layer's own 0.1
        tq = {"dn.dcn": quantize_weight_taps(dn.dcn.weight, None)}
        scales = {"t.dn.aspp.out": 0.05, "t.dn.dcn": 0.1}
        xq = fake_quant(x, 0.05)
        om = torch.cat([off, torch.full((2, 6, 5, 6), 7.0)], dim=1).half().float()        # 24 rows: the pad is not read
        DI.emulate(_Model(), P, x, None, dict(tq, fast={}), scales, {}, mlp)
        got = captured["other"](dcn_l, xq, {"dn.dcn.om": om})
        w, ws, _ = tq["dn.dcn"]
        wf = (w.float() * ws[:, None, None, None]).permute(0, 3, 1, 2).contiguous()
        seen = []
        want = _deform_conv2d_cpu(xq, om[:, :18], wf, 1, 1, 1, 4, 1, column=lambda c: (seen.append(c), fake_quant(c, 0.05))[1])
        assert torch.equal(got, fake_quant(want, 0.1))
        q = seen[0] / 0.05
        assert float((fake_quant(seen[0], 0.05) - seen[0]).abs().max()) > 1e-3         # the column rounding is not a no-op
        assert float((q - q.round()).abs().max()) > 0.1
        steps = got / 0.1
        assert float((steps - steps.round()).abs().max()) < 1e-4 and float(got.abs().max()) > 0
    finally:
        DI._bi.emulate = real


def test_calibration_cache_round_trip_with_the_new_site(plans, tmp_path):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd.quantization import MinMaxCalibrator
    plain, dcn = plans
    g = torch.Generator().manual_seed(4)
    cal = MinMaxCalibrator()
    for i, s in enumerate(dcn.sites):
        cal.collect(s, torch.randn(64, generator=g) * (i + 1))
    path = str(tmp_path / "bevdepth_dcn.calib")
    DI.save_calibration(cal, path, {"model": "bevdepth", "bev_half": "int8", "frames": 1})
    again = MinMaxCalibrator()
    DI.load_calibration(again, path)
    a, b = DI.scales_from(cal, dcn.sites), DI.scales_from(again, dcn.sites)
    assert a == b and len(a) == 38 and "bevdet.dn.dcn" in a and all(v > 0 for v in a.values())
    # a cache recorded without the layer's site: named in the refusal
    old = MinMaxCalibrator()
    for i, s in enumerate(plain.sites):
        old.collect(s, torch.randn(64, generator=g) * (i + 1))
    path2 = str(tmp_path / "bevdepth.calib")
    DI.save_calibration(old, path2, {"model": "bevdepth", "bev_half": "int8", "frames": 1})
    loaded = MinMaxCalibrator()
    DI.load_calibration(loaded, path2)
    with pytest.raises(ValueError, match=r"bevdet\.dn\.dcn") as e:
        DI.scales_from(loaded, dcn.sites, "build_int8_bevdet")
    assert "build_int8_bevdet" in str(e.value) and "dn.aspp.out" not in str(e.value)


def test_weight_reload_makes_the_operands_stale(models, plans):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    fp, plan = models[1], plans[1]
    model = DI.Int8BEVDepth(fp, {s: 0.05 for s in plan.sites})
    t0 = model.operands()
    dcn = fp.view.depth_net.dcn
    with torch.no_grad():
        dcn.conv_offset.bias.add_(0.25)
    assert model.operands(build=False) is None
    t1 = model.operands()
    assert t1 is not t0 and not torch.equal(t1["dn.dcn.offset"][2], t0["dn.dcn.offset"][2])
    assert torch.equal(t1["dn.dcn"][0], t0["dn.dcn"][0])
    with torch.no_grad():
        dcn.conv_offset.bias.sub_(0.25)
        dcn.weight.mul_(0.5)
    assert model.operands(build=False) is None
    assert not torch.equal(model.operands()["dn.dcn"][1], t1["dn.dcn"][1])
    with torch.no_grad():
        dcn.weight.mul_(2.0)


def test_the_keywords_error_cases():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDEPTH_R50_DCN, BEVDET_R50

    def frames():
        raise AssertionError("a frame ran")
        yield

    def model(c):
        class _Model(torch.nn.Module):
            cfg = c
        return _Model()

    cpu = torch.device("cpu")
    # the default: refused exactly as before, for either bev_half, before any frame runs; the message names the keyword
    for half in ("int8", "fp16"):
        with pytest.raises(NotImplementedError, match="DCN") as e:
            Q.build_int8_bevdet(model(BEVDEPTH_R50_DCN), cpu, frames(), bev_half=half)
        assert "depthnet_dcn" in str(e.value)
        with pytest.raises(NotImplementedError, match="DCN"):
            Q.build_int8_bevdet(None, cpu, frames(), bev_half=half, cfg=BEVDEPTH_R50_DCN, depthnet_dcn=None)
    # "int8" with bev_half="fp16": the existing BEVDepth refusal
    with pytest.raises(NotImplementedError, match="BEVDepth") as e:
        Q.build_int8_bevdet(model(BEVDEPTH_R50_DCN), cpu, frames(), depthnet_dcn="int8")
    assert 'bev_half="int8"' in str(e.value) and "DCN" not in str(e.value)
    # "int8" on a model without the layer
    for c in (BEVDEPTH_R50, BEVDET_R50):
        for half in ("int8", "fp16"):
            with pytest.raises(ValueError, match="no DCN layer"):
                Q.build_int8_bevdet(model(c), cpu, frames(), bev_half=half, depthnet_dcn="int8")
    with pytest.raises(ValueError, match="no DCN layer"):
        Q.build_int8_bevdet(None, cpu, frames(), bev_half="int8", depthnet_dcn="int8")
    # any other value
    for bad in ("fp16", "INT8", True, 8, ""):
        with pytest.raises(ValueError, match="depthnet_dcn"):
            Q.build_int8_bevdet(model(BEVDEPTH_R50_DCN), cpu, frames(), bev_half="int8", depthnet_dcn=bad)
    # "int8" with bev_half="int8" gets past every refusal: the build is reached with the model's configuration
    seen = []

    class Reached(Exception):
        pass

    class D:
        @staticmethod
        def BEVDet(**kw):
            seen.append(kw.get("cfg"))
            raise Reached()

    with pytest.raises(Reached):
        Q.build_int8_bevdet(D, cpu, frames(), bev_half="int8", cfg=BEVDEPTH_R50_DCN, depthnet_dcn="int8")
    assert seen == [BEVDEPTH_R50_DCN]
    import inspect
    assert list(inspect.signature(Q.build_int8_bevdet).parameters)[-1] == "depthnet_dcn"
    assert inspect.signature(Q.build_int8_bevdet).parameters["depthnet_dcn"].default is None


def test_default_build_imports_nothing_new_for_a_model_without_the_layer():
    code = ("import sys, torch, bevformer_tensorrt_amd\n"
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
            "from bevformer_tensorrt_amd import bevdepth_int8 as DI\n"
            "from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50\n"
            "fp = BEVDet(cfg=BEVDEPTH_R50, seed=0)\n"
            "plan = DI.build_plan(fp)\n"
            "assert 'dcn' not in plan.int8_ops and not any(l.op == 'dcn' for l in plan.layers)\n"
            "m = DI.Int8BEVDepth(fp, {s: 0.05 for s in plan.sites})\n"
            "m.fake_quant_reference  # (the statement's deformable part is imported where the layer runs)\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
