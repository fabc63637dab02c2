"""The INT8 BEVDepth with the DepthNet's DCN layer (quantization.build_int8_bevdet(<BEVDEPTH_R50_DCN model>,
bev_half="int8", depthnet_dcn="int8")) on the frame sizes of tests/test_bevdepth_int8_gpu.py, `conv_offset` scaled to
offsets of a standard deviation of one pixel as tests/test_bevdepth_dcn_gpu.py does: synthetic weights, two min-max
calibration frames, one build per module and one rebuild from the calibration cache.

* THE MODEL GATE of the other INT8 builds: at each of the six head outputs the rms error of the int8 kernels against the
  fp32 plain path is <= 1.25 x the fake-quant statement's.  Absolute errors against the fp16 model's 3e-2 bar are
  printed, not gated.
* every call of one forward against its own float64 statement; the two new calls: the offset convolution (int8, fp16
  out) inside the derived interval of the epilogue, the deformable convolution with the rules of
  tests/test_deform_conv_s8_gpu.py -- the column byte is rne(s64) except within EPS of a half-integer, where either
  neighbour passes, so the integer sum lies in [sum_min, sum_max] over those choices, and the output inside the
  epilogue's interval of that range;
* BEVDetRunner.step at batch 1 and batch 2 and step_raw replay bit-equal to the eager run; the capture guard; a weight
  reload (a changed conv_offset.bias included) rebuilds the operands; the cache rebuild gives the same scales without
  running a frame; exactly one deform_conv2d_q_nhwc per forward and no fp16 deformable launch."""
import numpy as np
import pytest
import torch

import test_bevdepth_dcn_int8_cpu as TC
import test_bevdepth_gpu as TD
import util_conv_slice_s8 as S
import util_deform_conv_s8 as D
from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50_DCN
from test_bevdepth_dcn_gpu import _build, _CountingOps

pytestmark = pytest.mark.gpu

NAMES = TD.NAMES


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    fp = _build(BEVDEPTH_R50_DCN, "hip", torch.float16)
    dcn = fp.view.depth_net.dcn
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        dcn.conv_offset.weight.copy_((torch.randn(18, 256, 3, 3, generator=g) * 0.02).to(dcn.conv_offset.weight))
        dcn.conv_offset.bias.copy_((torch.randn(18, generator=g) * 0.3).to(dcn.conv_offset.bias))
    rigs = [jittered_rig(fp.view, k) for k in (1, 2, 3)]
    rig = rigs[0]
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*rig)]
    mlp = fp.view.get_mlp_input(*rig).cuda()
    calib = fp.view.calibration_matrices(*rig).cuda()
    gen = torch.Generator().manual_seed(1)
    imgs = torch.randn(2, 6, 3, 256, 704, generator=gen).cuda().half()
    # the offset convolution scaled to a standard deviation of one pixel on this frame, measured on the fp32 plain DepthNet
    ref = _build(BEVDEPTH_R50_DCN, "torch", torch.float32, state=fp.state_dict())
    x32 = fp.image_features(imgs[0]).float().contiguous()
    seen = []
    hook = ref.view.depth_net.dcn.conv_offset.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
    with torch.no_grad():
        ref.view.depth_net(x32, mlp.reshape(6, 27))
        scale = 1.0 / float(seen[0].std())
        dcn.conv_offset.weight.mul_(scale)
        dcn.conv_offset.bias.mul_(scale)
    hook.remove()
    del ref, x32
    frames = [(torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks, mlp) for _ in range(2)]
    cache = str(tmp_path_factory.mktemp("calib") / "bevdepth_dcn.calib")
    kw = dict(bev_half="int8", calibration_cache=cache, depthnet_dcn="int8")
    model, qops, note = build_int8_bevdet(fp, "cuda", frames, "minmax", **kw)
    again, _, note2 = build_int8_bevdet(fp, "cuda", [], "minmax", **kw)
    x = model._features(imgs[:1]).clone()
    return dict(fp=fp, rigs=rigs, ranks=ranks, mlp=mlp, calib=calib, imgs=imgs, img=imgs[:1], model=model, note=note,
                again=again, note2=note2, x=x)


def test_notes_and_the_cache_rebuild(built):
    from bevformer_tensorrt_amd.bevdepth_int8 import Int8BEVDepth
    n, n2 = built["note"], built["note2"]
    m, m2 = built["model"], built["again"]
    assert type(m) is Int8BEVDepth and m.fp.view.depth_net.use_dcn
    plan = m.plan
    assert (n["bev_half"], n["calibration_frames"], n["depthnet_dcn"]) == ("int8", 2, "int8")
    assert (n["int8_bev_half_layers"], n["bev_half_scale_sites"]) == (plan.int8_layers, len(plan.sites)) == (39, 38)
    assert (n["depthnet_int8_layers"], n["depthnet_scale_sites"]) == (16, 12)
    assert n2["calibration_frames"] == 0 and {k: v for k, v in n.items() if k != "calibration_frames"} == \
        {k: v for k, v in n2.items() if k != "calibration_frames"}
    assert m.scales == m2.scales and len(m.scales) == 38 and m.scales["bevdet.dn.dcn"] > 0
    a = m.forward_calibrated(built["img"], built["calib"])
    b = m2.forward_calibrated(built["img"], built["calib"])
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(_bits(p), _bits(q)), name


def test_model_gate(built):
    """At each head output: rms(int8 kernels - fp32 plain path) <= 1.25 rms(fake-quant statement - fp32 plain path)."""
    model, x = built["model"], built["x"]
    mlp = built["mlp"].reshape(-1, 27)
    got = model.bev_half_calibrated(x, built["calib"])
    fq = model.fake_quant_reference(x, built["ranks"], mlp)
    ref = model.fake_quant_reference(x, built["ranks"], mlp, quantize=False)
    rows = []
    for name, g, f, r in zip(NAMES, got, fq, ref):
        e_k, e_f = _rms(g.float(), r), _rms(f, r)
        scale = max(1.0, float(r.abs().max()))
        print(f"{name}: rms error kernels {e_k:.4e}, fake-quant statement {e_f:.4e}, ratio {e_k / e_f:.3f}; max error "
              f"{float((g.float() - r).abs().max()):.3e} (the fp16 model's bar {3e-2 * scale:.3e}), |ref| max {scale:.3f}")
        rows.append((name, e_k, e_f))
    for name, e_k, e_f in rows:
        assert e_f > 0 and e_k <= 1.25 * e_f, name


def _replay_dcn(args, out):
    """The recorded deform_conv2d_q_nhwc call against the numpy statement of tests/util_deform_conv_s8.py."""
    x_q, sx, om, w, ws, bias, groups, _, s_out = args
    assert bias is None and out.dtype == torch.int8
    host = lambda t: t.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    s64 = D.column_s64(host(x_q), host(om))
    near = float(D.near_tie(s64).mean())
    assert near <= D.NEAR_TIE_CAP
    lo, hi = D.column_interval(s64)
    wq = w.cpu().numpy()
    wp, wn = np.maximum(wq, 0), np.minimum(wq, 0)
    acc_min = D.sums(lo, wp, groups) + D.sums(hi, wn, groups)
    acc_max = D.sums(hi, wp, groups) + D.sums(lo, wn, groups)
    wsn = ws.cpu().numpy()
    _, _, o_lo, _ = D.linear_interval(acc_min, sx, 1.0, wsn, None, 0, s_out)
    t, _, _, o_hi = D.linear_interval(acc_max, sx, 1.0, wsn, None, 0, s_out)
    got = host(out)
    share = S.check_interval(got, o_lo, o_hi)
    live = float(D.positions(host(om), *s64.shape[1:3])[2].mean())
    assert got.any() and 0.5 < live < 1.0 and float(np.abs(t).max()) > 50        # the layer's own scale is in use
    return (f"{near:.2e} of the column within EPS of a half-integer, {float((acc_min != acc_max).mean()):.3%} of the sums "
            f"admit a range, {share:.4%} of the outputs two bytes; {live:.1%} of the taps live")


def test_every_call_of_a_forward_against_its_own_statement(built):
    """tests/test_bevdepth_int8_gpu.py's replay with the layer: one eager run on a recording operator set (every read's
    scale asserted as it happens), then EVERY recorded call against its own statement."""
    import test_bevdepth_int8_gpu as TB
    import test_bevdet_int8_gpu as TI
    from bevformer_tensorrt_amd.functions import dispatch
    model, x, ranks = built["model"], built["x"], built["ranks"]
    mlp = built["mlp"].reshape(-1, 27)
    table = model.operands()
    rec = TC.ScaleRecorder(model.bev_ops, keep_calls=True)
    rb, rd, rf, ist, il = ranks
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)
    live = {}
    with dispatch.using(rule=True):
        packed = model.run(x, pool, table, rec, tensors=live, mlp_input=mlp)
    torch.cuda.synchronize()
    rec.check()
    assert packed.shape == (1, 32, 128, 128) and packed.dtype == torch.float16
    assert sorted(n for n, t in live.items() if t.dtype != torch.int8) == \
        ["depth_net", "dn.dcn.om", "dn.feat_cols", "dn.image_bias", "dn.rows", "head.packed", "x.f16"]
    assert tuple(live["dn.dcn.om"].shape) == (6, 24, 16, 44) and not live["dn.dcn.om"][:, 18:].any()   # exact zero pad rows
    std = float(live["dn.dcn.om"][:, :18].float().std())
    print(f"offset standard deviation on the frame: {std:.3f} pixels")
    assert 0.8 <= std <= 1.25
    counts, dilations, convs = {}, [], 0
    for name, args, kwargs, out in rec.calls:
        counts[name] = counts.get(name, 0) + 1
        own = name in ("se_gate2_nhwc_q", "global_avgpool_nhwc_q", "lss_camera_gate", "dense_auto")
        if name == "conv_slice_q_taps":
            convs += 1
            own = convs <= 15                                   # the DepthNet's convolutions come first
            if own:
                dilations.append(kwargs["dilation"])
            else:
                assert kwargs["dilation"] == 1 and kwargs["image_bias"] is None
        if name == "deform_conv2d_q_nhwc":
            assert convs == 14 and args[2] is live["dn.dcn.om"]      # behind the offset convolution, on its rows
            line = _replay_dcn(args, out)
        else:
            line = TB._replay_depthnet(name, args, kwargs, out) if own else TI._replay(name, args, kwargs, out, ranks)
        shape = tuple(out[0].shape) if isinstance(out, tuple) else tuple(out.shape)
        print(f"{name} {shape}: {line}")
    assert counts == dict(quantize_rows=1, lss_camera_gate=1, conv_slice_q_taps=37, se_gate2_nhwc_q=1,
                          global_avgpool_nhwc_q=1, dense_auto=2, deform_conv2d_q_nhwc=1, lss_depth_split_q=1,
                          bev_pool_v2_int8=1, upsample_bilinear_nhwc_q=2)
    assert dilations == [1] * 8 + [1, 6, 12, 18] + [1, 1, 1]
    got = model.bev_half_calibrated(x, built["calib"])
    for (a, b), o in zip(table["slices"], got):
        assert torch.equal(_bits(packed[:, a:b]), _bits(o))


def test_one_int8_deformable_launch_and_no_fp16_one(built):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    ops = _CountingOps()
    model = DI.Int8BEVDepth(built["fp"], built["model"].scales, ops=ops)
    x, calib = built["x"], built["calib"]
    want = built["model"].bev_half_calibrated(x, calib)
    model.bev_half_calibrated(x, calib)
    ops.active = True
    got = model.bev_half_calibrated(x, calib)
    ops.active = False
    torch.cuda.synchronize()
    print("int8 BEVDepth with the DCN layer behind image_features:", ops.calls)
    assert ops.calls["deform_conv2d_q_nhwc"] == 1 and ops.calls["conv_slice_q_taps"] == 37
    for name in ("deform_conv2d_nhwc", "deform_conv2d", "conv_offset_nhwc", "modulated_deformable_conv2d",
                 "modulated_deformable_conv2d_nhwc", "conv_slice_nhwc", "conv_nhwc"):
        assert name not in ops.calls, name
    for n, a, b in zip(NAMES, got, want):
        assert torch.equal(_bits(a), _bits(b)), n
    # no framework glue either
    probe = TD._Probe()
    probe.active = True
    with probe:
        built["model"].bev_half_calibrated(x, calib)
    torch.cuda.synchronize()
    assert probe.counts == dict(conv2d=0, interpolate=0, cat=0, adaptive_avg_pool2d=0, contiguous=0)


def test_replay_batch_one_and_step_raw(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img, calib = built["model"], built["img"], built["calib"]
    a = [o.clone() for o in model.forward_calibrated(img, calib)]
    runner = BEVDetRunner(model, "cuda", graph=True)
    for _ in range(2):
        out = runner.step(img, *built["rigs"][0])
    torch.cuda.synchronize()
    assert runner._graph is not None
    for name, p, q in zip(NAMES, a, out[:6]):
        assert torch.equal(_bits(p), _bits(q)), name
        assert p.dtype == torch.float16 and p.shape[2:] == (128, 128)
    c = model(img, *built["ranks"], built["mlp"])                 # the ranks as inputs (`forward`) pool the same sums
    for name, p, q in zip(NAMES, a, c):
        assert torch.equal(_bits(p), _bits(q)), name
    assert float(a[5].float().abs().max()) > 0
    s2e, _, k, _, _, bda = built["rigs"][0]
    raw = torch.randint(0, 256, (6, 900, 1600, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    eager = BEVDetRunner(model, "cuda", graph=False, raw_size=(900, 1600)).step_raw(raw, s2e, None, k, bda)
    eager = [o.clone() for o in eager]
    runner = BEVDetRunner(model, "cuda", graph=True, raw_size=(900, 1600))
    for _ in range(2):
        out = runner.step_raw(raw, s2e, None, k, bda)
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, eager, out):
        assert torch.equal(_bits(p), _bits(q)), name
    assert float(out[5].float().abs().max()) > 0


def test_replay_batch_two(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, imgs, rigs = built["model"], built["imgs"], built["rigs"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True, batch=2)
    pair = TD._batched(rigs[:2])
    out = [o.clone() for o in runner.step(imgs, *pair)]
    calib2 = model.view.calibration_matrices_batched(*pair).cuda()
    eager = model.forward_calibrated(imgs, calib2)
    torch.cuda.synchronize()
    assert runner._graph is not None
    for n, a, b in zip(NAMES, out, eager):
        assert a.shape[0] == 2 and torch.equal(_bits(a), _bits(b)), n
    assert not torch.equal(out[5][0], out[5][1])


def test_capture_guard_and_weight_reload(built):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    fp = _build(BEVDEPTH_R50_DCN, "hip", torch.float16, state=built["fp"].state_dict())
    model = DI.Int8BEVDepth(fp, built["model"].scales)
    x, calib = built["x"], built["calib"]
    scratch = torch.zeros(8, device="cuda")
    assert model.operands(build=False) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.bev_half_calibrated(x, calib)                      # raises before it launches anything
        with pytest.raises(RuntimeError):
            model.prepare_bev_half()
    del graph
    assert model.operands(build=False) is None                       # nothing was built inside the capture
    eager = [o.clone() for o in model.bev_half_calibrated(x, calib)]
    t0 = model.operands(build=False)
    assert t0 is not None
    for n, a, b in zip(NAMES, eager, built["model"].bev_half_calibrated(x, calib)):
        assert torch.equal(_bits(a), _bits(b)), n                    # the same weights and scales: the same bits
    # a reload that changes conv_offset.bias alone: every tap moves two pixels down -- the operands are rebuilt
    sd = {k: v.clone() for k, v in fp.state_dict().items()}
    sd["view.depth_net.depth_conv.4.conv_offset.bias"][0::2] += 2.0
    fp.load_state_dict(sd)
    assert model.operands(build=False) is None                       # stale
    moved = [o.clone() for o in model.bev_half_calibrated(x, calib)]
    t1 = model.operands(build=False)
    assert t1 is not None and t1 is not t0
    assert not torch.equal(t1["dn.dcn.offset"][2], t0["dn.dcn.offset"][2]) and torch.equal(t1["dn.dcn"][0], t0["dn.dcn"][0])
    assert not torch.equal(moved[5], eager[5])
    # ... and one that changes the deformable weight alone
    sd["view.depth_net.depth_conv.4.weight"] = sd["view.depth_net.depth_conv.4.weight"].flip(0)
    fp.load_state_dict(sd)
    assert model.operands(build=False) is None
    again = model.bev_half_calibrated(x, calib)
    t2 = model.operands(build=False)
    assert torch.equal(t2["dn.dcn"][0], t1["dn.dcn"][0].flip(0)) and not torch.equal(again[5], moved[5])
