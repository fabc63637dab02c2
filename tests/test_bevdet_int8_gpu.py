"""quantization.build_int8_bevdet(bev_half="int8") on the GPU: the synthetic BEVDet(seed=0), min-max calibration on two
random frames with the calibration of golden("bevdet_geometry").

* every call of one forward of the BEV half replayed against its own float64 statement from the operands the kernel
  actually received: the quantise pass and the pooling exactly, the convolutions exactly outside the derived near-tie
  interval of tests/util_centernet_int8.py, the two new launches (csrc/lss_split_s8.hip) under the interval rule of
  tests/util_lss_split_s8.py; every int8 tensor read with the scale it was written with;
* the model gate: rms error of the six head outputs against the fp32 plain path on the same weights at most 1.25 x that
  of the fp32 fake-quant statement of the same plan (the project's gate for a chain whose every layer is in the
  statement: the softmax quantisation and the pooling's integer sums are stated exactly).  The absolute errors against
  the fp16 model's 3e-2 bar are printed, not gated (synthetic weights, min-max scales);
* eager / eager / BEVDetRunner replay bit equality with get_bboxes in the graph, the probes (no framework glue, no fp16
  tensor inside the BEV half but depth_net's logits), the capture guard and the weight reload, the cache rebuild, and
  the fp16 BEVDet(bev_half="hip") and the default build_int8_bevdet model keeping their bits."""
import numpy as np
import pytest
import torch

import test_bevdet_bev_half_gpu as TB
import util_bevdet_int8 as U
import util_lss_split_s8 as L
from conftest import golden

pytestmark = pytest.mark.gpu

NAMES = TB.NAMES


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _by_rule(model, *args):
    """A frame with the dense / convolution dispatch by rule: the measured table's library convolutions are not
    run-to-run reproducible on the MI355X (bevdet.BEVDet.forward_calibrated), so bits are compared under the rule."""
    from bevformer_tensorrt_amd.functions import dispatch
    with dispatch.using(rule=True):
        return model(*args)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from bevformer_tensorrt_amd.bevdet import BEVDet
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    g = golden("bevdet_geometry")
    t = lambda k: torch.from_numpy(g[k])
    fp = BEVDet(seed=0, bev_half="hip").cuda().half()
    geom = (t("sensor2ego"), None, t("cam2imgs"), t("post_rots"), t("post_trans"), t("bda"))
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*geom)]
    calib = fp.view.calibration_matrices(*geom).cuda()
    gen = torch.Generator().manual_seed(1)
    img = torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half()
    frames = [(torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks) for _ in range(2)]
    hip_before = [o.clone() for o in fp.forward_calibrated(img, calib)]
    default, _, _ = build_int8_bevdet(fp, "cuda", frames, "minmax")
    default(img, *ranks)                 # (a frame in front of the two that are compared: the dispatch's choices are made)
    default_before = [o.clone() for o in _by_rule(default, img, *ranks)]
    cache = str(tmp_path_factory.mktemp("calib") / "bevdet.calib")
    model, qops, note = build_int8_bevdet(fp, "cuda", frames, "minmax", bev_half="int8", calibration_cache=cache)
    again, _, note2 = build_int8_bevdet(fp, "cuda", [], "minmax", bev_half="int8", calibration_cache=cache)
    x = model._features(img).clone()
    return dict(fp=fp, geom=geom, ranks=ranks, calib=calib, img=img, hip_before=hip_before, default=default,
                default_before=default_before, model=model, note=note, again=again, note2=note2, x=x)


def test_notes_and_the_cache_rebuild(built):
    n, n2 = built["note"], built["note2"]
    assert (n["bev_half"], n["int8_bev_half_layers"], n["bev_half_scale_sites"], n["calibration_frames"]) == ("int8", 24, 26, 2)
    assert n2["calibration_frames"] == 0 and {k: v for k, v in n.items() if k != "calibration_frames"} == \
        {k: v for k, v in n2.items() if k != "calibration_frames"}
    m, m2 = built["model"], built["again"]
    assert m.scales == m2.scales and len(m.scales) == 26
    assert m.fp.int8_chain.s_stem == m2.fp.int8_chain.s_stem
    a = m.forward_calibrated(built["img"], built["calib"])
    b = m2.forward_calibrated(built["img"], built["calib"])
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(_bits(p), _bits(q)), name


def test_the_other_models_keep_their_bits(built):
    for name, a, b in zip(NAMES, built["hip_before"], built["fp"].forward_calibrated(built["img"], built["calib"])):
        assert torch.equal(_bits(a), _bits(b)), name
    for name, a, b in zip(NAMES, built["default_before"], _by_rule(built["default"], built["img"], *built["ranks"])):
        assert torch.equal(_bits(a), _bits(b)), name


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _replay(name, args, kwargs, out, ranks):
    """One recorded call against its float64 statement.  -> a line for the log."""
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    if name == "conv_slice_q_taps":
        x, sx, w, ws, b, act, res, sres, stride, _, sout, odt = args
        assert kwargs["res_first"] == (res is not None)
        acc = U.conv_sums(x, w, stride)
        t = U.epilogue_interval(acc, sx, ws, b, None if res is None else _nhwc(res), sres, act == "relu",
                                sout if odt == torch.int8 else None)
        share, off = U.check_output(_nhwc(out), *t)
        return f"{share:.4%} within delta of a boundary, {off:.4%} differ from the rounding"
    if name == "quantize_rows":
        x, s = args
        inv = x.float() / torch.tensor(s, dtype=torch.float32, device=x.device)
        assert torch.equal(out, inv.round().clamp(-127, 127).to(torch.int8))
        return "exact"
    if name == "bev_pool_v2_int8":
        d, f, rd, rf, rb, ist, il, sd, sf, so, h, w = args
        f32 = lambda s: torch.tensor(s, dtype=torch.float32)
        want = BI.pool_statement(d, f, (rb, rd, rf), float(f32(sd) * f32(sf) / f32(so)), h * w)
        assert torch.equal(out.view(h * w, -1), want.to(torch.int8)) and bool(out.any())
        return "exact"
    if name == "lss_depth_split_q":
        x, n, D, C, doff, foff, sd, sf = args
        dq, fq = out
        xn = x.cpu().numpy()
        logits = xn[:, doff:doff + D]
        t, eps = L.depth_statement(logits, sd), L.depth_eps(logits, D)
        got = dq.reshape(n, D, -1).permute(0, 2, 1).reshape(-1, D).cpu().numpy()
        assert L.interval_ok(got, t, eps).all()
        tf = L.feat_statement(xn[:, foff:foff + C], sf).astype(np.float32).astype(np.float64)
        assert np.array_equal(fq.reshape(-1, C).cpu().numpy(), L.saturate(tf).astype(np.int8))
        return (f"eps {eps:.2e}, near-tie share {L.near_tie_share(t, eps):.2e}, {int((got != L.saturate(t)).sum())} of "
                f"{t.size} depth bytes differ from the rounding")
    b, sb, so = args
    bn = _nhwc(b).cpu().numpy()
    assert bn.min() >= 0                                   # behind a ReLU: the relative interval rule applies
    h, w = out.shape[2:]
    t, eps = L.upsample_statement(bn, h, w, L.f32_ratio(sb, so)), L.upsample_eps(h, w)
    got = _nhwc(out).cpu().numpy()
    assert L.interval_ok(got, t, eps).all()
    return f"eps {eps:.2e}, near-tie share {L.near_tie_share(t, eps):.2e}, {int((got != L.saturate(t)).sum())} of {t.size} bytes differ from the rounding"


def test_every_call_of_a_forward_against_its_own_statement(built):
    import bevformer_tensorrt_amd.functions as fn
    model, ranks = built["model"], built["ranks"]
    rb, rd, rf, ist, il = ranks
    rec = U.ScaleRecorder(fn, keep_calls=True)
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)
    live = {}
    packed = model.run(built["x"], pool, model.operands(), rec, tensors=live)      # (every read's scale is asserted as it happens)
    torch.cuda.synchronize()
    rec.check()
    assert packed.shape == (1, 32, 128, 128) and packed.dtype == torch.float16
    # no fp16 tensor between the quantisation of x and the packed output other than depth_net's logits
    assert sorted(n for n, t in live.items() if t.dtype != torch.int8) == ["depth_net", "head.packed", "x.f16"]
    counts = {}
    for name, args, kwargs, out in rec.calls:
        counts[name] = counts.get(name, 0) + 1
        line = _replay(name, args, kwargs, out, ranks)
        shape = tuple(out[0].shape) if isinstance(out, tuple) else tuple(out.shape)
        print(f"{name} {shape}: {line}")
    assert counts == dict(quantize_rows=1, conv_slice_q_taps=23, lss_depth_split_q=1, bev_pool_v2_int8=1,
                          upsample_bilinear_nhwc_q=2)
    # the indirect pooling of the calibrated path gives the same packed bits
    got = model.bev_half_calibrated(built["x"], built["calib"])
    for (a, b), o in zip(model.operands()["slices"], got):
        assert torch.equal(_bits(packed[:, a:b]), _bits(o))


def test_model_gate(built):
    model, x = built["model"], built["x"]
    got = model.bev_half_calibrated(x, built["calib"])
    fq = model.fake_quant_reference(x, built["ranks"])
    ref = model.fake_quant_reference(x, built["ranks"], quantize=False)
    rows = []
    for name, g, f, r in zip(NAMES, got, fq, ref):
        e_k, e_f = _rms(g.float(), r), _rms(f, r)
        scale = max(1.0, float(r.abs().max()))
        print(f"{name}: rms error kernels {e_k:.4e}, fake-quant statement {e_f:.4e}, ratio {e_k / e_f:.3f}; max error "
              f"{float((g.float() - r).abs().max()):.3e} (the fp16 model's bar {3e-2 * scale:.3e}), |ref| max {scale:.3f}")
        rows.append((name, e_k, e_f))
    for name, e_k, e_f in rows:
        assert e_f > 0 and e_k <= 1.25 * e_f, name


def test_two_runs_and_the_replay_give_equal_bits(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img, calib = built["model"], built["img"], built["calib"]
    a = [o.clone() for o in model.forward_calibrated(img, calib)]
    b = model.forward_calibrated(img, calib)
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(_bits(p), _bits(q)), name
        assert p.dtype == torch.float16 and p.shape[2:] == (128, 128)
    boxes = model.get_bboxes(b, padded=True)
    runner = BEVDetRunner(model, "cuda", graph=True, post="bboxes")
    for _ in range(2):
        out = runner.step(img, *built["geom"])
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, a, out[:6]):
        assert torch.equal(_bits(p), _bits(q)), name
    for name, p, q in zip(("boxes", "scores", "labels", "count", "index"), boxes, out[6:]):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), name
    # the ranks as inputs (`forward`) pool the same sums
    c = model(img, *built["ranks"])
    for name, p, q in zip(NAMES, a, c):
        assert torch.equal(_bits(p), _bits(q)), name


def test_step_raw_replays_to_the_eager_bits(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model = built["model"]
    s2e, _, k, _, _, bda = built["geom"]
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


def test_no_framework_glue_in_the_bev_half(built):
    from bevformer_tensorrt_amd.functions import conv as C
    model, x, calib = built["model"], built["x"], built["calib"]
    model.bev_half_calibrated(x, calib)
    misses = list(C.CONV_MISSES)
    probe = TB._Probe()
    probe.active = True
    with probe:
        model.bev_half_calibrated(x, calib)
    torch.cuda.synchronize()
    print("int8 BEV half:", probe.counts)
    assert probe.counts == dict(conv2d=0, interpolate=0, cat=0, softmax=0, contiguous=0)
    assert C.CONV_MISSES == misses
    probe = TB._Probe()
    probe.active = True
    with probe:
        model.fake_quant_reference(x, built["ranks"])          # the probe sees the torch statement
    assert probe.counts["conv2d"] >= 23 and probe.counts["interpolate"] >= 2 and probe.counts["softmax"] >= 1


def test_capture_guard_and_weight_reload(built):
    from bevformer_tensorrt_amd.bevdet import BEVDet
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    fp = BEVDet(seed=3).cuda().half()
    model = BI.Int8BEVDet(fp, built["model"].scales)
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
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [o.clone() for o in model.bev_half_calibrated(x, calib)]
    torch.cuda.current_stream().wait_stream(s)
    t0 = model.operands(build=False)
    assert t0 is not None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = model.bev_half_calibrated(x, calib)
    graph.replay()
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, outs, eager):
        assert torch.equal(_bits(a), _bits(b)), n
    del graph, outs
    # new head weights: height's final convolution becomes the constant 0.5, every other head keeps its bits
    with torch.no_grad():
        fp.heads["height"][1].weight.zero_()
        fp.heads["height"][1].bias.fill_(0.5)
    assert model.operands(build=False) is None                       # stale
    new = model.bev_half_calibrated(x, calib)
    assert model.operands(build=False) is not t0
    for n, a, b in zip(NAMES, new, eager):
        if n == "height":
            assert bool((a == 0.5).all())
        else:
            assert torch.equal(_bits(a), _bits(b)), n
    with pytest.raises(ValueError):
        model.bev_half_calibrated(x.float(), calib)
