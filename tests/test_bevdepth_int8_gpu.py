"""The INT8 BEVDepth (bevformer_tensorrt_amd/bevdepth_int8.py; quantization.build_int8_bevdet(<BEVDepth model>,
bev_half="int8")) on the model of tests/test_bevdepth_gpu.py's frame: synthetic weights, two min-max calibration frames,
one build per module (and one rebuild from the calibration cache).

* THE MODEL GATE, the project's bar for an INT8 build: at each of the six head outputs the rms error of the int8 kernels
  against the fp32 plain path is <= 1.25 x the fake-quant statement's (`fake_quant_reference`: gate quantisation, the
  average pool and the image-bias rounding are in the statement).  Absolute errors against the fp16 model's 3e-2 bar
  are printed, not gated.
* every call of the DepthNet in one forward against its own float64 / interval / numpy statement;
* replay bit-equal to the eager run through BEVDetRunner at batch 1 (get_bboxes in the graph, step_raw) and batch 2; a
  changed calibration -- the MLP part alone included -- is followed without a new capture; a sample keeps its bits when its
  neighbour is replaced; the capture guard; a weight reload rebuilds the operands; the cache rebuild gives the same
  scales without running a frame; no framework glue behind image_features;
* the fp16 BEVDepth frame and Int8BEVDet on the default model keep the bits a build of the parent commit gave on the
  same GPU."""
import pytest
import torch
import torch.nn.functional as F

import test_bevdepth_gpu as TD

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
    fp = TD._build("hip", torch.float16)
    rigs = [jittered_rig(fp.view, k) for k in (1, 2, 3)]
    rig = rigs[0]
    ranks = [r.cuda() for r in fp.view.get_bev_pool_input(*rig)]
    mlp = fp.view.get_mlp_input(*rig).cuda()
    calib = fp.view.calibration_matrices(*rig).cuda()
    gen = torch.Generator().manual_seed(1)
    imgs = torch.randn(2, 6, 3, 256, 704, generator=gen).cuda().half()
    frames = [(torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks, mlp) for _ in range(2)]
    cache = str(tmp_path_factory.mktemp("calib") / "bevdepth.calib")
    model, qops, note = build_int8_bevdet(fp, "cuda", frames, "minmax", bev_half="int8", calibration_cache=cache)
    again, _, note2 = build_int8_bevdet(fp, "cuda", [], "minmax", bev_half="int8", calibration_cache=cache)
    x = model._features(imgs[:1]).clone()
    return dict(fp=fp, rigs=rigs, ranks=ranks, mlp=mlp, calib=calib, imgs=imgs, img=imgs[:1], model=model, note=note,
                again=again, note2=note2, x=x)


def test_notes_and_the_cache_rebuild(built):
    from bevformer_tensorrt_amd.bevdepth_int8 import Int8BEVDepth
    n, n2 = built["note"], built["note2"]
    assert type(built["model"]) is Int8BEVDepth
    assert (n["bev_half"], n["int8_bev_half_layers"], n["bev_half_scale_sites"], n["calibration_frames"]) == ("int8", 37, 37, 2)
    assert (n["depthnet_int8_layers"], n["depthnet_scale_sites"]) == (14, 11)
    assert n2["calibration_frames"] == 0 and {k: v for k, v in n.items() if k != "calibration_frames"} == \
        {k: v for k, v in n2.items() if k != "calibration_frames"}
    m, m2 = built["model"], built["again"]
    assert m.scales == m2.scales and len(m.scales) == 37
    a = m.forward_calibrated(built["img"], built["calib"])
    b = m2.forward_calibrated(built["img"], built["calib"])
    for name, p, q in zip(NAMES, a, b):
        assert torch.equal(_bits(p), _bits(q)), name


def test_model_gate(built):
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


def _dilated_sums(x_q, w_q_taps, d):
    """tests/util_bevdet_int8.py's conv_sums (stride 1) at dilation d: exact integer sums, float64 [B, H, W, Cout]."""
    cout, k, _, cin = w_q_taps.shape
    B, _, H, W = x_q.shape
    cols = F.unfold(x_q.double().contiguous(), k, dilation=d, padding=(k // 2) * d)
    wm = w_q_taps.permute(0, 3, 1, 2).reshape(cout, cin * k * k).double()
    return torch.matmul(wm, cols).view(B, cout, H, W).permute(0, 2, 3, 1)


U32 = 2.0 ** -24


def _camera_gate_interval(v, packed, mid):
    """The documented order of bevops_lss_camera_gate on the packed block in float64 with a forward error bound: a layer
    is a chain of kdim fmas and one addition, (kdim + 1) roundings -> (kdim + 1) u (|in| |W| + |b|) (1.01 for the higher
    orders) on top of the incoming error through |W|; ReLU is 1-Lipschitz; the sigmoid's slope is at most 1/4 and its own
    evaluation stays under 2^-17 relative (tests/test_lss_depthnet_gpu.py's sigmoid_bound).  -> (gates, bound) [2, n, mid]."""
    import numpy as np
    import test_lss_depthnet_gpu as TG
    words = TG.branch_words(mid)
    gates, bounds = [], []
    for br in (0, 1):
        q, at = packed[br * words:(br + 1) * words].astype(np.float64), 0
        h, e = v.astype(np.float64), 0.0
        for li, kdim in enumerate((27, mid, mid, mid)):
            w, b = q[at:at + kdim * mid].reshape(kdim, mid), q[at + kdim * mid:at + kdim * mid + mid]
            at += kdim * mid + mid
            e = e @ np.abs(w) + 1.01 * (kdim + 1) * U32 * (np.abs(h) @ np.abs(w) + np.abs(b)) if li else \
                1.01 * (kdim + 1) * U32 * (np.abs(h) @ np.abs(w) + np.abs(b))
            h = h @ w + b
            if li in (0, 2):
                h = np.maximum(h, 0)
        g = 1 / (1 + np.exp(-h))
        gates.append(g)
        bounds.append(0.25 * e + TG.sigmoid_bound(g) + U32 * g)      # (+ the result's own rounding to fp32)
    return np.stack(gates), np.stack(bounds)


def _replay_depthnet(name, args, kwargs, out):
    """One recorded call of an entry that bevdet_int8's plan does not have, against its own statement.  -> a log line."""
    import util_bevdet_int8 as U
    import util_lss_depthnet_s8 as UL
    host = lambda t: t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).cpu().numpy()
    if name == "conv_slice_q_taps":          # the statement of tests/util_bevdet_int8.py with the dilation and the image bias
        x_q, sx, w, ws, bias, act, res, sres, stride, _, s_out, odt = args
        d, ib = kwargs["dilation"], kwargs["image_bias"]
        assert stride == 1 and kwargs["res_first"] == (res is not None) and (ib is None) != (bias is None)
        acc = _dilated_sums(x_q, w, d)
        b = bias if ib is None else ib[:, None, None, :w.shape[0]]
        t = U.epilogue_interval(acc, sx, ws, b, None if res is None else res.permute(0, 2, 3, 1), sres, act == "relu",
                                s_out if odt == torch.int8 else None)
        share, off = U.check_output(out.permute(0, 2, 3, 1), *t)
        return (f"dilation {d}{', image bias' if ib is not None else ''}: {share:.4%} within delta of a boundary, {off:.4%} "
                f"differ from the rounding")
    if name == "se_gate2_nhwc_q":
        x_q, sx, gates, sa, sb = args
        gn = gates.cpu().numpy()
        assert (host(out[0]) == UL.gate_statement(host(x_q), sx, gn[0], sa)).all()
        assert (host(out[1]) == UL.gate_statement(host(x_q), sx, gn[1], sb)).all() and bool(out[0].any()) and bool(out[1].any())
        return "exact"
    if name == "global_avgpool_nhwc_q":
        x_q, sx = args
        want = UL.pool_statement(host(x_q), sx)
        assert (out.cpu().numpy().view("int16") == want.view("int16")).all() and want.any()
        return "exact"
    if name == "lss_camera_gate":
        v, packed, mid = args
        g, bound = _camera_gate_interval(v.cpu().numpy(), packed.cpu().numpy(), mid)
        err = abs(out.double().cpu().numpy() - g)
        assert (err <= bound).all() and g.std() > 0.02
        return f"max err / bound {(err / bound).max():.3f}"
    assert name == "dense_auto"
    x, w, b, res, relu = args                 # fp16 operands, fp32 sums in some order, bias, one rounding to binary16
    assert res is None
    K = x.shape[1]
    y = x.double() @ w.double().t() + b.double()
    e = 1.01 * (K + 2) * U32 * (x.double().abs() @ w.double().abs().t() + b.double().abs())
    act = (lambda a: a.clamp(min=0.0)) if relu else (lambda a: a)
    lo, hi, g = act(y - e).half().double(), act(y + e).half().double(), out.double()
    assert bool(((g >= lo) & (g <= hi)).all()) and bool(out.any())
    return f"{float((lo != hi).double().mean()):.4%} of the outputs admit two roundings"


def test_every_call_of_a_forward_against_its_own_statement(built):
    """One eager run on a recording operator set (every read's scale is asserted as it happens), then EVERY recorded call
    against its own statement: the entries bevdet_int8's plan has through tests/test_bevdet_int8_gpu.py's `_replay` -- the
    quantise pass, the 22 BEV-half convolutions, the softmax + split (which here reads the row buffer two fp16-out int8
    convolutions wrote), the pooling, the two up-samplers -- and the DepthNet's own through `_replay_depthnet`: its 14
    convolutions with the dilation and the per-image bias in the statement, the camera gates, both gated copies, the
    average pool and the pooled branch's two GEMMs."""
    import test_bevdet_int8_gpu as TI
    import util_bevdepth_int8 as UD
    from bevformer_tensorrt_amd.functions import dispatch
    model, x, ranks = built["model"], built["x"], built["ranks"]
    mlp = built["mlp"].reshape(-1, 27)
    table = model.operands()
    rec = UD.ScaleRecorder(model.bev_ops, keep_calls=True)
    rb, rd, rf, ist, il = ranks
    pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)
    live = {}
    with dispatch.using(rule=True):
        packed = model.run(x, pool, table, rec, tensors=live, mlp_input=mlp)
    torch.cuda.synchronize()
    rec.check()
    assert packed.shape == (1, 32, 128, 128) and packed.dtype == torch.float16
    # no fp16 tensor behind the quantisation of x other than the row buffer (and its two views), the pooled branch's
    # per-image bias and the packed output
    assert sorted(n for n, t in live.items() if t.dtype != torch.int8) == \
        ["depth_net", "dn.feat_cols", "dn.image_bias", "dn.rows", "head.packed", "x.f16"]
    counts, dilations, convs = {}, [], 0
    for name, args, kwargs, out in rec.calls:
        counts[name] = counts.get(name, 0) + 1
        own = name in ("se_gate2_nhwc_q", "global_avgpool_nhwc_q", "lss_camera_gate", "dense_auto")
        if name == "conv_slice_q_taps":
            convs += 1
            own = convs <= 14                                   # the DepthNet's convolutions come first
            if own:
                dilations.append(kwargs["dilation"])
            else:
                assert kwargs["dilation"] == 1 and kwargs["image_bias"] is None
        line = _replay_depthnet(name, args, kwargs, out) if own else TI._replay(name, args, kwargs, out, ranks)
        shape = tuple(out[0].shape) if isinstance(out, tuple) else tuple(out.shape)
        print(f"{name} {shape}: {line}")
    assert counts == dict(quantize_rows=1, lss_camera_gate=1, conv_slice_q_taps=36, se_gate2_nhwc_q=1,
                          global_avgpool_nhwc_q=1, dense_auto=2, lss_depth_split_q=1, bev_pool_v2_int8=1,
                          upsample_bilinear_nhwc_q=2)
    assert dilations == [1] * 8 + [1, 6, 12, 18] + [1, 1]
    # the indirect pooling of the calibrated path gives the same packed bits
    got = model.bev_half_calibrated(x, built["calib"])
    for (a, b), o in zip(table["slices"], got):
        assert torch.equal(_bits(packed[:, a:b]), _bits(o))


def test_replay_batch_one_with_bboxes_and_forward(built):
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
        out = runner.step(img, *built["rigs"][0])
    torch.cuda.synchronize()
    for name, p, q in zip(NAMES, a, out[:6]):
        assert torch.equal(_bits(p), _bits(q)), name
    for name, p, q in zip(("boxes", "scores", "labels", "count", "index"), boxes, out[6:]):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), name
    c = model(img, *built["ranks"], built["mlp"])                 # the ranks as inputs (`forward`) pool the same sums
    for name, p, q in zip(NAMES, a, c):
        assert torch.equal(_bits(p), _bits(q)), name
    assert float(a[5].float().abs().max()) > 0


def test_a_changed_calibration_is_followed_without_a_new_capture(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img, rigs = built["model"], built["img"], built["rigs"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True)
    eager = BEVDetRunner(model, torch.device("cuda"), graph=False)
    seen = []
    for rig in rigs:
        out = runner.step(img, *rig)
        want = eager.step(img, *rig)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, out, want):
            assert torch.equal(_bits(a), _bits(b)), n
        seen.append(out[5].clone())
    graph = runner._graph
    assert graph is not None and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    host = model.view.calibration_matrices(*rigs[0]).clone()
    host[6 * 24 + 9 + 0] += 25.0                                   # camera 0's fx in the MLP part only: the gate moves
    runner._in["calib"].copy_(host.cuda())
    runner._graph.replay()
    moved = [o.clone() for o in runner._outs]
    plain = model.forward_calibrated(img, host.cuda())
    torch.cuda.synchronize()
    assert runner._graph is graph
    for n, a, b in zip(NAMES, moved, plain):
        assert torch.equal(_bits(a), _bits(b)), n
    assert not torch.equal(moved[5], seen[0])


def test_step_raw_replays_to_the_eager_bits(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model = built["model"]
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


def test_batch_two_and_sample_independence(built):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, imgs, rigs = built["model"], built["imgs"], built["rigs"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True, batch=2)
    pair = TD._batched(rigs[:2])
    out = [o.clone() for o in runner.step(imgs, *pair)]
    calib2 = model.view.calibration_matrices_batched(*pair).cuda()
    assert calib2.shape == (2, 6 * 51 + 9)
    eager = model.forward_calibrated(imgs, calib2)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, out, eager):
        assert a.shape[0] == 2 and torch.equal(_bits(a), _bits(b)), n
    graph = runner._graph
    out_b = [o.clone() for o in runner.step(imgs, *TD._batched([rigs[0], rigs[2]]))]
    torch.cuda.synchronize()
    assert runner._graph is graph
    for n, a, b in zip(NAMES, out, out_b):
        assert torch.equal(_bits(a[0]), _bits(b[0])), n
    assert not torch.equal(out[5][1], out_b[5][1])
    calib_c = model.view.calibration_matrices_batched(*TD._batched([rigs[2], rigs[1]])).cuda()
    out_c = model.forward_calibrated(torch.stack([imgs[1], imgs[1]]), calib_c)
    torch.cuda.synchronize()
    for n, a, c in zip(NAMES, out, out_c):
        assert torch.equal(_bits(a[1]), _bits(c[1])), n
        assert not torch.equal(a[0], c[0])


def test_no_framework_glue_behind_image_features(built):
    from bevformer_tensorrt_amd.functions import conv as C
    model, x, calib = built["model"], built["x"], built["calib"]
    model.bev_half_calibrated(x, calib)
    misses = list(C.CONV_MISSES)
    probe = TD._Probe()
    probe.active = True
    with probe:
        model.bev_half_calibrated(x, calib)
    torch.cuda.synchronize()
    print("int8 BEVDepth behind image_features:", probe.counts)
    assert probe.counts == dict(conv2d=0, interpolate=0, cat=0, adaptive_avg_pool2d=0, contiguous=0)
    assert C.CONV_MISSES == misses
    probe = TD._Probe()
    probe.active = True
    with probe:
        model.fake_quant_reference(x, built["ranks"], built["mlp"].reshape(-1, 27))     # the probe sees the torch statement
    assert probe.counts["conv2d"] >= 36 and probe.counts["interpolate"] >= 2


def test_capture_guard_and_weight_reload(built):
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    fp = TD._build("hip", torch.float16, state=built["fp"].state_dict())
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
    # a reload: the last 1 x 1 of the DepthNet now prefers depth bin 7 everywhere -- the int8 operands are rebuilt
    sd = {k: v.clone() for k, v in fp.state_dict().items()}
    sd["view.depth_net.depth_conv.4.weight"].zero_()
    sd["view.depth_net.depth_conv.4.bias"].zero_()
    sd["view.depth_net.depth_conv.4.bias"][7] = 30.0
    fp.load_state_dict(sd)
    assert model.operands(build=False) is None                       # stale
    live = {}
    ops = model.bev_ops
    rb, rd, rf, ist, il = built["ranks"]
    pool = lambda d, f, s: ops.bev_pool_v2_int8(d, f, rd, rf, rb, ist, il, *s, 128, 128)
    new = model.bev_half_calibrated(x, calib)
    t1 = model.operands(build=False)
    assert t1 is not None and t1 is not t0 and not t1["dn.last"][0].any() and float(t1["dn.last"][2][7]) == 30.0
    model.run(x, pool, t1, ops, tensors=live, mlp_input=built["mlp"].reshape(-1, 27))
    torch.cuda.synchronize()
    # (softmax = 1 in bin 7; the depth scale is at most 1 / 127, so the plane saturates and the other bins are empty)
    assert model.scale("depth") <= 1.0 / 127.0 * (1 + 1e-6)
    assert bool((live["depth"][:, 7] == 127).all()) and not live["depth"][:, :7].any() and not live["depth"][:, 8:].any()
    assert not torch.equal(new[5], eager[5])


# sha-256 (tests/test_bevdepth_gpu.py's frame_digest) of the six maps of the two frames below, taken from a build of
# the PARENT commit on an MI355X: the fp16 BEVDepth path and the int8
# BEV half of the default model keep their launches and their bits (conv_slice_s8.hip, bevdet_int8.py and
# quantization.py were edited)
PARENT_FP16_BEVDEPTH_DIGEST = "f4b1946b2a04acec08a30cc12816940aa75d739eee819d6be101fb699967fc82"
PARENT_INT8_BEVDET_DIGEST = "8a8bde8dd88c3a11971f1994ecccc082b9be4fda54ebf8ece427fa4eeeccef4c"


def fp16_bevdepth_frame():
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    model = TD._build("hip", torch.float16)
    calib = model.view.calibration_matrices(*jittered_rig(model.view, 5)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(3)).cuda().half()
    model.forward_calibrated(img, calib)
    outs = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    return outs


def int8_bevdet_frame():
    """Int8BEVDet around the default fp16 model with scales from a formula (no calibration run: nothing but the plan's
    own kernels decides the bits)."""
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    fp = BEVDet(seed=0, bev_half="hip").cuda().half()
    sites = BI.build_plan(fp).sites
    scales = {s: 0.02 + 0.001 * i for i, s in enumerate(sites)}
    scales["bevdet.depth"] = 1.0 / 127.0
    model = BI.Int8BEVDet(fp, scales)
    calib = fp.view.calibration_matrices(*jittered_rig(fp.view, 5)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(3)).cuda().half()
    model.forward_calibrated(img, calib)
    outs = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    return outs


def test_the_fp16_bevdepth_frame_keeps_the_parent_commits_bits():
    got = TD.frame_digest(fp16_bevdepth_frame())
    print("fp16 BEVDepth frame:", got)
    assert got == PARENT_FP16_BEVDEPTH_DIGEST


def test_int8_bevdet_on_the_default_model_keeps_the_parent_commits_bits():
    outs = int8_bevdet_frame()
    got = TD.frame_digest(outs)
    print("Int8BEVDet frame:", got)
    assert float(outs[5].float().abs().max()) > 0
    assert got == PARENT_INT8_BEVDET_DIGEST
