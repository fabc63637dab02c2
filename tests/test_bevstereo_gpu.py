"""BEVStereo on the GPU (bevformer_tensorrt_amd/bevdepth.py: DepthNet(stereo=True), LSSViewTransformerBEVStereo;
bevdet.BEVSTEREO_R50) at small sizes -- 2 cameras, a 64 x 96 input: DepthNet.forward_hip against the fp32 plain path
at the bar tests/test_bevdepth_gpu.py applies (3e-2 max(1, max |fp32|)), the stereo launches of a forward each
replayed against its own statement, the first frame, and BEVDet(BEVSTEREO_R50-shaped cfg).forward_calibrated eager
against a captured graph, the capture guards, a weight reload, and call probes for torch.cat / grid_sample / softmax."""
import pytest
import torch
import torch.nn.functional as F

import util_stereo as U

pytestmark = pytest.mark.gpu

MID, CTX, D, CST = 32, 16, 11, 16          # DepthNet widths, depth bins, stereo feature channels
H, W = 4, 6                                # the stride-16 map of a 64 x 96 input; the stereo map is 16 x 24


def _randomise(net, gen):
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=gen) * (1.2 / p[0].numel() ** 0.5))
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))
        net.bn.weight.fill_(1.0)
        net.bn.running_var.fill_(1.0)
        net.bn.running_mean.zero_()


def _geometry(n, hc, wc, depth, seed=3):
    from bevformer_tensorrt_amd.bevdet import LSSViewTransformer, jittered_rig
    from bevformer_tensorrt_amd.functions import stereo_calibration, stereo_frustum_tables
    size = (4 * hc, 4 * wc)
    cfg = dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=depth)
    view = LSSViewTransformer(grid_config=cfg, input_size=size, downsample=4, in_channels=32, out_channels=16, ops=object())
    _, _, K, pr, pt, _ = jittered_rig(view, seed, n_cams=n)
    pt[0, :, 0] *= size[1] / 704.0
    k2s = torch.eye(4).repeat(1, n, 1, 1)
    k2s[0, :, :3, 3] = torch.tensor([[0.3, 0.02, 0.1], [-0.2, 0.0, 0.6]])[:n]
    return dict(k2s_sensor=k2s, intrins=K, post_rots=pr, post_trans=pt, frustum=view.frustum,
                consts=stereo_calibration(k2s, K, pr, pt), tables=stereo_frustum_tables(view.frustum))


@pytest.fixture(scope="module")
def nets():
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    g = torch.Generator().manual_seed(4)
    ref = DepthNet(MID, MID, CTX, D, stereo=True, bias=5.0).eval()
    _randomise(ref, g)
    hip = DepthNet(MID, MID, CTX, D, stereo=True, bias=5.0).eval()
    hip.load_state_dict(ref.state_dict())
    hip = hip.cuda().half()
    ref.load_state_dict({k: v.float().cpu() for k, v in hip.state_dict().items()})        # the fp16 weights, in fp32
    geo = _geometry(2, 4 * H, 4 * W, [1.0, 1.0 + D, 1.0])
    x = torch.randn(2, MID, H, W, generator=g).half()
    mlp = 0.5 * torch.randn(2, 27, generator=g)
    prev, curr = U.relu_like((2, CST, 4 * H, 4 * W), g, 0.5), U.relu_like((2, CST, 4 * H, 4 * W), g, 0.5)
    return dict(ref=ref, hip=hip, geo=geo, x=x, mlp=mlp, prev=prev, curr=curr)


def _metas(c, prev=True):
    g = c["geo"]
    return dict(cv_feat_list=[c["prev"] if prev else None, c["curr"]], k2s_sensor=g["k2s_sensor"], intrins=g["intrins"],
                post_rots=g["post_rots"], post_trans=g["post_trans"], frustum=g["frustum"], downsample=16, cv_downsample=4)


class _Recorder:
    """The operator set with every call of the listed functions recorded: (name, args, kwargs, result)."""

    def __init__(self, names):
        from bevformer_tensorrt_amd import functions
        self._f, self._names, self.calls = functions, names, []

    def __getattr__(self, name):
        fn = getattr(self._f, name)
        if name not in self._names:
            return fn

        def wrapped(*a, **k):
            out = fn(*a, **k)
            self.calls.append((name, a, k, out))
            return out
        return wrapped


def _fast(c, ops, prev=True):
    dev = lambda t: t.half().cuda().contiguous(memory_format=torch.channels_last)
    g = c["geo"]
    stereo = (dev(c["prev"]) if prev else None, dev(c["curr"]), g["consts"].cuda(), tuple(t.cuda() for t in g["tables"]))
    from bevformer_tensorrt_amd.bevdet import _rule_dispatch
    with torch.no_grad(), _rule_dispatch():
        rows, lay = c["hip"].forward_hip(dev(c["x"]), c["mlp"].cuda(), ops, stereo=stereo)
    torch.cuda.synchronize()
    rows = rows.float().cpu().view(2, H, W, -1).permute(0, 3, 1, 2)
    o = lay["depth_offset"]
    assert bool((rows[:, o + D:o + lay["depth_padded"]] == 0).all())
    return torch.cat([rows[:, o:o + D], rows[:, :CTX]], 1)        # the plain path's [depth logits | context]


@pytest.mark.parametrize("prev", [True, False], ids=["frame", "first-frame"])
def test_forward_hip_against_the_fp32_plain_path(nets, prev):
    from bevformer_tensorrt_amd import functions
    with torch.no_grad():
        want = nets["ref"](nets["x"].float(), nets["mlp"], _metas(nets, prev))
    got = _fast(nets, functions, prev)
    err, bar = (got - want).abs().max().item(), 3e-2 * max(1.0, want.abs().max().item())
    print(f"DepthNet(stereo).forward_hip vs fp32 plain ({'frame' if prev else 'first frame'}): {err:.4e} (bar {bar:.4e}, "
          f"max |want| {want.abs().max().item():.3f})")
    assert err <= bar
    if prev:        # the cost volume is live: the first frame's logits differ
        with torch.no_grad():
            other = nets["ref"](nets["x"].float(), nets["mlp"], _metas(nets, False))
        assert (other[:, :D] - want[:, :D]).abs().max().item() > 1e-2


def test_every_stereo_launch_against_its_own_statement(nets):
    """The launches the stereo branch adds to or changes in a forward, each replayed from its recorded operands: the
    gated copies against x * gate (equal bits) with the slice's neighbouring columns untouched, the cost volume against
    the float64 statement, the four convolutions on mid + Dpad / Dpad columns against F.conv2d in fp32 on the same fp16
    operands; the pad columns exact zeros all the way.  The launches behind the first block (the other blocks, ASPP, the
    last 1 x 1, the split) are the non-stereo net's, call for call: tests/test_bevdepth_gpu.py and
    tests/test_lss_depthnet_gpu.py replay those, and test_non_stereo_models_keep_their_bits below pins that this change
    left them alone."""
    ops = _Recorder(("stereo_cost_volume", "conv_slice_nhwc", "se_gate2_nhwc"))
    _fast(nets, ops)
    hip = nets["hip"]
    dp = hip.stereo_padded()
    assert dp == 32
    names = [c[0] for c in ops.calls]
    assert names[:4] == ["se_gate2_nhwc", "stereo_cost_volume", "conv_slice_nhwc", "conv_slice_nhwc"]
    (_, a, k, out) = ops.calls[1]
    assert out.shape == (2, dp, 4 * H, 4 * W) and k["dpad"] == dp
    grid = __import__("bevformer_tensorrt_amd").functions.stereo_grid(a[2], k["frustum_tables"]).cpu()
    ref = U.ref_cost_volume(a[0].float().cpu(), a[1].float().cpu(), grid, hip.bias)
    err = (out[:, :D].double().cpu() - ref["prob"]).abs()
    assert bool((err <= U.general_bound(ref["prob"], ref["mag"])).all()) and not bool(out[:, D:].any())
    assert 0.05 < ref["gate"].float().mean().item() < 0.95
    (_, ga, gk, gouts) = ops.calls[0]
    gate_out = gouts[0]
    both = gate_out._base if gate_out._base is not None else gate_out
    # the gated depth copy: one fp32 product and one rounding per value, written into columns 0 .. mid of the buffer
    r, gates = ga[0], ga[1]
    assert gk["out_a"].data_ptr() == gate_out.data_ptr() and gate_out.shape == (2, MID, H, W)
    want_gate = (r.float() * gates[0][:, :, None, None]).half()
    assert torch.equal(gate_out.contiguous().view(torch.int16), want_gate.contiguous().view(torch.int16))
    assert torch.equal(gouts[1].contiguous().view(torch.int16),
                       (r.float() * gates[1][:, :, None, None]).half().contiguous().view(torch.int16))
    # ... and nothing beside them: the same call into a buffer of sentinels leaves the cost volume's share alone
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    sentinel = nhwc_empty(2, MID + dp, H, W, r.device)
    sentinel.fill_(7.0)
    ops._f.se_gate2_nhwc(r, gates, out_a=sentinel[:, :MID])
    torch.cuda.synchronize()
    assert bool((sentinel[:, MID:] == 7.0).all()) and torch.equal(sentinel[:, :MID], gate_out)
    convs = [c for c in ops.calls if c[0] == "conv_slice_nhwc"]
    blk = hip.depth_conv[0]
    want_w = [hip.cost_volumn_net[0].weight, hip.cost_volumn_net[1].weight, hip.context_conv.weight, blk.conv1.weight,
              blk.downsample.weight]
    seen = 0
    for (_, a, k, out) in convs:
        x, w, b, act = a[0], a[1], a[2], a[3]
        hit = [i for i, t in enumerate(want_w) if t is w]
        if not hit or hit[0] == 2:
            continue
        seen += 1
        cin, cout = w.shape[1], w.shape[0]
        assert x.shape[1] % 32 == 0 and not bool(x[:, cin:].any())                 # the pad channels arrive as exact zeros
        y = F.conv2d(x[:, :cin].float(), w.float(), None if b is None else b.float()[:cout], stride=k.get("stride", 1),
                     padding=w.shape[2] // 2)
        if act == "relu":
            y = F.relu(y)
        tol = 2.0 ** -10 * max(1.0, y.abs().max().item()) + 1e-3
        assert (out[:, :cout].float() - y).abs().max().item() <= tol, (hit[0], tol)
        assert not bool(out[:, cout:].any())
    assert seen == 4
    # the second stride-2 convolution wrote the cost volume's share of the block's input; the gate wrote the rest
    assert convs[1][3].data_ptr() == gate_out.data_ptr() + 2 * MID and convs[1][3].shape[1] == dp
    assert both.numel() == 2 * H * W * (MID + dp)


@pytest.fixture(scope="module")
def model():
    from bevformer_tensorrt_amd.bevdet import BEVSTEREO_R50, BEVDet, jittered_rig
    cfg = dict(BEVSTEREO_R50, input_size=(64, 96))
    m = BEVDet(cfg, seed=0, bev_half="hip")
    rig = jittered_rig(m.view, 2, n_cams=2)
    rig[4][0, :, 0] *= 96 / 704.0
    with torch.no_grad():
        v = m.view.get_mlp_input(*rig).reshape(-1, 27)
        bn = m.view.depth_net.bn
        bn.running_mean.copy_(v.mean(0))
        bn.running_var.copy_((0.02 * v.abs().mean(0) + 0.05) ** 2)
    m = m.cuda().half()
    calib = m.view.calibration_matrices(*rig).cuda()
    img = torch.randn(1, 2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda().half()
    k2s = torch.eye(4).repeat(1, 2, 1, 1)
    k2s[0, :, :3, 3] = torch.tensor([[0.3, 0.02, 0.1], [-0.2, 0.0, 0.6]])
    with torch.no_grad():
        _, feat = m.image_features(img.flatten(0, 1), stereo=True)
    prev = feat.roll(1, 3).contiguous(memory_format=torch.channels_last)
    metas = m.view.stereo_metas(prev, None, k2s, rig[2], rig[3], rig[4], prepare=True)
    return dict(m=m, cfg=cfg, rig=rig, calib=calib, img=img, metas=metas, k2s=k2s)


def test_model_eager_equals_graph_and_follows_the_previous_frame(model):
    m, img, calib, metas = model["m"], model["img"], model["calib"], model["metas"]
    assert m.view.D == 59 and m.view.depth_net.stereo_padded() == 64
    eager = [o.clone() for o in m.forward_calibrated(img, calib, metas)]
    again = m.forward_calibrated(img, calib, metas)
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in eager)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    first = m.forward_calibrated(img, calib, dict(metas, cv_feat_list=[None, None]))
    moved = m.forward_calibrated(img, calib, dict(metas, cv_feat_list=[metas["cv_feat_list"][0].roll(2, 2).contiguous(memory_format=torch.channels_last), None]))
    assert not torch.equal(first[5], eager[5]) and not torch.equal(moved[5], eager[5])
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        m.forward_calibrated(img, calib, metas)
    torch.cuda.current_stream().wait_stream(stream)
    with torch.cuda.graph(graph):
        outs = m.forward_calibrated(img, calib, metas)
    for _ in range(2):
        for o in outs:
            o.fill_(3.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, outs):
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
    # the fp16 plain path of the same weights: close (the bar of the frame tests)
    from bevformer_tensorrt_amd.bevdet import BEVDet
    plain = BEVDet(model["cfg"], seed=0, bev_half="torch").cuda().half()
    plain.load_state_dict(m.state_dict())
    want = plain.forward_calibrated(img, calib, {k: v for k, v in metas.items() if k not in ("consts", "tables")})
    for a, b in zip(eager, want):
        bar = 3e-2 * max(1.0, b.float().abs().max().item())
        assert (a.float() - b.float()).abs().max().item() <= bar


class _Probe(torch.overrides.TorchFunctionMode):
    def __init__(self):
        super().__init__()
        self.counts = dict(cat=0, grid_sample=0, softmax=0)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func in (torch.cat, torch.concat, torch.concatenate):
            self.counts["cat"] += 1
        elif func in (F.grid_sample, torch.grid_sampler):
            self.counts["grid_sample"] += 1
        elif func in (F.softmax, torch.softmax, torch.Tensor.softmax):
            self.counts["softmax"] += 1
        return func(*args, **(kwargs or {}))


def test_no_cat_grid_sample_or_softmax_on_the_fast_path(model):
    m, calib, metas = model["m"], model["calib"], model["metas"]
    with torch.no_grad():
        x, feat = m.image_features(model["img"].flatten(0, 1), stereo=True)
    full = dict(metas, cv_feat_list=[metas["cv_feat_list"][0], feat])
    m.bev_half_calibrated(x, calib, stereo_metas=full)
    with _Probe() as probe:
        m.bev_half_calibrated(x, calib, stereo_metas=full)
    torch.cuda.synchronize()
    print("hip  :", probe.counts)
    assert probe.counts == dict(cat=0, grid_sample=0, softmax=0)
    from bevformer_tensorrt_amd.bevdet import BEVDet
    plain = BEVDet(model["cfg"], seed=0, bev_half="torch").cuda().half()
    with _Probe() as probe:
        plain.bev_half_calibrated(x, calib, stereo_metas=full)
    print("torch:", probe.counts)
    assert all(v >= 1 for v in probe.counts.values())


def test_capture_guards_and_weight_reload(model):
    from bevformer_tensorrt_amd.bevdet import BEVDet
    m = BEVDet(model["cfg"], seed=0, bev_half="hip").cuda().half()
    m.load_state_dict(model["m"].state_dict())
    img, calib, metas = model["img"], model["calib"], model["metas"]
    bare = {k: v for k, v in metas.items() if k not in ("consts", "tables")}
    assert m.view.depth_net_merged(build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            m.forward_calibrated(img, calib, metas)
    del graph
    assert m.view.depth_net_merged(build=False) is None
    first = [o.clone() for o in m.forward_calibrated(img, calib, metas)]
    for a, b in zip(first, m.forward_calibrated(img, calib, bare)):        # derived constants: the same bits
        assert torch.equal(a, b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare=True"):           # metas without the uploaded constants
            m.forward_calibrated(img, calib, bare)
    del graph
    # a reload of the cost-volume net alone: the packed operands are stale, rebuilt, and the frame follows
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["view.depth_net.cost_volumn_net.1.weight"].mul_(-3.0)
    m.load_state_dict(sd)
    assert m.view.depth_net_merged(build=False) is None
    new = m.forward_calibrated(img, calib, metas)
    torch.cuda.synchronize()
    assert m.view.depth_net_merged(build=False) is not None and not torch.equal(new[5], first[5])


def test_int8_build_refuses_the_stereo_model(model):
    from bevformer_tensorrt_amd import quantization as Q
    with pytest.raises(NotImplementedError, match="stereo"):
        Q.build_int8_bevdet(model["m"], torch.device("cuda"), [])


def _parent_forward_hip(net, x, mlp_input, ops):
    """DepthNet.forward_hip as the parent commit had it (no stereo branch, no `downsample` case), restated call for call."""
    from bevformer_tensorrt_amd.bevdepth import ASPP_DILATIONS
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    P = net.fast_operands()
    lay, mid = P["layout"], net.mid_channels
    n, _, h, w = x.shape
    gates = ops.lss_camera_gate(mlp_input, P["gate"], mid)
    r = ops.conv_nhwc(x, net.reduce_conv.weight, net.reduce_conv.bias, True)
    depth, context = ops.se_gate2_nhwc(r, gates)
    rows = nhwc_empty(n, lay["row_stride"], h, w, x.device)
    o = lay["depth_offset"]
    ops.conv_slice_nhwc(context, net.context_conv.weight, net.context_conv.bias, "none", out=rows[:, :o])
    for m in net.depth_conv[:3]:
        t = ops.conv_nhwc(depth, m.conv1.weight, m.conv1.bias, True)
        depth = ops.conv_nhwc(t, m.conv2.weight, m.conv2.bias, True, depth)
    if net.use_aspp:
        a = net.aspp
        amid = a.aspp1.out_channels
        cat = nhwc_empty(n, 4 * amid, h, w, x.device)
        for i, (m, d) in enumerate(zip(a.branches(), ASPP_DILATIONS)):
            ops.conv_slice_nhwc(depth, m.weight, m.bias, "relu", out=cat[:, i * amid:(i + 1) * amid], dilation=d)
        pooled = ops.global_avgpool_nhwc(depth)
        g = ops.dense_auto(pooled, P["pool_w"], a.global_avg_pool.bias, None, True)
        image_bias = ops.dense_auto(g, P["conv1_pool"], a.conv1.bias, None, False)
        depth = ops.conv_slice_nhwc(cat, P["conv1_main"], None, "relu", image_bias=image_bias)
    if net.use_dcn:
        depth = net.dcn.forward_hip(depth, ops)
    ops.conv_slice_nhwc(depth, P["wd"], P["bd"], "none", out=rows[:, o:o + lay["depth_padded"]])
    return rows.permute(0, 2, 3, 1).reshape(n * h * w, lay["row_stride"])


def test_non_stereo_models_keep_their_bits():
    """The three non-stereo configurations share DepthNet.forward / forward_hip, _depth_feat and BEVDet's entry points
    with the stereo model.  BEVDet() and BEVDet(BEVDEPTH_R50): the parent commits' frame digests that
    tests/test_bevdepth_gpu.py (PARENT_DIGEST) and tests/test_bevdepth_dcn_gpu.py (PARENT_DIGEST_BEVDEPTH) record, asserted
    here again beside the stereo model.  BEVDEPTH_R50_DCN has no recorded digest: its DepthNet at R50 widths (mid 256,
    D 59, six 16 x 44 maps) through forward_hip equals, bit for bit, the parent commit's launch sequence restated above
    on the same operands; so does the net without the layer."""
    from bevformer_tensorrt_amd import functions
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.bevdet import _rule_dispatch
    from test_bevdepth_dcn_gpu import PARENT_DIGEST_BEVDEPTH, bevdepth_frame
    from test_bevdepth_gpu import PARENT_DIGEST, default_frame, frame_digest
    model, outs = default_frame()
    assert not model.stereo and model.backbone.out_indices == (2, 3) and frame_digest(outs) == PARENT_DIGEST
    model, outs = bevdepth_frame()
    assert not model.stereo and not model.view.depth_net.stereo and frame_digest(outs) == PARENT_DIGEST_BEVDEPTH
    del model, outs
    g = torch.Generator().manual_seed(8)
    x = torch.randn(6, 256, 16, 44, generator=g).half().cuda().contiguous(memory_format=torch.channels_last)
    mlp = (0.5 * torch.randn(6, 27, generator=g)).cuda()
    for use_dcn in (True, False):
        net = DepthNet(256, 256, 64, 59, use_dcn=use_dcn).eval()
        _randomise(net, g)
        if use_dcn:
            with torch.no_grad():           # live offsets (the zero initialisation samples at the integer taps)
                net.dcn.conv_offset.bias.copy_(torch.randn(18, generator=g))
        net = net.cuda().half()
        with torch.no_grad(), _rule_dispatch():
            want = _parent_forward_hip(net, x, mlp, functions).clone()
            got, lay = net.forward_hip(x, mlp, functions)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got.float()).all()) and got.float().std().item() > 1e-2
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), use_dcn
        with pytest.raises(ValueError, match="stereo"):
            net.forward_hip(x, mlp, functions, stereo=(None, x, mlp, ()))
