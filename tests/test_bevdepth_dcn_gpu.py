"""BEVDet(BEVDEPTH_R50_DCN): the DepthNet with the reference's DCN layer (mmcv's DCNv1 pack, groups = 4) behind the ASPP,
fast path (conv_offset_nhwc + deform_conv2d_nhwc) against the fp32 plain path on the same weights.  The fixture sets
`conv_offset` so that the offsets have a standard deviation of about one pixel: with mmcv's zero initialisation the
layer is a plain grouped convolution and nothing here would show.  Helpers and sizes of tests/test_bevdepth_gpu.py."""
import pytest
import torch

from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDEPTH_R50_DCN
from test_bevdepth_gpu import NAMES, _OraclePoolOps, _batched, _probe, _settle_bn, frame_digest

pytestmark = pytest.mark.gpu


class _CountingOps:
    """The package's operator set, counting the calls by name: every function the fast path calls behind the image neck
    is one C entry."""

    def __init__(self):
        import bevformer_tensorrt_amd.functions as fn
        self._fn, self.calls, self.active = fn, {}, False

    def __getattr__(self, name):
        f = getattr(self._fn, name)
        if not callable(f):
            return f

        def counted(*a, **k):
            if self.active:
                self.calls[name] = self.calls.get(name, 0) + 1
            return f(*a, **k)
        return counted


def _build(cfg, bev_half, dtype, ops=None, state=None):
    from bevformer_tensorrt_amd.bevdet import BEVDet, synthetic_rig
    m = BEVDet(cfg, ops=ops, seed=0, bev_half=bev_half)
    _settle_bn(m, synthetic_rig(m.view))
    m = m.cuda().to(dtype)
    if state is not None:
        m.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in state.items()})
    return m


@pytest.fixture(scope="module")
def frame():
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    hip = _build(BEVDEPTH_R50_DCN, "hip", torch.float16)
    dcn = hip.view.depth_net.dcn
    g = torch.Generator().manual_seed(21)
    with torch.no_grad():
        dcn.conv_offset.weight.copy_((torch.randn(18, 256, 3, 3, generator=g) * 0.02).to(dcn.conv_offset.weight))
        dcn.conv_offset.bias.copy_((torch.randn(18, generator=g) * 0.3).to(dcn.conv_offset.bias))
    ref = _build(BEVDEPTH_R50_DCN, "torch", torch.float32, ops=_OraclePoolOps, state=hip.state_dict())
    rigs = [jittered_rig(hip.view, k) for k in (1, 2, 3)]
    rig = rigs[0]
    ranks = [r.cuda() for r in hip.view.get_bev_pool_input(*rig)]
    mlp = hip.view.get_mlp_input(*rig).cuda()
    calib = hip.view.calibration_matrices(*rig).cuda()
    imgs = torch.randn(2, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda()
    # the DepthNet's input as the fast path sees it (fp16 image features), and the offset convolution scaled to a standard
    # deviation of one pixel on this frame (measured on the fp32 plain DepthNet)
    x16 = hip.image_features(imgs[0].half())
    x32 = x16.float().contiguous()
    seen = []
    hook = ref.view.depth_net.dcn.conv_offset.register_forward_hook(lambda m, a, out: seen.append(out.detach()))
    ref.view.depth_net(x32, mlp.reshape(6, 27))
    scale = 1.0 / float(seen[0].std())
    with torch.no_grad():
        for m in (dcn, ref.view.depth_net.dcn):
            m.conv_offset.weight.mul_(scale)
            m.conv_offset.bias.mul_(scale)
    rows32 = ref.view.depth_net(x32, mlp.reshape(6, 27))
    hook.remove()
    tor = _build(BEVDEPTH_R50_DCN, "torch", torch.float16, state=hip.state_dict())
    want = ref(imgs[:1], *ranks, mlp_input=mlp)
    del ref
    return dict(hip=hip, torch=tor, rigs=rigs, ranks=ranks, mlp=mlp, calib=calib, imgs=imgs.half(), img=imgs[:1].half(),
                want=want, rows32=rows32, x16=x16, offset_std=float(seen[1].float().std()))


def test_the_layer_is_there_and_its_offsets_are_live(frame):
    from bevformer_tensorrt_amd.bevdepth import DeformConv2dPack
    dn = frame["hip"].view.depth_net
    assert dn.use_dcn and isinstance(dn.depth_conv[4], DeformConv2dPack) and len(dn.depth_conv) == 6
    assert tuple(dn.depth_conv[4].weight.shape) == (256, 64, 3, 3)
    print(f"offset standard deviation on the frame: {frame['offset_std']:.3f} pixels")
    assert 0.9 <= frame["offset_std"] <= 1.1


def test_depthnet_rows_and_head_maps(frame):
    """DepthNet rows: rms(forward_hip - fp32 plain) <= 1.25 rms(plain fp16 - fp32 plain) (design/bevdepth.md section 4:
    the fallback gate).  The six head maps: max |hip - fp32| <= 3e-2 max(1, max |fp32|)."""
    from bevformer_tensorrt_amd.bevdet import HEADS_R50, _rule_dispatch
    hip, tor, img = frame["hip"], frame["torch"], frame["img"]
    dn = hip.view.depth_net
    x = frame["x16"]
    mlp = frame["mlp"].reshape(6, 27)
    hip.prepare_bev_half()
    with _rule_dispatch():
        rows, lay = dn.forward_hip(x, mlp.float(), hip.ops)
    n, _, H, W = x.shape
    D, C, o = dn.depth_channels, dn.context_channels, lay["depth_offset"]
    rows = rows.view(n, H, W, -1).float()
    fast = torch.cat([rows[..., o:o + D], rows[..., :C]], dim=-1).permute(0, 3, 1, 2)
    plain = tor.view.depth_net(x, mlp.half()).float()
    ref = frame["rows32"]
    assert fast.shape == plain.shape == ref.shape == (6, D + C, 16, 44)
    rms = lambda t: float(t.detach().double().pow(2).mean().sqrt())
    for name, sl in (("depth logits", slice(0, D)), ("context", slice(D, D + C)), ("all rows", slice(0, D + C))):
        e_fast, e_plain = rms(fast[:, sl] - ref[:, sl]), rms(plain[:, sl] - ref[:, sl])
        print(f"DepthNet {name}: rms error fast {e_fast:.4e}, plain fp16 {e_plain:.4e}, rms |fp32| {rms(ref[:, sl]):.4e}")
        assert e_plain > 0 and e_fast <= 1.25 * e_plain, name
    got = [t.clone() for t in hip(img, *frame["ranks"], mlp_input=frame["mlp"])]
    again = hip(img, *frame["ranks"], mlp_input=frame["mlp"])
    torch.cuda.synchronize()
    for (name, c), a, a2, b in zip(HEADS_R50, got, again, frame["want"]):
        assert a.shape == b.shape == (1, c, 128, 128) and a.dtype == torch.float16, name
        err, bar = (a.float() - b).abs().max().item(), 3e-2 * max(1.0, b.abs().max().item())
        print(f"{name}: hip vs fp32 plain {err:.4e} (bar {bar:.4e})")
        assert err <= bar, (name, err, bar)
        assert torch.equal(a.contiguous().view(torch.int16), a2.contiguous().view(torch.int16)), name   # two frames
    # the layer matters: with its offsets zeroed the depth logits move
    sd = {k: v.clone() for k, v in hip.state_dict().items()}
    with torch.no_grad():
        dn.dcn.conv_offset.weight.zero_()
        dn.dcn.conv_offset.bias.zero_()
    with _rule_dispatch():
        rows0, _ = dn.forward_hip(x, mlp.float(), hip.ops)
    hip.load_state_dict(sd)
    assert rms(rows0.view(n, H, W, -1)[..., o:o + D].float() - rows[..., o:o + D]) > 10 * rms(fast[:, :D] - ref[:, :D])


def test_two_more_launches_and_no_framework_glue(frame):
    img, calib = frame["img"], frame["calib"]
    calls = {}
    for key, cfg in (("dcn", BEVDEPTH_R50_DCN), ("plain", BEVDEPTH_R50)):
        ops = _CountingOps()
        m = _build(cfg, "hip", torch.float16, ops=ops)
        m.forward_calibrated(img, calib)
        x = m.image_features(img.flatten(0, 1))
        ops.active = True
        m.view._depth_feat(x, m.view.split_calibration(calib)[1])
        ops.active = False
        calls[key] = dict(ops.calls)
        if key == "dcn":
            counts = _probe(m, img, calib)
            print("framework calls behind the image neck:", counts)
            assert counts == dict(conv2d=0, interpolate=0, cat=0, adaptive_avg_pool2d=0, contiguous=0)
    print("operator calls of the DepthNet + split:", calls)
    extra = {k: calls["dcn"].get(k, 0) - calls["plain"].get(k, 0) for k in set(calls["dcn"]) | set(calls["plain"])}
    assert {k: v for k, v in extra.items() if v} == dict(conv_offset_nhwc=1, deform_conv2d_nhwc=1)


def test_runner_batch_one_and_two_replay_bit_equal_and_samples_are_independent(frame):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img, imgs, rigs = frame["hip"], frame["img"], frame["imgs"], frame["rigs"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True)
    eager = BEVDetRunner(model, torch.device("cuda"), graph=False)
    seen = []
    for rig in rigs[:2]:
        out, want = runner.step(img, *rig), eager.step(img, *rig)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, out, want):
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), n
        seen.append(out[5].clone())
    assert runner._graph is not None and not torch.equal(seen[0], seen[1])
    runner2 = BEVDetRunner(model, torch.device("cuda"), graph=True, batch=2)
    pair = _batched(rigs[:2])
    out = [o.clone() for o in runner2.step(imgs, *pair)]
    calib2 = model.view.calibration_matrices_batched(*pair).cuda()
    plain = model.forward_calibrated(imgs, calib2)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, out, plain):
        assert a.shape[0] == 2 and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), n
    graph = runner2._graph
    # sample 1's image and calibration replaced: sample 0 keeps its bits, no new capture
    other = torch.stack([imgs[0], imgs[0].flip(-1)])
    out_b = [o.clone() for o in runner2.step(other, *_batched([rigs[0], rigs[2]]))]
    torch.cuda.synchronize()
    assert runner2._graph is graph
    for n, a, b in zip(NAMES, out, out_b):
        assert torch.equal(a[0].contiguous().view(torch.int16), b[0].contiguous().view(torch.int16)), n
    assert not torch.equal(out[5][1], out_b[5][1])


def test_step_raw_replays_bit_equal_to_the_eager_run(frame):
    """BEVDetRunner.step_raw (raw camera frames, the device front end) reaches the same DepthNet."""
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, rig = frame["hip"], frame["rigs"][0]
    raw = torch.randint(0, 256, (6, 900, 1600, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).cuda()
    args = (rig[0], rig[1], rig[2], rig[5])
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True, raw_size=(900, 1600))
    eager = BEVDetRunner(model, torch.device("cuda"), graph=False, raw_size=(900, 1600))
    a = [o.clone() for o in runner.step_raw(raw, *args)]
    b = [o.clone() for o in eager.step_raw(raw, *args)]
    torch.cuda.synchronize()
    assert runner._graph_raw is not None
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16)), n
        assert bool(torch.isfinite(x.float()).all()), n


def test_capture_guard_and_weight_reload(frame):
    from bevformer_tensorrt_amd.bevdet import synthetic_rig
    from bevformer_tensorrt_amd.functions import deform_conv_packed_weight
    model = _build(BEVDEPTH_R50_DCN, "hip", torch.float16, state=frame["hip"].state_dict())
    calib = model.view.calibration_matrices(*synthetic_rig(model.view)).cuda()
    img, dcn = frame["img"], model.view.depth_net.dcn
    assert model.view.depth_net_merged(build=False) is None and deform_conv_packed_weight(dcn.weight, build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.forward_calibrated(img, calib)
    del graph
    assert model.view.depth_net_merged(build=False) is None and deform_conv_packed_weight(dcn.weight, build=False) is None
    first = [o.clone() for o in model.forward_calibrated(img, calib)]
    assert model.view.depth_net_merged(build=False) is not None
    packed = deform_conv_packed_weight(dcn.weight, build=False)
    assert packed is not None
    # a reload that changes the DCN weight alone: the operands are stale, rebuilt, and the frame moves
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["view.depth_net.depth_conv.4.weight"].mul_(-1.0)
    model.load_state_dict(sd)
    assert model.view.depth_net_merged(build=False) is None
    new = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    assert model.view.depth_net_merged(build=False) is not None
    assert not torch.equal(new[5], first[5])
    # ... and the offset convolution's bias alone
    with torch.no_grad():
        dcn.conv_offset.bias.add_(0.5)
    assert model.view.depth_net_merged(build=False) is None
    moved = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    assert not torch.equal(moved[5], new[5])


def test_int8_build_refuses_before_any_frame(frame):
    from bevformer_tensorrt_amd import quantization as Q

    def frames():
        raise AssertionError("a frame ran")
        yield

    for half in ("int8", "fp16"):
        with pytest.raises(NotImplementedError, match="DCN"):
            Q.build_int8_bevdet(frame["hip"], torch.device("cuda"), frames(), bev_half=half)


# sha-256 of the six maps of one BEVDet(BEVDEPTH_R50) frame (below), taken from a build of the PARENT commit on the same
# MI355X in the session that added the DCN layer: the model without the layer keeps its modules, its launches and its bits
PARENT_DIGEST_BEVDEPTH = "b3e34581ba971503cd1f48ba405fafd5a296599840001384802d308ed779139f"


def bevdepth_frame():
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    model = BEVDet(BEVDEPTH_R50, seed=0, bev_half="hip").cuda().half()
    calib = model.view.calibration_matrices(*jittered_rig(model.view, 5)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(3)).cuda().half()
    model.forward_calibrated(img, calib)
    outs = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    return model, outs


def test_models_without_the_layer_keep_the_parent_commits_bits():
    import sys
    from test_bevdepth_gpu import PARENT_DIGEST, default_frame
    assert "bevformer_tensorrt_amd.functions.deform_conv" in sys.modules          # the new operator module is loaded
    model, outs = bevdepth_frame()
    assert not model.view.depth_net.use_dcn and len(model.view.depth_net.depth_conv) == 5
    assert not any("conv_offset" in k for k in model.state_dict())
    assert frame_digest(outs) == PARENT_DIGEST_BEVDEPTH
    _, outs = default_frame()
    assert frame_digest(outs) == PARENT_DIGEST
