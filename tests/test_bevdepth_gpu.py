"""BEVDet(BEVDEPTH_R50): the camera-aware DepthNet with ASPP (bevformer_tensorrt_amd/bevdepth.py) in front of the LSS
pooling, fast path (bev_half="hip", this package's kernels) against the fp32 plain path on the same synthetic weights
at the bar of tests/test_bevdet_bev_half_gpu.py, the absence of framework glue behind the image neck, run-to-run bits,
BEVDetRunner at batch 1 and 2 with a calibration that changes between frames, the capture guard and a weight reload.
256 x 704, six cameras: the sizes of that file."""
import hashlib

import pytest
import torch
import torch.nn.functional as F

from util_bevpool import index_add_reference

pytestmark = pytest.mark.gpu

NAMES = ("reg", "height", "dim", "rot", "vel", "heatmap")


class _OraclePoolOps:
    """The reference data path: library convolutions and the oracle statement of bev_pool_v2 (fp64 index_add)."""

    @staticmethod
    def bev_pool_v2_2(depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, bev_h, bev_w):
        want = index_add_reference(depth.float().cpu().numpy(), feat.float().cpu().numpy(), ranks_depth.cpu().numpy(),
                                   ranks_feat.cpu().numpy(), ranks_bev.cpu().numpy(), bev_h, bev_w)
        return torch.from_numpy(want).to(depth.device, depth.dtype)


def _settle_bn(model, rig):
    """Running statistics of the DepthNet's BatchNorm1d that fit the calibration values (focal lengths above 1000 next
    to rotation entries below 1), so that the gates spread instead of saturating; weights and shift randomised."""
    v = model.view.get_mlp_input(*rig).reshape(-1, 27)
    g = torch.Generator().manual_seed(7)
    bn = model.view.depth_net.bn
    with torch.no_grad():
        bn.running_mean.copy_(v.mean(0) + 0.05 * v.abs().mean(0) * torch.randn(27, generator=g))
        bn.running_var.copy_((0.02 * v.abs().mean(0) + 0.05) ** 2)
        bn.weight.copy_(1.0 + 0.2 * torch.randn(27, generator=g))
        bn.bias.copy_(0.2 * torch.randn(27, generator=g))


def _build(bev_half, dtype, ops=None, state=None):
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDet, synthetic_rig
    m = BEVDet(BEVDEPTH_R50, ops=ops, seed=0, bev_half=bev_half)
    _settle_bn(m, synthetic_rig(m.view))
    m = m.cuda().to(dtype)
    if state is not None:
        m.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in state.items()})
    return m


@pytest.fixture(scope="module")
def frame():
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    hip = _build("hip", torch.float16)
    tor = _build("torch", torch.float16, state=hip.state_dict())
    ref = _build("torch", torch.float32, ops=_OraclePoolOps, state=hip.state_dict())
    rigs = [jittered_rig(hip.view, k) for k in (1, 2, 3)]
    rig = rigs[0]
    ranks = [r.cuda() for r in hip.view.get_bev_pool_input(*rig)]
    mlp = hip.view.get_mlp_input(*rig).cuda()
    calib = hip.view.calibration_matrices(*rig).cuda()
    imgs = torch.randn(2, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda()
    want = ref(imgs[:1], *ranks, mlp_input=mlp)
    del ref
    return dict(hip=hip, torch=tor, rigs=rigs, ranks=ranks, mlp=mlp, calib=calib, imgs=imgs.half(), img=imgs[:1].half(),
                want=want)


def test_the_view_transformer_is_the_bevdepth_one_and_the_row_has_two_parts(frame):
    from bevformer_tensorrt_amd.bevdepth import DepthNet, LSSViewTransformerBEVDepth
    view = frame["hip"].view
    assert type(view) is LSSViewTransformerBEVDepth and type(view.depth_net) is DepthNet
    assert frame["calib"].shape == (6 * 51 + 9,)
    geo, mlp = view.split_calibration(frame["calib"])
    assert geo.shape == (6 * 24 + 9,) and mlp.shape == (6, 27) and torch.equal(mlp, frame["mlp"].reshape(6, 27))
    assert geo.data_ptr() == frame["calib"].data_ptr()                       # views: no copy at batch 1


def test_fast_path_against_the_fp32_plain_path(frame):
    """The bar and statement of tests/test_bevdet_bev_half_gpu.py's "hip" frame: max |hip - fp32| <= 3e-2 max(1, max|fp32|)
    per output map."""
    from bevformer_tensorrt_amd.bevdet import HEADS_R50
    hip, img = frame["hip"], frame["img"]
    got = [o.clone() for o in hip(img, *frame["ranks"], mlp_input=frame["mlp"])]
    again = hip(img, *frame["ranks"], mlp_input=frame["mlp"])
    plain = frame["torch"](img, *frame["ranks"], mlp_input=frame["mlp"])
    cal = hip.forward_calibrated(img, frame["calib"])
    torch.cuda.synchronize()
    for (n, c), a, a2, b, p, k in zip(HEADS_R50, got, again, frame["want"], plain, cal):
        assert a.shape == b.shape == p.shape == (1, c, 128, 128) and a.dtype == torch.float16, n
        err, bar = (a.float() - b).abs().max().item(), 3e-2 * max(1.0, b.abs().max().item())
        print(f"{n}: hip vs fp32 plain {err:.4e} (bar {bar:.4e}); plain fp16 vs fp32 plain "
              f"{(p.float() - b).abs().max().item():.4e}; hip vs plain fp16 {(a.float() - p.float()).abs().max().item():.4e}")
        assert err <= bar, (n, err, bar)
        assert torch.equal(a.contiguous().view(torch.int16), a2.contiguous().view(torch.int16)), n     # two frames: equal bits
        # the device index build orders points inside a cell differently from the host ranks: close, not equal
        assert (k.float() - a.float()).abs().max().item() <= bar, n
    # the DepthNet alone: the gate moves the features (a network that ignored it would pass the frame test too)
    x = hip.image_features(img.flatten(0, 1))
    d1, f1, fast = hip.view._depth_feat(x, frame["mlp"].reshape(6, 27))
    other = frame["mlp"].reshape(6, 27).clone()
    other[:, 0] += 40.0
    d2, f2, _ = hip.view._depth_feat(x, other)
    assert fast and not torch.equal(f1, f2) and not torch.equal(d1, d2)
    assert torch.allclose(d1.float().sum(1), torch.ones_like(d1[:, 0]).float(), atol=2e-2)


class _Probe(torch.overrides.TorchFunctionMode):
    CONV = (torch.conv2d, F.conv2d, torch.convolution, torch._convolution)
    POOL = (F.adaptive_avg_pool2d, torch._C._nn.adaptive_avg_pool2d)

    def __init__(self):
        super().__init__()
        self.active = False
        self.counts = dict(conv2d=0, interpolate=0, cat=0, adaptive_avg_pool2d=0, contiguous=0)

    def __torch_function__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if self.active:
            if func in self.CONV:
                self.counts["conv2d"] += 1
            elif func is F.interpolate:
                self.counts["interpolate"] += 1
            elif func in (torch.cat, torch.concat, torch.concatenate):
                self.counts["cat"] += 1
            elif func in self.POOL:
                self.counts["adaptive_avg_pool2d"] += 1
            elif func is torch.Tensor.contiguous and \
                    out.untyped_storage().data_ptr() != args[0].untyped_storage().data_ptr():
                self.counts["contiguous"] += 1
        return out


def _probe(model, img, calib):
    probe, inner = _Probe(), model.image_features

    def image_features(image):
        out = inner(image)
        probe.active = True
        return out

    model.image_features = image_features
    try:
        with probe:
            model.forward_calibrated(img, calib)
    finally:
        probe.active = False
        del model.image_features
    torch.cuda.synchronize()
    return probe.counts


def test_no_framework_glue_behind_image_features(frame):
    for m in (frame["hip"], frame["torch"]):
        m.forward_calibrated(frame["img"], frame["calib"])
    counts = _probe(frame["hip"], frame["img"], frame["calib"])
    print("hip  :", counts)
    assert counts == dict(conv2d=0, interpolate=0, cat=0, adaptive_avg_pool2d=0, contiguous=0)
    counts = _probe(frame["torch"], frame["img"], frame["calib"])
    print("torch:", counts)
    assert all(counts[k] >= 1 for k in ("conv2d", "interpolate", "cat", "adaptive_avg_pool2d")), counts


def test_runner_batch_one_follows_the_calibration_without_a_new_capture(frame):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img = frame["hip"], frame["img"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True)
    eager = BEVDetRunner(model, torch.device("cuda"), graph=False)
    rigs = list(frame["rigs"])
    seen = []
    for rig in rigs:
        out = runner.step(img, *rig)
        want = eager.step(img, *rig)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, out, want):
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), n
        seen.append(out[5].clone())
    graph = runner._graph
    assert graph is not None
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    # a changed intrinsic that moves ONLY the gate: every calibration value enters the geometry too, so the change is
    # made in the row's MLP part -- the index arrays stay, the gate moves, the graph is the same
    calib_a = model.view.calibration_matrices(*rigs[0])
    host = calib_a.clone()
    host[6 * 24 + 9 + 0] += 25.0                                               # camera 0's fx in the MLP part only
    runner._in["calib"].copy_(host.cuda())
    runner._graph.replay()
    moved = [o.clone() for o in runner._outs]
    plain = model.forward_calibrated(img, host.cuda())
    torch.cuda.synchronize()
    assert runner._graph is graph
    for n, a, b in zip(NAMES, moved, plain):
        assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), n
    assert not torch.equal(moved[5], seen[0])


def _batched(rigs):
    return tuple(None if rigs[0][i] is None else torch.cat([r[i] for r in rigs], 0) for i in range(6))


def test_runner_batch_two_and_sample_independence(frame):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, imgs, rigs = frame["hip"], frame["imgs"], frame["rigs"]
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True, batch=2)
    pair = _batched(rigs[:2])
    out = [o.clone() for o in runner.step(imgs, *pair)]
    calib2 = model.view.calibration_matrices_batched(*pair).cuda()
    assert calib2.shape == (2, 6 * 51 + 9)
    eager = model.forward_calibrated(imgs, calib2)
    torch.cuda.synchronize()
    for n, a, b in zip(NAMES, out, eager):
        assert a.shape[0] == 2 and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), n
    graph = runner._graph
    # another calibration for sample 1 only: sample 0 keeps its bits, sample 1 follows, no new capture
    pair_b = _batched([rigs[0], rigs[2]])
    out_b = [o.clone() for o in runner.step(imgs, *pair_b)]
    torch.cuda.synchronize()
    assert runner._graph is graph
    for n, a, b in zip(NAMES, out, out_b):
        assert torch.equal(a[0].contiguous().view(torch.int16), b[0].contiguous().view(torch.int16)), n
    assert not torch.equal(out[5][1], out_b[5][1])
    # the other way round, eagerly: sample 0 replaced, sample 1 keeps its bits (the project's statement of independence,
    # tests/test_bevdet_batch_gpu.py: same B, another neighbour -- a batch-1 run takes other tile shapes)
    calib_c = model.view.calibration_matrices_batched(*_batched([rigs[2], rigs[1]])).cuda()
    out_c = model.forward_calibrated(torch.stack([imgs[1], imgs[1]]), calib_c)
    torch.cuda.synchronize()
    for n, a, c in zip(NAMES, out, out_c):
        assert torch.equal(a[1].contiguous().view(torch.int16), c[1].contiguous().view(torch.int16)), n
        assert not torch.equal(a[0], c[0])


def test_capture_guard_and_weight_reload(frame):
    from bevformer_tensorrt_amd.bevdet import synthetic_rig
    model = _build("hip", torch.float16, state=frame["hip"].state_dict())
    calib = model.view.calibration_matrices(*synthetic_rig(model.view)).cuda()
    img = frame["img"]
    assert model.view.depth_net_merged(build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.forward_calibrated(img, calib)
        with pytest.raises(RuntimeError):
            model.prepare_bev_half()
    del graph
    assert model.view.depth_net_merged(build=False) is None                  # nothing was built inside the capture
    first = [o.clone() for o in model.forward_calibrated(img, calib)]
    assert model.view.depth_net_merged(build=False) is not None
    # a reload: the last 1 x 1 of the DepthNet now prefers depth bin 7 everywhere -- the packed operands are rebuilt
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["view.depth_net.depth_conv.4.weight"].zero_()
    sd["view.depth_net.depth_conv.4.bias"].zero_()
    sd["view.depth_net.depth_conv.4.bias"][7] = 30.0
    model.load_state_dict(sd)
    assert model.view.depth_net_merged(build=False) is None                  # stale
    x = model.image_features(img.flatten(0, 1))
    depth, _, fast = model.view._depth_feat(x, model.view.split_calibration(calib)[1])
    torch.cuda.synchronize()
    assert fast and model.view.depth_net_merged(build=False) is not None
    assert bool((depth[:, 7] > 0.999).all())
    new = model.forward_calibrated(img, calib)
    assert not torch.equal(new[5], first[5])
    # a gate parameter alone
    with torch.no_grad():
        model.view.depth_net.context_se.conv_expand.bias.add_(1.0)
    assert model.view.depth_net_merged(build=False) is None


def test_int8_build_refuses_the_bevdepth_model(frame):
    from bevformer_tensorrt_amd import quantization as Q
    with pytest.raises(NotImplementedError, match="BEVDepth"):
        Q.build_int8_bevdet(frame["hip"], torch.device("cuda"), [])


def frame_digest(outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(o.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


# sha-256 of the six maps of one default-configuration frame (below), taken from a build of the PARENT commit on the
# same MI355X in the session that added bevdepth.py: BEVDet() keeps its modules, its launches and its bits
PARENT_DIGEST = "496f7f43e2f6e68fc9ccd726dbdb9058d3e889699d7d839586cc221e79ce230a"


def default_frame():
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    model = BEVDet(seed=0, bev_half="hip").cuda().half()
    calib = model.view.calibration_matrices(*jittered_rig(model.view, 5)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(3)).cuda().half()
    model.forward_calibrated(img, calib)
    outs = model.forward_calibrated(img, calib)
    torch.cuda.synchronize()
    return model, outs


def test_default_bevdet_keeps_the_parent_commits_bits():
    from bevformer_tensorrt_amd.bevdet import LSSViewTransformer
    model, outs = default_frame()
    assert type(model.view) is LSSViewTransformer and type(model.view.depth_net) is torch.nn.Conv2d
    assert not any("depth_net.depth_conv" in k or "depth_mlp" in k for k in model.state_dict())
    assert frame_digest(outs) == PARENT_DIGEST
