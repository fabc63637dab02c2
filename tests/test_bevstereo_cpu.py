"""CPU-only: BEVStereo's DepthNet and view transformer (bevformer_tensorrt_amd/bevdepth.py: DepthNet(stereo=True),
LSSViewTransformerBEVStereo; bevdet.BEVSTEREO_R50) against the fixture tests/golden/bevstereo.npz, which
tests/golden/make_bevstereo_golden.py records by EXECUTING the reference's DepthNet (lifted by AST) in fp32: the plain
path within 1e-5 of the lifted forward (the bar of tests/test_bevdepth_cpu.py: the BatchNorm fold moves roundings) for
both biases and the first frame, the checkpoint's key list, the width rule, the INT8 refusal and the model's plumbing.
mmdet's BasicBlock is restated by the fixture script (not installed): parity with mmdet's class is unpinned."""
import pytest
import torch

from conftest import golden


@pytest.fixture(scope="module")
def G():
    return golden("bevstereo")


@pytest.fixture(scope="module")
def net(G):
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.checkpoint import load_depthnet_state_dict
    m = DepthNet(32, 32, 16, 6, stereo=True, bias=5.0).eval()
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G if k.startswith("sd.")}
    missing, unexpected = load_depthnet_state_dict(m, sd, strict=True)
    assert not missing and not unexpected
    return m


def _metas(G, prev=True):
    t = lambda k: torch.from_numpy(G[k])
    return dict(cv_feat_list=[t("prev") if prev else None, t("curr")], k2s_sensor=t("k2s_sensor"), intrins=t("intrins"),
                post_rots=t("post_rots"), post_trans=t("post_trans"), frustum=t("cv_frustum"),
                downsample=int(G["downsample"]), cv_downsample=int(G["cv_downsample"]))


def test_plain_path_within_1e_5_of_the_lifted_forward(G, net):
    x, v = torch.from_numpy(G["x"]), torch.from_numpy(G["mlp_input"])
    outs = {}
    try:
        for tag, bias, prev in (("b5", 5.0, True), ("b0", 0.0, True), ("first", 5.0, False)):
            net.bias = bias
            with torch.no_grad():
                got = net(x, v, _metas(G, prev))
            want = torch.from_numpy(G["out_" + tag])
            assert got.shape == want.shape == (2, 6 + 16, 2, 3)
            err = (got - want).abs().max().item()
            print(f"DepthNet(stereo) plain path vs lifted forward, {tag}: {err:.3e} (max |want| {want.abs().max().item():.3f})")
            assert err <= 1e-5, tag
            outs[tag] = want
    finally:
        net.bias = 5.0
    # the three cases differ where the cost volume enters (the depth logits), and only there
    for a, b in (("b5", "b0"), ("b5", "first")):
        assert (outs[a][:, :6] - outs[b][:, :6]).abs().max().item() > 1e-3
        assert torch.equal(outs[a][:, 6:], outs[b][:, 6:])
    with pytest.raises(ValueError, match="stereo_metas"):
        net(x, v)


def test_first_frame_runs_the_cost_volume_net_on_zeros(G, net):
    """The reference builds a zero cost volume and still runs cost_volumn_net on it: biases through two padded
    stride-2 convolutions are not constant at the borders."""
    with torch.no_grad():
        cv = net.cost_volume(_metas(G, prev=False), torch.zeros(2, 32, 2, 3))
        assert cv.shape == (2, 6, 8, 12) and not bool(cv.any())
        for m in net.cost_volumn_net:
            cv = m(cv)
    assert cv.shape == (2, 6, 2, 3)
    assert (cv[..., 0, 0] - cv[..., 1, 1]).abs().max().item() > 1e-3


def test_key_list(G, net):
    from bevformer_tensorrt_amd.checkpoint import depthnet_key_map, depthnet_reference_keys
    keys = sorted(G["keys"].tolist())
    assert depthnet_reference_keys(net) == keys
    assert set(depthnet_key_map(net)) == {n for n, _ in net.named_parameters()}
    p = "img_view_transformer.depth_net."
    for k in ("cost_volumn_net.0.weight", "cost_volumn_net.0.bias", "cost_volumn_net.1.running_var", "cost_volumn_net.2.weight",
              "cost_volumn_net.3.bias", "depth_conv.0.downsample.weight", "depth_conv.0.downsample.bias"):
        assert p + k in keys, k
    assert tuple(net.depth_conv[0].downsample.weight.shape) == (32, 38, 1, 1) and len(net.cost_volumn_net) == 2
    assert all(m.stride == (2, 2) and m.padding == (1, 1) and m.kernel_size == (3, 3) for m in net.cost_volumn_net)


def test_width_rule_and_what_is_refused():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdepth import DepthNet, LSSViewTransformerBEVDepth, LSSViewTransformerBEVStereo
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, BEVSTEREO_R50
    with pytest.raises(NotImplementedError, match=r"stereo.*mid_channels % 32"):
        DepthNet(16, 16, 16, 8, stereo=True)
    with pytest.raises(NotImplementedError, match="stereo"):
        DepthNet(48, 48, 16, 8, stereo=True)
    m = DepthNet(32, 32, 16, 8, stereo=True, bias=5.0)
    assert m.stereo and m.bias == 5.0 and m.stereo_padded() == 32
    assert DepthNet(32, 64, 16, 59, stereo=True).stereo_padded() == 64
    assert not DepthNet(16, 16, 16, 8).stereo and not hasattr(DepthNet(16, 16, 16, 8), "cost_volumn_net")
    assert BEVSTEREO_R50 == dict(BEVDET_R50, view_transformer="bevstereo",
                                 depthnet_cfg=dict(use_dcn=False, stereo=True, bias=5.0))

    class _Model(torch.nn.Module):
        cfg = BEVSTEREO_R50

    with pytest.raises(NotImplementedError, match="stereo"):
        Q.build_int8_bevdet(_Model(), torch.device("cpu"), [])
    with pytest.raises(NotImplementedError, match="stereo"):
        Q.build_int8_bevdet(_Model(), torch.device("cpu"), [], bev_half="int8")
    cfg = dict(BEVDET_R50, in_channels=32, out_channels=16)
    with pytest.raises(ValueError, match="stereo=True"):
        LSSViewTransformerBEVStereo(**cfg, ops=object(), depthnet_cfg=dict(use_dcn=False))
    plain = LSSViewTransformerBEVDepth(**cfg, ops=object(), depthnet_cfg=dict(use_dcn=False))
    with pytest.raises(ValueError, match="stereo_metas"):
        plain._depth_feat(torch.zeros(1, 32, 16, 44), torch.zeros(1, 27), dict())


def test_view_transformer_carries_cv_frustum_and_hands_the_metas_through(G, net):
    from bevformer_tensorrt_amd.bevdepth import STEREO_META_KEYS, LSSViewTransformerBEVStereo
    cfg = dict(grid_config=dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 7.0, 1.0]),
               input_size=(32, 48), downsample=16, in_channels=32, out_channels=16)
    view = LSSViewTransformerBEVStereo(**cfg, ops=object(), depthnet_cfg=dict(use_dcn=False, stereo=True, bias=5.0))
    assert view.D == 6 and view.frustum.shape == (6, 2, 3, 3)
    assert torch.equal(view.cv_frustum, torch.from_numpy(G["cv_frustum"]))
    assert "cv_frustum" not in view.state_dict()
    view.depth_net.load_state_dict(net.state_dict())
    view.eval()
    t = lambda k: torch.from_numpy(G[k])
    metas = view.stereo_metas(t("prev"), t("curr"), t("k2s_sensor"), t("intrins"), t("post_rots"), t("post_trans"))
    assert tuple(metas) == STEREO_META_KEYS and metas["downsample"] == 16 and metas["cv_downsample"] == 4
    depth, feat, fast = view._depth_feat(t("x"), t("mlp_input").reshape(2, 27), metas)
    want = t("out_b5")
    assert not fast and depth.shape == (2, 6, 2, 3) and feat.shape == (2, 2, 3, 16)
    assert (depth - want[:, :6].softmax(1)).abs().max().item() <= 1e-5
    assert (feat - want[:, 6:].permute(0, 2, 3, 1)).abs().max().item() <= 1e-5
    with pytest.raises(ValueError, match="stereo_metas"):
        view._depth_feat(t("x"), t("mlp_input").reshape(2, 27), None)
    with pytest.raises(ValueError, match="lacks"):
        view._depth_feat(t("x"), t("mlp_input").reshape(2, 27), dict(cv_feat_list=[None, t("curr")]))
    prepared = view.stereo_metas(None, t("curr"), t("k2s_sensor"), t("intrins"), t("post_rots"), t("post_trans"), prepare=True)
    assert prepared["consts"].shape == (2, 40) and [x.numel() for x in prepared["tables"]] == [12, 8, 6]


def test_model_plumbing():
    """BEVDet(BEVSTEREO_R50-shaped cfg): the backbone also returns its stride-4 stage, image_features(stereo=True) the
    pair of image_encoder; the other configurations keep their backbone and refuse the metas."""
    from bevformer_tensorrt_amd.bevdepth import LSSViewTransformerBEVStereo
    from bevformer_tensorrt_amd.bevdet import BEVSTEREO_R50, BEVDet
    m = BEVDet(dict(BEVSTEREO_R50, input_size=(64, 96)), ops=object(), bev_half="torch")
    assert type(m.view) is LSSViewTransformerBEVStereo and m.backbone.out_indices == (0, 2, 3) and m.view.D == 59
    assert m.view.cv_frustum.shape == (59, 16, 24, 3) and m.view.depth_net.stereo and m.view.depth_net.bias == 5.0
    img = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(0))
    x, feat = m.image_features(img, stereo=True)
    assert x.shape == (1, 256, 4, 6) and feat.shape == (1, 256, 16, 24)
    assert torch.equal(m.image_features(img), x)
    x2, kw = m._frame_features(img, dict(cv_feat_list=[None, None]))
    assert torch.equal(kw["stereo_metas"]["cv_feat_list"][1], feat) and kw["stereo_metas"]["cv_feat_list"][0] is None
    with pytest.raises(ValueError, match="stereo_metas"):
        m._frame_features(img, None)
    d = BEVDet(ops=object(), bev_half="torch")
    assert d.backbone.out_indices == (2, 3) and not d.stereo
    with pytest.raises(ValueError, match="BEVStereo"):
        d.image_features(img, stereo=True)
    with pytest.raises(ValueError, match="BEVStereo"):
        d._frame_features(img, dict())
    with pytest.raises(ValueError, match="bevstereo"):
        BEVDet(dict(BEVSTEREO_R50, view_transformer="nope"), ops=object())
