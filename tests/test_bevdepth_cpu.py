"""CPU-only: BEVDepth's DepthNet and view transformer (bevformer_tensorrt_amd/bevdepth.py) against the fixture
tests/golden/bevdepth.npz, which tests/golden/make_bevdepth_golden.py records by EXECUTING the reference's own classes
(lifted by AST) in fp32 -- get_mlp_input bit for bit, the re-hosted plain path within 1e-5 of the lifted forward (the
BatchNorm fold moves roundings; the project's bar for its re-hosted wrappers), the two parts of the packed calibration
row, the per-image-bias fold of ASPP's pooled branch in float64, the checkpoint's key list, and what the variant
refuses.  mmdet's BasicBlock is restated by the fixture script (not installed): parity with mmdet's class is unpinned."""
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import golden


@pytest.fixture(scope="module")
def G():
    return golden("bevdepth")


@pytest.fixture(scope="module")
def net(G):
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.checkpoint import load_depthnet_state_dict
    m = DepthNet(16, 16, 16, 8).eval()
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G if k.startswith("sd.")}
    missing, unexpected = load_depthnet_state_dict(m, sd, strict=True)
    assert not missing and not unexpected
    return m


def _view(n_cams=2):
    from bevformer_tensorrt_amd.bevdepth import LSSViewTransformerBEVDepth
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50
    cfg = dict(BEVDET_R50, in_channels=16, out_channels=16)
    return LSSViewTransformerBEVDepth(**cfg, ops=object(), depthnet_cfg=dict(use_dcn=False))


def _rig(G):
    t = lambda k: torch.from_numpy(G[k])
    return t("sensor2ego"), None, t("cam2imgs"), t("post_rots"), t("post_trans"), t("bda")


def test_get_mlp_input_bit_for_bit(G):
    got = _view().get_mlp_input(*_rig(G))
    want = torch.from_numpy(G["mlp_input"])
    assert got.shape == want.shape == (1, 2, 27) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got[0, 0, 0]) > 1000.0                                         # a focal length: not an fp16 quantity


def test_plain_path_within_1e_5_of_the_lifted_forward(G, net):
    x, v = torch.from_numpy(G["x"]), torch.from_numpy(G["mlp_input"])
    with torch.no_grad():
        got = net(x, v)
        aspp = net.aspp(torch.from_numpy(G["aspp_in"]))
    want, want_aspp = torch.from_numpy(G["out"]), torch.from_numpy(G["aspp_out"])
    assert got.shape == want.shape == (2, 8 + 16, 6, 10)
    err, err_aspp = (got - want).abs().max().item(), (aspp - want_aspp).abs().max().item()
    print(f"DepthNet plain path vs lifted forward: {err:.3e} (max |want| {want.abs().max().item():.3f}); ASPP {err_aspp:.3e}")
    assert err <= 1e-5 and err_aspp <= 1e-5
    assert want.std() > 0.05 and want[:, :8].std() > 0.01 and want[:, 8:].std() > 0.01
    # the gate is live: other calibration values, another result
    with torch.no_grad():
        other = net(x, v * 1.01)
    assert (other - got).abs().max().item() > 1e-3


def test_calibration_row_has_the_parents_part_then_the_mlp_inputs(G):
    from bevformer_tensorrt_amd.bevdet import LSSViewTransformer
    view, rig = _view(), _rig(G)
    row = view.calibration_matrices(*rig)
    assert row.shape == (2 * 51 + 9,) and row.dtype == torch.float32 and row.is_contiguous()
    geo, mlp = view.split_calibration(row)
    parent = LSSViewTransformer.calibration_matrices(view, *rig)
    assert torch.equal(geo, parent) and geo.data_ptr() == row.data_ptr()
    assert torch.equal(mlp.view(torch.int32), torch.from_numpy(G["mlp_input"]).reshape(2, 27).view(torch.int32))
    # batched: row b is sample b's own row; the split gives dense tables
    rig2 = tuple(None if t is None else torch.cat([t, t * 1.0], 0) for t in rig)
    rows = view.calibration_matrices_batched(*rig2)
    assert rows.shape == (2, 2 * 51 + 9) and torch.equal(rows[0], row) and torch.equal(rows[1], row)
    geo2, mlp2 = view.split_calibration(rows)
    assert geo2.shape == (2, 2 * 24 + 9) and geo2.is_contiguous() and mlp2.shape == (4, 27) and mlp2.is_contiguous()
    assert torch.equal(geo2[1], parent) and torch.equal(mlp2[2:], mlp)
    # the geometry of the parent reads the long row through the split
    assert torch.equal(view.lidar_coor_plain(row), LSSViewTransformer.lidar_coor_plain(view, parent))
    with pytest.raises(ValueError):
        view.split_calibration(torch.zeros(2 * 24 + 9))


def test_pooled_branch_is_a_per_image_bias_of_conv1_in_float64(G, net):
    """A bilinear up-sampling of a 1 x 1 map is a constant, so the fifth input of ASPP's concatenation enters conv1 as
    conv1.weight[:, 4 mid:] @ x5 per image: the four-branch convolution plus that bias equals the five-branch one."""
    from bevformer_tensorrt_amd.bevdepth import fold_pooled_branch
    a = net.aspp.double()
    try:
        x = torch.from_numpy(G["aspp_in"]).double()
        with torch.no_grad():
            want = a(x)
            four = torch.cat([F.relu(F.conv2d(x, m.weight, m.bias, 1, m.padding, m.dilation)) for m in a.branches()], 1)
            bias = fold_pooled_branch(a, x.mean(dim=(2, 3)))
            got = F.relu(F.conv2d(four, a.conv1.weight[:, :4 * 16]) + bias[:, :, None, None])
        assert bias.shape == (2, 16) and (bias[0] - bias[1]).abs().max().item() > 1e-3
        assert (got - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())
    finally:
        net.float()


def test_key_list(G, net):
    from bevformer_tensorrt_amd.checkpoint import depthnet_key_map, depthnet_reference_keys
    assert depthnet_reference_keys(net) == sorted(G["keys"].tolist())
    own = {n for n, _ in net.named_parameters()}
    assert set(depthnet_key_map(net)) == own
    for name in ("reduce_conv", "context_conv", "bn", "depth_mlp", "depth_se", "context_mlp", "context_se", "depth_conv"):
        assert hasattr(net, name), name
    for name in ("aspp1", "aspp2", "aspp3", "aspp4", "global_avg_pool", "conv1"):
        assert hasattr(net.aspp, name), name
    assert [m.dilation[0] for m in net.aspp.branches()] == [1, 6, 12, 18]


def test_what_the_variant_refuses():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50
    with pytest.raises(NotImplementedError, match="DCN"):
        DepthNet(16, 16, 16, 8, use_dcn=True)
    with pytest.raises(NotImplementedError, match="stereo"):
        DepthNet(16, 16, 16, 8, stereo=True)
    assert BEVDEPTH_R50["view_transformer"] == "bevdepth" and BEVDEPTH_R50["depthnet_cfg"] == dict(use_dcn=False)

    class _Model(torch.nn.Module):
        cfg = BEVDEPTH_R50

    with pytest.raises(NotImplementedError, match="BEVDepth"):
        Q.build_int8_bevdet(_Model(), torch.device("cpu"), [])
    view = _view()
    with pytest.raises(ValueError, match="mlp_input"):
        view.view_transform(torch.zeros(2, 16, 16, 44), *([None] * 5))


def test_default_bevdet_has_no_new_module_and_never_imports_bevdepth():
    code = ("import sys\n"
            "from bevformer_tensorrt_amd.bevdet import BEVDet, LSSViewTransformer\n"
            "import torch\n"
            "m = BEVDet()\n"
            "assert type(m.view) is LSSViewTransformer and type(m.view.depth_net) is torch.nn.Conv2d\n"
            "assert m.view.calibration_matrices.__func__ is LSSViewTransformer.calibration_matrices\n"
            "assert 'bevformer_tensorrt_amd.bevdepth' not in sys.modules\n"
            "assert sum(1 for _ in m.view.modules()) == 2\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(__import__("pathlib").Path(
        __file__).resolve().parent.parent))
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
