"""CPU-only: the grouped, unmodulated deformable convolution of the DepthNet's DCN layer (design/bevdepth_dcn.md).

The premise of the exact GPU tests on the float64 statement alone (tests/util_dcn.py: dcn_ref with a ones mask on the
lattice), the CPU `deform_conv2d` statement against it and against the C oracle, group isolation, every pre-launch
status of bevops_deform_conv3x3_nhwc_f16 in the order include/bevops.h states, and the model side: the width rule, the
state_dict names and `depth_conv` indices, the checkpoint key map, and what stays refused."""
import ctypes

import numpy as np
import pytest
import torch

import util_dcn as U
from bevformer_tensorrt_amd.functions import deform_conv2d

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3

# (B, H, W, Cin, Cout, groups): the issue's cases
PREMISE = [(2, 6, 7, 128, 128, 4), (2, 6, 7, 256, 256, 4), (1, 16, 44, 256, 256, 4)]


def _lattice(B, H, W, cin, cout, groups):
    lat = U.lattice(B, cin, cout, H, W, 1, 1, 1, groups, 1)
    ones = torch.ones(B, 9, H, W)
    return lat, ones


@pytest.fixture(scope="module")
def small():
    lat, ones = _lattice(2, 6, 7, 128, 128, 4)
    return lat, ones, U.dcn_ref(lat["x"], lat["offset"], ones, lat["weight"], None, 1, 1, 1, 4, 1)


@pytest.mark.parametrize("B,H,W,cin,cout,groups", PREMISE)
def test_premise_of_the_exact_tests(B, H, W, cin, cout, groups):
    lat, ones = _lattice(B, H, W, cin, cout, groups)
    out = U.dcn_ref(lat["x"], lat["offset"], ones, lat["weight"], lat["bias"], 1, 1, 1, groups, 1)
    assert torch.equal(out.float().double(), out)                             # exact in fp32: any summation order
    moved = (out.half().double() != out).double().mean().item()
    nonzero = (out != 0).double().mean().item()
    print(f"{(B, H, W, cin, cout, groups)}: {moved:.3f} change under the fp16 rounding, {nonzero:.3f} non-zero")
    assert moved >= 0.10 and nonzero >= 0.5
    assert bool(torch.isfinite(out.half()).all())


def test_cpu_statement_equals_dcn_ref_on_the_lattice(small):
    lat, ones, want = small
    got64 = deform_conv2d(lat["x"].double(), lat["offset"].double(), lat["weight"].double(), 1, 1, 1, 4, 1)
    assert got64.dtype == torch.float64 and torch.equal(got64, want)
    got32 = deform_conv2d(lat["x"], lat["offset"], lat["weight"], 1, 1, 1, 4, 1)
    assert got32.dtype == torch.float32 and torch.equal(got32, want.float())
    assert (want != 0).double().mean().item() >= 0.5


def test_cpu_statement_agrees_with_the_c_oracle():
    """oracle.mdconv with a ones mask: written independently (C, fp32).  Gaussian operands, offsets of about a pixel."""
    import oracle
    g = torch.Generator().manual_seed(3)
    B, C, H, W, G = 2, 64, 5, 9, 4
    x, off = torch.randn(B, C, H, W, generator=g), torch.randn(B, 18, H, W, generator=g) * 1.5
    w = torch.randn(C, C // G, 3, 3, generator=g) * 0.1
    got = deform_conv2d(x, off, w, 1, 1, 1, G, 1)
    want = torch.from_numpy(oracle.mdconv(x.numpy(), off.numpy(), np.ones((B, 9, H, W), np.float32), w.numpy(), None,
                                          (1, 1), (1, 1), (1, 1), G, 1))
    k = 9 * C // G
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"deform_conv2d (CPU) vs oracle.mdconv: {err:.3e} at max |out| {scale:.3f}")
    assert scale > 1.0 and err <= (k + 8) * 2.0 ** -24 * 4.0 * scale         # fp32 accumulation over K terms, twice
    # other strides / dilations / deform groups go through the same statement
    off2 = torch.randn(B, 2 * 18, 3, 5, generator=g)
    got2 = deform_conv2d(x, off2, w, 2, 2, 2, G, 2)
    want2 = U.dcn_ref(x, off2, torch.ones(B, 18, 3, 5), w, None, 2, 2, 2, G, 2)
    assert float((got2.double() - want2).abs().max()) <= 1e-4 * float(want2.abs().max())


def test_group_isolation(small):
    lat, _, want = small
    x2 = lat["x"].clone()
    x2[:, :32] = x2[:, :32] * 0.5 + 1.0                                        # group 0's input channels
    got = deform_conv2d(x2, lat["offset"], lat["weight"], 1, 1, 1, 4, 1)
    assert torch.equal(got[:, 32:], want[:, 32:].float())
    assert not torch.equal(got[:, :32], want[:, :32].float())


# ---- the entry's pre-launch statuses

@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    return (ctypes.addressof(buf) + 255) & ~255, buf          # aligned host address: never dereferenced


def test_symbol_resolves_and_is_exported(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    name = "bevops_deform_conv3x3_nhwc_f16"
    assert name in SIGNATURES
    assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    for f in ("deform_conv2d", "deform_conv2d_nhwc"):
        assert f in fn.__all__ and getattr(bev, f) is getattr(fn, f) and f not in bev.TRT_FUNCTIONS


def test_status_codes(lib, p):
    p = p[0]

    def call(x=p, off=p + 256, oc=32, w=p + 512, b=None, out=p + 768, relu=0, B=1, H=4, W=5, cin=128, cout=128, g=4):
        return lib.bevops_deform_conv3x3_nhwc_f16(x, off, oc, w, b, out, relu, B, H, W, cin, cout, g, None)

    for k in ("x", "off", "w", "out"):
        assert call(**{k: None}) == BAD_PARAM, k
        assert call(**{k: p + 1024 + 8}) == BAD_PARAM, k
    assert call(b=p + 1024 + 2) == BAD_PARAM
    assert call(B=-1) == BAD_PARAM and call(H=0) == BAD_PARAM and call(W=0) == BAD_PARAM
    assert call(cin=0) == BAD_PARAM and call(cout=0) == BAD_PARAM and call(g=0) == BAD_PARAM and call(g=-4) == BAD_PARAM
    assert call(relu=2) == BAD_PARAM and call(relu=-1) == BAD_PARAM
    assert call(oc=16) == BAD_PARAM and call(oc=19) == BAD_PARAM and call(oc=0) == BAD_PARAM
    # the domain, behind the parameter checks; answered for an empty batch too
    assert call(cin=130) == NOT_SUPPORTED and call(cout=130) == NOT_SUPPORTED
    assert call(cin=64) == NOT_SUPPORTED and call(cout=64) == NOT_SUPPORTED and call(cin=192, g=4) == NOT_SUPPORTED
    assert call(cin=64, B=0) == NOT_SUPPORTED
    assert call(cin=64, oc=16) == BAD_PARAM and call(cin=64, x=None) == BAD_PARAM
    # size limits: the 32-bit pixel index, the grid's row count
    assert call(B=1 << 15, H=1 << 8, W=1 << 8) == NOT_SUPPORTED
    assert call(B=1, H=1 << 16, W=1 << 16) == NOT_SUPPORTED
    assert call(B=0, cin=32 * 65536, cout=32 * 65536, g=65536) == NOT_SUPPORTED
    # an empty batch inside the domain: success, nothing launched (no device is needed)
    assert call(B=0) == SUCCESS and call(B=0, oc=18, b=p + 1024, relu=1) == SUCCESS
    assert call(B=0, cin=32, cout=32, g=1) == SUCCESS and call(B=0, cin=256, cout=128, g=4) == SUCCESS


# ---- the model

def test_width_rule():
    from bevformer_tensorrt_amd.bevdepth import DeformConv2dPack, DepthNet
    for mid in (128, 256):
        net = DepthNet(mid, mid, 16, 8, use_dcn=True)
        assert isinstance(net.depth_conv[4], DeformConv2dPack) and net.dcn is net.depth_conv[4] and net.use_dcn
    for mid in (16, 64, 192):
        with pytest.raises(NotImplementedError, match="DCN") as e:
            DepthNet(mid, mid, 16, 8, use_dcn=True)
        assert "% 128" in str(e.value)
    assert DepthNet(16, 16, 16, 8).dcn is None and not DepthNet(16, 16, 16, 8).use_dcn


def test_state_dict_names_shapes_and_indices():
    from bevformer_tensorrt_amd.bevdepth import ASPP, DepthNet
    from bevformer_tensorrt_amd.checkpoint import depthnet_key_map, depthnet_reference_keys, load_depthnet_state_dict
    net = DepthNet(128, 128, 16, 8, use_dcn=True)
    sd = net.state_dict()
    assert tuple(sd["depth_conv.4.weight"].shape) == (128, 32, 3, 3) and "depth_conv.4.bias" not in sd
    assert tuple(sd["depth_conv.4.conv_offset.weight"].shape) == (18, 128, 3, 3)
    assert tuple(sd["depth_conv.4.conv_offset.bias"].shape) == (18,)
    assert tuple(sd["depth_conv.5.weight"].shape) == (8, 128, 1, 1) and tuple(sd["depth_conv.5.bias"].shape) == (8,)
    assert isinstance(net.depth_conv[3], ASPP) and len(net.depth_conv) == 6
    d = net.depth_conv[4]
    assert (d.groups, d.deform_groups, d.in_channels, d.out_channels) == (4, 1, 128, 128)
    assert float(d.conv_offset.weight.detach().abs().max()) == 0.0 and float(d.conv_offset.bias.detach().abs().max()) == 0.0   # mmcv's init
    assert float(d.weight.detach().std()) > 0
    # the key map covers every parameter; the reference's list has the three new names and the shifted last layer
    km = depthnet_key_map(net)
    assert set(km) == {n for n, _ in net.named_parameters()}
    pre = "img_view_transformer.depth_net."
    keys = depthnet_reference_keys(net)
    for n in ("depth_conv.4.weight", "depth_conv.4.conv_offset.weight", "depth_conv.4.conv_offset.bias",
              "depth_conv.5.weight", "depth_conv.5.bias"):
        assert pre + n in keys, n
    assert pre + "depth_conv.4.bias" not in keys
    without = depthnet_reference_keys(DepthNet(128, 128, 16, 8))
    assert set(keys) - set(without) == {pre + "depth_conv.4.conv_offset.weight", pre + "depth_conv.4.conv_offset.bias",
                                        pre + "depth_conv.5.weight", pre + "depth_conv.5.bias"}
    # the loader fills the layer from the reference's names
    g = torch.Generator().manual_seed(0)
    names = ("depth_conv.4.weight", "depth_conv.4.conv_offset.weight", "depth_conv.4.conv_offset.bias",
             "depth_conv.5.weight", "depth_conv.5.bias")
    ref = {pre + n: torch.randn(sd[n].shape, generator=g) for n in names}
    other = DepthNet(128, 128, 16, 8, use_dcn=True)
    missing, unexpected = load_depthnet_state_dict(other, ref, strict=False)
    assert not unexpected and not any(m.startswith(("depth_conv.4", "depth_conv.5")) for m in missing) and missing
    for n in names:
        assert torch.equal(other.state_dict()[n], ref[pre + n]), n


def test_plain_forward_with_zero_offsets_is_a_grouped_convolution():
    import torch.nn.functional as F
    from bevformer_tensorrt_amd.bevdepth import DeformConv2dPack
    torch.manual_seed(0)
    d = DeformConv2dPack(128, 128).double()
    x = torch.randn(1, 128, 5, 6, dtype=torch.float64)
    with torch.no_grad():
        got, want = d(x), F.conv2d(x, d.weight, None, 1, 1, 1, 4)
        assert float((got - want).abs().max()) <= 1e-12
        d.conv_offset.bias.fill_(0.5)
        assert float((d(x) - want).abs().max()) > 1e-3                        # live offsets: another result


def test_int8_build_refuses_and_the_configs():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDEPTH_R50_DCN, BEVDET_R50
    assert BEVDEPTH_R50 == dict(BEVDET_R50, view_transformer="bevdepth", depthnet_cfg=dict(use_dcn=False))
    assert BEVDEPTH_R50_DCN == dict(BEVDET_R50, view_transformer="bevdepth", depthnet_cfg=dict(use_dcn=True))

    class _Model(torch.nn.Module):
        cfg = BEVDEPTH_R50_DCN

    def frames():
        raise AssertionError("a frame ran")
        yield

    for half in ("int8", "fp16"):
        with pytest.raises(NotImplementedError, match="DCN"):
            Q.build_int8_bevdet(_Model(), torch.device("cpu"), frames(), bev_half=half)
        with pytest.raises(NotImplementedError, match="DCN"):
            Q.build_int8_bevdet(None, torch.device("cpu"), frames(), bev_half=half, cfg=BEVDEPTH_R50_DCN)


def test_depthnet_plain_path_runs_on_the_cpu():
    from bevformer_tensorrt_amd.bevdepth import DepthNet
    torch.manual_seed(1)
    net = DepthNet(128, 128, 16, 8, use_dcn=True).eval()
    with torch.no_grad():
        net.dcn.conv_offset.weight.normal_(0, 0.02)
        x, v = torch.randn(2, 128, 4, 5), torch.randn(2, 27)
        y = net(x, v)
        net.dcn.conv_offset.weight.zero_()
        y0 = net(x, v)
    assert y.shape == (2, 8 + 16, 4, 5) and bool(torch.isfinite(y).all())
    assert float((y[:, :8] - y0[:, :8]).abs().max()) > 1e-4 and torch.equal(y[:, 8:], y0[:, 8:])   # depth rows only
