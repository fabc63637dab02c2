"""CPU-only: the transposed convolution's weight pack and parity / tap map (functions/deconv.py) against
F.conv_transpose2d in float64, the pre-launch status contract of the three bevops_deconv4x4s2 entries, the BN fold behind a
transposed convolution, mmdet's CenterNet key map and the CenterNet head merge (checkpoint.py, centernet.py)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_exact_dense as X

F32, F16, I8 = 0, 1, 2
SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


# ------------------------------------------------------------------------------------------------ pack and parity map
def four_gemms(x, packed, bias=None):
    """The kernel's arithmetic as numpy statements over the packed weight, float64: x [B, H, W, Cin], packed
    [4, Cout, 2, 2, Cin].  Per parity (py, px) ONE matrix product of the [B H W, 4 Cin] rows gathered from the zero-padded
    input (k ordered [dy][dx][Cin], tap (dy, dx) = input pixel (y - 1 + py + dy, x - 1 + px + dx)) with the parity's
    [Cout, 4 Cin] matrix -> out [B, 2H, 2W, Cout]."""
    B, H, W, Cin = x.shape
    Cout = packed.shape[1]
    xp = np.zeros((B, H + 2, W + 2, Cin))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((B, 2 * H, 2 * W, Cout))
    for py in range(2):
        for px in range(2):
            rows = np.concatenate([xp[:, py + dy:py + dy + H, px + dx:px + dx + W] for dy in range(2) for dx in range(2)],
                                  axis=-1).reshape(B * H * W, 4 * Cin)
            prod = rows @ packed[2 * py + px].reshape(Cout, 4 * Cin).T
            out[:, py::2, px::2] = prod.reshape(B, H, W, Cout)
    return out if bias is None else out + bias


@pytest.mark.parametrize("case", [(1, 1, 1, 32, 8), (2, 3, 5, 64, 24), (1, 7, 4, 32, 72)], ids=str)
def test_pack_and_parity_map_equal_conv_transpose2d_exactly(case):
    from bevformer_tensorrt_amd.functions.deconv import deconv4x4s2_tap, pack_deconv4x4s2
    B, H, W, Cin, Cout = case
    r = X._rng("deconv cpu", case)
    x, w = X.gen_f16_small(r, (B, H, W, Cin)), X.gen_f16_small(r, (Cin, Cout, 4, 4))
    bias = X.gen_bias(r, Cout, X.F16)
    packed = pack_deconv4x4s2(torch.from_numpy(w))
    assert packed.shape == (4, Cout, 2, 2, Cin) and packed.is_contiguous() and packed.dtype == torch.float16
    # every weight lands in exactly one (parity, tap) slot
    idx = pack_deconv4x4s2(torch.arange(Cin * Cout * 16, dtype=torch.float64).reshape(Cin, Cout, 4, 4))
    assert sorted(idx.flatten().tolist()) == list(range(Cin * Cout * 16))
    seen = set()
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    (oy, ox), (ky, kx) = deconv4x4s2_tap(py, px, dy, dx)
                    assert 2 * (oy + 0) + ky - 1 == py and 2 * ox + kx - 1 == px      # out = 2 * in - padding + k
                    seen.add((ky, kx))
                    assert torch.equal(idx[2 * py + px, :, dy, dx, :], idx.new_tensor(
                        np.arange(Cin * Cout * 16).reshape(Cin, Cout, 4, 4)[:, :, ky, kx].T.copy()))
    assert len(seen) == 16
    x64, w64, b64 = (torch.from_numpy(t.astype(np.float64)) for t in (x, w, bias))
    want = F.conv_transpose2d(x64.permute(0, 3, 1, 2), w64, b64, stride=2, padding=1).permute(0, 2, 3, 1).numpy()
    got = four_gemms(x.astype(np.float64), packed.numpy().astype(np.float64), bias.astype(np.float64))
    assert np.array_equal(got, want)            # dyadic operands: float64 sums are exact in any order
    assert np.abs(want).max() * 2.0 ** 8 < 2.0 ** 24 and want.any()


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_symbols_resolve_and_are_not_registry_functions(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_deconv4x4s2_f16", "bevops_deconv4x4s2_pack_weight", "bevops_deconv4x4s2_packed_weight_size"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    assert "conv_transpose2d_nhwc" in fn.__all__ and bev.conv_transpose2d_nhwc is fn.conv_transpose2d_nhwc
    assert "conv_transpose2d_nhwc" not in bev.TRT_FUNCTIONS


def test_status_codes_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced

    def fwd(dt=F16, x=p, w=p + 256, b=p + 512, o=p + 768, B=1, H=4, W=4, Cin=32, Cout=8, ks=4, s=2, pad=1):
        return lib.bevops_deconv4x4s2_f16(dt, x, w, b, o, B, H, W, Cin, Cout, ks, s, pad, 0, None)

    assert fwd(Cin=48) == NOT_SUPPORTED and fwd(Cin=16) == NOT_SUPPORTED
    assert fwd(Cout=12) == NOT_SUPPORTED
    assert fwd(dt=F32) == NOT_SUPPORTED and fwd(dt=I8) == NOT_SUPPORTED
    assert fwd(ks=3) == NOT_SUPPORTED and fwd(s=1) == NOT_SUPPORTED and fwd(pad=0) == NOT_SUPPORTED
    assert fwd(H=0) == BAD_PARAM and fwd(W=-1) == BAD_PARAM and fwd(B=-1) == BAD_PARAM and fwd(Cin=0) == BAD_PARAM
    assert fwd(x=None) == BAD_PARAM and fwd(w=None) == BAD_PARAM and fwd(o=None) == BAD_PARAM
    assert fwd(x=p + 8) == BAD_PARAM and fwd(w=p + 264) == BAD_PARAM and fwd(o=p + 770) == BAD_PARAM
    assert fwd(B=0) == SUCCESS and fwd(B=0, b=None) == SUCCESS
    # the activation is addressed through 32-bit byte offsets: 0xFFFFFF00 bytes and more are refused
    assert fwd(B=1, H=32768, W=2048, Cin=32) == NOT_SUPPORTED          # 2^32 bytes
    size = lib.bevops_deconv4x4s2_packed_weight_size
    assert size(F16, 64, 64) == 16 * 64 * 64 * 2 and size(F16, 32, 8) == 16 * 32 * 8 * 2
    assert size(F16, 48, 64) == 0 and size(F16, 64, 12) == 0 and size(F32, 64, 64) == 0 and size(F16, 0, 8) == 0
    pack = lib.bevops_deconv4x4s2_pack_weight
    assert pack(F16, None, p, 32, 8, None) == BAD_PARAM and pack(F16, p, None, 32, 8, None) == BAD_PARAM
    assert pack(F16, p, p + 256, 48, 8, None) == NOT_SUPPORTED and pack(F32, p, p + 256, 32, 8, None) == NOT_SUPPORTED


def test_wrapper_checks_its_arguments_before_any_device_call():
    import bevformer_tensorrt_amd as bev
    x = torch.zeros(1, 32, 2, 2, dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(AssertionError):
        bev.conv_transpose2d_nhwc(x, torch.zeros(32, 8, 4, 4, dtype=torch.float16))        # not a device tensor
    with pytest.raises(ValueError):
        bev.pack_deconv4x4s2(torch.zeros(32, 8, 3, 3))


# ------------------------------------------------------------------------------------------------ BN fold
def test_fold_deconv_bn():
    from bevformer_tensorrt_amd.checkpoint import BN_EPS, fold_deconv_bn
    g = torch.Generator().manual_seed(3)
    cin, cout = 6, 10
    x = torch.randn(2, cin, 5, 4, generator=g, dtype=torch.float64)
    w = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64)
    gamma, beta, mean = (torch.randn(cout, generator=g, dtype=torch.float64) for _ in range(3))
    var = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    for cb in (None, torch.randn(cout, generator=g, dtype=torch.float64)):
        want = F.batch_norm(F.conv_transpose2d(x, w, cb, 2, 1), mean, var, gamma, beta, False, 0.0, BN_EPS)
        wf, bf = fold_deconv_bn(w, cb, gamma, beta, mean, var)
        got = F.conv_transpose2d(x, wf, bf, 2, 1)
        assert wf.shape == w.shape and bf.shape == (cout,)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------ key map
def _mmdet_state_dict(model, g):
    """A synthetic state dict with mmdet 2.x's CenterNet key names and shapes, built from the NAMES alone (not from the
    key map under test): ResNet-18, CTResNetNeck(use_dcn), CenterNetHead."""
    sd = {}
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)

    def bn(prefix, c):
        sd[prefix + ".weight"], sd[prefix + ".bias"], sd[prefix + ".running_mean"] = rnd(c), rnd(c), rnd(c)
        sd[prefix + ".running_var"] = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
        sd[prefix + ".num_batches_tracked"] = torch.tensor(7)

    sd["backbone.conv1.weight"] = rnd(64, 3, 7, 7)
    bn("backbone.bn1", 64)
    cin = 64
    for i in range(4):
        planes = 64 * 2 ** i
        for j in range(2):
            ref = f"backbone.layer{i + 1}.{j}"
            sd[ref + ".conv1.weight"] = rnd(planes, cin if j == 0 else planes, 3, 3)
            bn(ref + ".bn1", planes)
            sd[ref + ".conv2.weight"] = rnd(planes, planes, 3, 3)
            bn(ref + ".bn2", planes)
            if j == 0 and i > 0:
                sd[ref + ".downsample.0.weight"] = rnd(planes, cin, 1, 1)
                bn(ref + ".downsample.1", planes)
        cin = planes
    for i, c in enumerate((256, 128, 64)):
        ref = f"neck.deconv_layers.{2 * i}"
        sd[ref + ".conv.weight"] = rnd(c, cin, 3, 3)
        sd[ref + ".conv.conv_offset.weight"], sd[ref + ".conv.conv_offset.bias"] = rnd(27, cin, 3, 3), rnd(27)
        bn(ref + ".bn", c)
        ref = f"neck.deconv_layers.{2 * i + 1}"
        sd[ref + ".conv.weight"] = rnd(c, c, 4, 4)
        bn(ref + ".bn", c)
        cin = c
    for k, n in (("heatmap", 80), ("wh", 2), ("offset", 2)):
        sd[f"bbox_head.{k}_head.0.weight"], sd[f"bbox_head.{k}_head.0.bias"] = rnd(64, 64, 3, 3), rnd(64)
        sd[f"bbox_head.{k}_head.2.weight"], sd[f"bbox_head.{k}_head.2.bias"] = rnd(n, 64, 1, 1), rnd(n)
    return sd


def test_centernet_key_map_assigns_every_parameter_once():
    from bevformer_tensorrt_amd.centernet import CenterNet
    from bevformer_tensorrt_amd.checkpoint import (centernet_key_map, fold_conv_bn, fold_deconv_bn,
                                                   load_centernet_state_dict)
    model = CenterNet().double()
    sd = _mmdet_state_dict(model, torch.Generator().manual_seed(5))
    kmap = centernet_key_map(model)
    own = dict(model.named_parameters())
    assert set(kmap) == set(own)                          # every parameter has exactly one source, and nothing else has
    before = {k: v.detach().clone() for k, v in own.items()}
    missing, unexpected = load_centernet_state_dict(model, sd, strict=True)
    assert missing == [] and unexpected == []
    assert all(not torch.equal(before[k], own[k]) for k in own), "a parameter kept its initial value"
    # every reference tensor (but the BN counters) is the source of some parameter
    used = set()
    for src in kmap.values():
        if isinstance(src, tuple):
            _, conv, bnp = src
            used.update([conv + ".weight"] + [f"{bnp}.{n}" for n in ("weight", "bias", "running_mean", "running_var")])
        else:
            used.add(src)
    assert used == {k for k in sd if not k.endswith("num_batches_tracked")}
    # spot values: a folded convolution, a folded transposed convolution, a copied tensor
    bnv = lambda p: [sd[f"{p}.{n}"] for n in ("weight", "bias", "running_mean", "running_var")]
    w, b = fold_conv_bn(sd["backbone.layer2.0.downsample.0.weight"], None, *bnv("backbone.layer2.0.downsample.1"))
    assert torch.equal(own["backbone.stages.1.0.downsample.weight"], w)
    assert torch.equal(own["backbone.stages.1.0.downsample.bias"], b)
    w, b = fold_deconv_bn(sd["neck.deconv_layers.3.conv.weight"], None, *bnv("neck.deconv_layers.3.bn"))
    assert torch.equal(own["neck.deconv.1.weight"], w) and torch.equal(own["neck.deconv.1.bias"], b)
    w, b = fold_conv_bn(sd["neck.deconv_layers.4.conv.weight"], None, *bnv("neck.deconv_layers.4.bn"))
    assert torch.equal(own["neck.dcn.2.weight"], w) and torch.equal(own["neck.dcn.2.bias"], b)
    assert torch.equal(own["neck.dcn.0.conv_offset.weight"], sd["neck.deconv_layers.0.conv.conv_offset.weight"])
    assert torch.equal(own["heads.wh.1.bias"], sd["bbox_head.wh_head.2.bias"])
    # a key nobody asked for is reported, and refused under strict
    sd["neck.deconv_layers.6.conv.weight"] = torch.zeros(1)
    assert load_centernet_state_dict(model, sd, strict=False) == ([], ["neck.deconv_layers.6.conv.weight"])
    with pytest.raises(KeyError):
        load_centernet_state_dict(model, sd, strict=True)


# ------------------------------------------------------------------------------------------------ head merge
@torch.no_grad()
def test_merged_head_equals_its_branches():
    from bevformer_tensorrt_amd.centernet import HEADS, CenterNet, merge_centernet_heads
    model = CenterNet(seed=4).double()
    g = torch.Generator().manual_seed(6)
    for h in model.heads.values():
        for c in h:
            c.bias.data = torch.randn(c.bias.shape, generator=g, dtype=torch.float64)
    hs = [model.heads[k] for k in HEADS]
    w1, b1, w2, b2, slices = merge_centernet_heads([(h[0].weight, h[0].bias) for h in hs],
                                                   [(h[1].weight, h[1].bias) for h in hs])
    assert w1.shape == (192, 64, 3, 3) and w2.shape == (88, 192, 1, 1) and slices == [(0, 80), (80, 82), (82, 84)]
    x = torch.randn(2, 64, 5, 7, generator=g, dtype=torch.float64)
    packed = F.conv2d(F.relu(F.conv2d(x, w1, b1, 1, 1)), w2, b2)
    for h, (a, b) in zip(hs, slices):
        want = F.conv2d(F.relu(F.conv2d(x, h[0].weight, h[0].bias, 1, 1)), h[1].weight, h[1].bias)
        assert float((packed[:, a:b] - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert not packed[:, 84:].any()
    # the model caches the merged operands and rebuilds them when a source changes
    m0 = model.heads_merged()
    assert model.heads_merged() is m0 and model.heads_merged(build=False) is m0
    model.heads["wh"][1].weight.mul_(2.0)
    assert model.heads_merged(build=False) is None and model.heads_merged() is not m0


def test_forward_rejects_sizes_that_are_no_multiple_of_32():
    from bevformer_tensorrt_amd.centernet import CenterNet
    model = CenterNet()
    for shape in ((1, 3, 48, 64), (1, 3, 64, 40), (1, 4, 64, 64), (3, 64, 64)):
        with pytest.raises(ValueError):
            model(torch.zeros(shape))
