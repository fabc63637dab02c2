"""CPU-only: the pre-launch status contract of bevops_conv_slice_f16 (csrc/conv_slice.hip) and of the three entries of
csrc/yolox.hip, the channel padding of functions/yolox_ops.py and its inverse, and a float64 statement of "the padded
96-channel layer is the 80-channel layer", exact on a dyadic lattice."""
import ctypes

import numpy as np
import pytest
import torch

import util_exact_dense as X

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_char * 8192)()
    addr = (ctypes.addressof(buf) + 255) & ~255          # aligned host address: never dereferenced
    return addr, buf


def test_symbols_resolve_and_are_not_registry_functions(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.utils.lib import SIGNATURES
    for name in ("bevops_conv_slice_f16", "bevops_focus_nhwc", "bevops_spp_maxpool_nhwc", "bevops_upsample_nearest2x_nhwc"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    for name in ("conv_slice_nhwc", "focus_nhwc", "spp_maxpool_nhwc", "upsample_nearest2x_nhwc"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS


def test_conv_slice_status_codes_without_gpu(lib, p):
    p = p[0]

    def call(x=p, xp=32, w=p + 256, b=p + 512, r=None, rp=0, o=p + 768, op=8, B=1, H=4, W=4, Cin=32, Cout=8, ks=3, s=1,
             act=2):
        return lib.bevops_conv_slice_f16(x, xp, w, b, r, rp, o, op, B, H, W, Cin, Cout, ks, s, act, None)

    # outside the domain
    assert call(Cin=48, xp=48) == NOT_SUPPORTED and call(Cin=16, xp=16) == NOT_SUPPORTED
    assert call(Cout=12, op=16) == NOT_SUPPORTED
    assert call(ks=5) == NOT_SUPPORTED and call(ks=2) == NOT_SUPPORTED and call(s=3) == NOT_SUPPORTED
    assert call(act=3) == NOT_SUPPORTED and call(act=-1) == NOT_SUPPORTED
    # bad parameters
    assert call(H=0) == BAD_PARAM and call(W=-1) == BAD_PARAM and call(B=-1) == BAD_PARAM
    assert call(Cin=0) == BAD_PARAM and call(Cout=0) == BAD_PARAM and call(ks=0) == BAD_PARAM and call(s=0) == BAD_PARAM
    assert call(x=None) == BAD_PARAM and call(w=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(w=p + 264) == BAD_PARAM and call(o=p + 770) == BAD_PARAM
    assert call(r=p + 1024 + 8, rp=8) == BAD_PARAM and call(b=p + 513) == BAD_PARAM
    assert call(xp=24) == BAD_PARAM and call(op=0) == BAD_PARAM and call(r=p + 1024, rp=0) == BAD_PARAM   # pitch < channels
    assert call(xp=36) == BAD_PARAM and call(op=12) == BAD_PARAM and call(r=p + 1024, rp=12) == BAD_PARAM  # pitch % 8
    # nothing to do
    assert call(B=0) == SUCCESS and call(B=0, b=None) == SUCCESS and call(B=0, r=p + 1024, rp=16, xp=72, op=24) == SUCCESS
    # x is addressed through 32-bit byte offsets: B H W x_pitch of 0xFFFFFF00 bytes and more are refused
    assert call(B=1, H=32768, W=2048, Cin=32) == NOT_SUPPORTED                 # 2^32 bytes
    assert call(B=1, H=32768, W=1024, Cin=32, xp=64) == NOT_SUPPORTED          # the pitch counts, not the channels


def test_yolox_entries_status_codes_without_gpu(lib, p):
    p = p[0]

    def focus(img=p, o=p + 256, op=32, B=1, H=4, W=4):
        return lib.bevops_focus_nhwc(img, o, op, B, H, W, None)

    assert focus(H=3) == NOT_SUPPORTED and focus(W=5) == NOT_SUPPORTED
    assert focus(img=None) == BAD_PARAM and focus(o=None) == BAD_PARAM and focus(o=p + 264) == BAD_PARAM
    assert focus(img=p + 1) == BAD_PARAM and focus(op=24) == BAD_PARAM and focus(op=36) == BAD_PARAM
    assert focus(H=0) == BAD_PARAM and focus(B=-1) == BAD_PARAM
    assert focus(B=0) == SUCCESS
    assert focus(H=65536, W=65536) == NOT_SUPPORTED

    def spp(x=p, xp=8, o=p + 256, op=24, B=1, H=4, W=4, C=8, k=(5, 9, 13)):
        return lib.bevops_spp_maxpool_nhwc(x, xp, o, op, B, H, W, C, *k, None)

    assert spp(C=12, xp=16, op=40) == NOT_SUPPORTED
    assert spp(k=(4, 9, 13)) == NOT_SUPPORTED and spp(k=(5, 9, 15)) == NOT_SUPPORTED
    assert spp(k=(0, 9, 13)) == BAD_PARAM
    assert spp(x=None) == BAD_PARAM and spp(o=None) == BAD_PARAM and spp(x=p + 8) == BAD_PARAM and spp(o=p + 260) == BAD_PARAM
    assert spp(xp=4) == BAD_PARAM and spp(op=16) == BAD_PARAM and spp(op=28) == BAD_PARAM   # out holds three slices
    assert spp(W=0) == BAD_PARAM and spp(C=0) == BAD_PARAM
    assert spp(B=0) == SUCCESS
    assert spp(H=65536, W=65536) == NOT_SUPPORTED

    def up(x=p, xp=8, o=p + 256, op=8, B=1, H=4, W=4, C=8):
        return lib.bevops_upsample_nearest2x_nhwc(x, xp, o, op, B, H, W, C, None)

    assert up(C=4, xp=8, op=8) == NOT_SUPPORTED
    assert up(x=None) == BAD_PARAM and up(o=None) == BAD_PARAM and up(x=p + 2) == BAD_PARAM and up(o=p + 264) == BAD_PARAM
    assert up(xp=0) == BAD_PARAM and up(op=4) == BAD_PARAM and up(H=-1) == BAD_PARAM
    assert up(B=0) == SUCCESS
    assert up(H=32768, W=32768) == NOT_SUPPORTED


# ------------------------------------------------------------------------------------------------ channel padding
def test_pad_channels_round_trip():
    from bevformer_tensorrt_amd.functions.yolox_ops import pad_channels, padded_width, unpad_channels
    assert [padded_width(c) for c in (12, 32, 80, 96, 160)] == [32, 32, 96, 96, 160]
    g = torch.Generator().manual_seed(0)
    w, b = torch.randn((80, 160, 3, 3), generator=g), torch.randn((80,), generator=g)
    wp, bp = pad_channels(w, b, groups_in=(80, 80))
    assert wp.shape == (96, 192, 3, 3) and bp.shape == (96,)
    assert torch.equal(wp[:80, :80], w[:, :80]) and torch.equal(wp[:80, 96:176], w[:, 80:])
    assert not wp[80:].any() and not wp[:, 80:96].any() and not wp[:, 176:].any() and not bp[80:].any()
    w2, b2 = unpad_channels(wp, bp, groups_in=(80, 80), groups_out=(80,))
    assert torch.equal(w2, w) and torch.equal(b2, b)
    wp, bp = pad_channels(w[:, :12], None)                      # the stem: Focus' 12 channels at 32
    assert wp.shape == (96, 32, 3, 3) and bp is None and torch.equal(wp[:80, :12], w[:, :12]) and not wp[:, 12:].any()
    same, _ = pad_channels(torch.ones((64, 32, 1, 1)))
    assert same.shape == (64, 32, 1, 1)
    with pytest.raises(ValueError):
        pad_channels(w, b, groups_in=(80, 40))
    with pytest.raises(ValueError):
        unpad_channels(w, b, groups_in=(80, 80), groups_out=(80,))


def _conv64(x, w, k):
    return X.int_conv(x, w, k, 1).reshape(x.shape[:3] + (w.shape[0],))


def _silu64(v):
    return v / (1.0 + np.exp(-v))


@pytest.mark.parametrize("layer", ["1x1", "3x3+identity", "final 1x1 behind the concatenation"])
def test_padded_96_channel_layer_is_the_80_channel_layer_exactly(layer):
    """The three layer kinds of a stage-1 CSP layer of YOLOX-x, 80 channels wide, against the same layer padded to 96
    (192 behind the concatenation of two padded tensors) channels: out = silu(conv(x) + bias) + identity in numpy
    float64 on the dyadic lattice, where every sum is exact in any order, so the real channels are EQUAL and the pad
    channels are exact zeros (silu(0 + 0) + 0 = 0)."""
    from bevformer_tensorrt_amd.functions.yolox_ops import pad_channels
    r = X._rng("pad 80 -> 96", layer)
    B, H, W, C = 2, 5, 6, 80
    k = 3 if layer.startswith("3x3") else 1
    groups = (C, C) if layer.startswith("final") else (C,)
    cin, cout = sum(groups), sum(groups)
    parts = [X.gen_f16_small(r, (B, H, W, g)).astype(np.float64) for g in groups]
    w, b = X.gen_f16_small(r, (cout, cin, k, k)), X.gen_bias(r, cout, X.F16)
    idt = X.gen_f16_small(r, (B, H, W, cout)).astype(np.float64) if "identity" in layer else None
    taps = lambda t: np.ascontiguousarray(np.transpose(t, (0, 2, 3, 1))).astype(np.float64)    # noqa: E731
    pad = lambda t, n: np.concatenate([t, np.zeros(t.shape[:3] + (n,))], axis=-1)               # noqa: E731

    def run(x, w, b, idt):
        s = _conv64(x, taps(w), k) + b.astype(np.float64)
        X.f32_exact(s, "sum + bias")
        y = _silu64(s)
        return y if idt is None else y + idt

    want = run(np.concatenate(parts, axis=-1), w, b, idt)
    wp, bp = pad_channels(torch.from_numpy(w), torch.from_numpy(b), groups_in=groups)
    assert wp.shape == ((cout + 31) // 32 * 32, 96 * len(groups), k, k)
    npad = wp.shape[0] - cout
    got = run(np.concatenate([pad(t, 16) for t in parts], axis=-1), wp.numpy(), bp.numpy(),
              None if idt is None else pad(idt, npad))
    assert np.array_equal(got[..., :cout], want) and want.any()
    assert npad == 0 or not got[..., cout:].any()
