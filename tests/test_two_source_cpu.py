"""CPU-only: the host side of the two-source GEMM (bevops_gemm2_f16) and of the route that uses it
(bevformer.Bottleneck.forward_nhwc): the entry's rejections before any device call, the stacked weight / summed bias of
a first block and their cache, and the route's predicate."""
import ctypes

import pytest
import torch
from torch import nn


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_entry_rejects_without_a_device(lib):
    BAD, UNSUP = 2, 3
    ll = ctypes.c_longlong
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(a1=p, a2=p, w=p, bias=None, out=p, m=70, n=256, k1=64, k2=64, B=1, H=1, W=70, s=1):
        return lib.bevops_gemm2_f16(a1, a2, w, bias, out, ll(m), n, k1, k2, B, H, W, s, 1, None)
    for kw in (dict(a1=None), dict(a2=None), dict(w=None), dict(out=None), dict(m=0), dict(n=0), dict(k1=0), dict(k2=-64),
               dict(B=0), dict(H=0), dict(W=0), dict(s=0)):
        assert call(**kw) == BAD, kw
    for kw in (dict(k1=96), dict(k2=32), dict(k1=100, k2=28), dict(n=100), dict(s=3)):
        assert call(**kw) == UNSUP, kw
    # geometry: M must be B * Ho * Wo of the second source
    for kw in (dict(W=71), dict(B=2), dict(m=69), dict(H=2, s=2), dict(H=5, W=7, s=2, B=2, m=2 * 3 * 4 + 1)):
        assert call(**kw) == BAD, kw
    for kw in (dict(a1=p + 8), dict(a2=p + 2), dict(w=p + 4), dict(out=p + 8), dict(bias=p + 2)):
        assert call(**kw) == BAD, kw
    # byte ranges beyond the 32-bit buffer offsets: rows of source 1, pixels of source 2, the weight
    big = 0x7fffffff
    assert call(m=big, W=big) == UNSUP
    assert call(m=1 << 24, W=1 << 25, s=2, k2=128) == UNSUP
    assert call(n=1 << 24, k1=128, k2=128) == UNSUP


def _first_block(cin=64, planes=64, stride=1):
    from bevformer_tensorrt_amd import bevformer as B
    torch.manual_seed(3)
    return B, B.Bottleneck(cin, planes, stride, False, None, True).half()


def test_stacked_weight_and_bias_follow_the_parameters():
    B, blk = _first_block(256, 128, 2)
    w, b = B._stacked_pair(blk)
    assert w.shape == (512, 128 + 256) and w.dtype == torch.float16 and w.is_contiguous() and b.shape == (512,)
    assert torch.equal(w[:, :128], blk.conv3.weight.detach().view(512, 128))
    assert torch.equal(w[:, 128:], blk.downsample.weight.detach().view(512, 256))
    assert torch.equal(b, (blk.conv3.bias.detach().float() + blk.downsample.bias.detach().float()).half())
    w2, b2 = B._stacked_pair(blk)
    assert w2 is w and b2 is b                               # cached
    with torch.no_grad():
        blk.downsample.weight.mul_(2)                        # in-place update: re-stacked
    w3, b3 = B._stacked_pair(blk)
    assert w3 is not w and torch.equal(w3[:, 128:], blk.downsample.weight.detach().view(512, 256)) and torch.equal(w3[:, :128], w[:, :128])
    with torch.no_grad():
        blk.conv3.bias.add_(1)
    assert torch.equal(B._stacked_pair(blk)[1], (blk.conv3.bias.detach().float() + blk.downsample.bias.detach().float()).half())
    blk.conv3.weight = nn.Parameter(torch.zeros_like(blk.conv3.weight))      # new storage: re-stacked
    assert float(B._stacked_pair(blk)[0][:, :128].abs().max()) == 0.0


class _Rows:
    """What the predicate asks of the block's input: an fp16 channels-last 4-d tensor on the GPU."""
    dtype, is_cuda = torch.float16, True

    def __init__(self, dtype=torch.float16, cuda=True, nhwc=True):
        self.dtype, self.is_cuda, self.nhwc = dtype, cuda, nhwc

    def dim(self):
        return 4

    def is_contiguous(self, memory_format=None):
        return self.nhwc if memory_format is torch.channels_last else True


class _Ops:
    gemm2 = staticmethod(lambda *a, **k: None)


def test_route_predicate(monkeypatch):
    B, blk = _first_block()
    ok = lambda b=blk, x=None, ops=_Ops: B._two_source_ok(ops, b, x or _Rows())      # noqa: E731
    assert B._FUSED_DOWNSAMPLE["enabled"] and ok()
    for cin, planes, stride in ((256, 128, 2), (512, 256, 2), (1024, 512, 2)):      # a shape class decides, nothing else
        assert ok(_first_block(cin, planes, stride)[1]) == ((planes, cin, stride) in B._FUSED_DOWNSAMPLE_SHAPES)
    # the switches
    for flag in (B._FUSED_DOWNSAMPLE, B._R3, B._FUSED_LINEAR):
        monkeypatch.setitem(flag, "enabled", False)
        assert not ok()
        monkeypatch.setitem(flag, "enabled", True)
    assert ok()
    # no downsample, an operator set without the entry, calibration, quantised layers, other tensors
    later = B.Bottleneck(256, 64, 1, False, None, False).half()
    assert not ok(later)
    assert not ok(ops=object())
    cal = _first_block()[1]
    cal.chain_cal = object()
    assert not ok(cal)
    q = _first_block()[1]
    q.conv3.lin = object()                                   # quantization.Conv2dQ carries its LinearQ as .lin
    assert not ok(q)

    class ConvQ(nn.Conv2d):
        pass
    q = _first_block()[1]
    q.downsample = ConvQ(64, 256, 1).half()
    assert not ok(q)
    assert not ok(_first_block()[1].float())                 # fp32 parameters
    assert not ok(x=_Rows(dtype=torch.float32)) and not ok(x=_Rows(cuda=False)) and not ok(x=_Rows(nhwc=False))
    odd = _first_block(64, 32, 1)[1]                          # K1 = 32: no shape class
    assert not ok(odd)


def test_environment_switch_is_read_at_import():
    import os
    import subprocess
    import sys
    code = "from bevformer_tensorrt_amd import bevformer as B; print(B._FUSED_DOWNSAMPLE['enabled'])"
    from conftest import ROOT
    env = dict(os.environ, BEVOPS_FUSED_DOWNSAMPLE="0", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "False"
