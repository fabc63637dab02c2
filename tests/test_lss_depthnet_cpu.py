"""CPU-only: the pre-launch status contract of the three entries of csrc/lss_depthnet.hip in the order include/bevops.h
documents, and pack_camera_gate (functions/lss_depthnet.py): the layout of the block and the BatchNorm1d fold against a
float64 evaluation of BN-then-fc1."""
import ctypes
import types

import numpy as np
import pytest
import torch

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
    for name in ("bevops_lss_camera_gate", "bevops_lss_camera_gate_packed_size", "bevops_se_gate2_nhwc",
                 "bevops_global_avgpool_nhwc"):
        assert name in SIGNATURES
        assert lib.bevops_query(name.encode()) == ctypes.cast(getattr(lib, name), ctypes.c_void_p).value, name
    for name in ("lss_camera_gate", "se_gate2_nhwc", "global_avgpool_nhwc", "pack_camera_gate", "camera_gate_packed"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS


def test_camera_gate_status_codes(lib, p):
    p = p[0]

    def call(v=p, ip=27, pk=p + 1024, g=p + 4096, n=1, mid=32):
        return lib.bevops_lss_camera_gate(v, ip, pk, g, n, mid, None)

    assert call(v=None) == BAD_PARAM and call(pk=None) == BAD_PARAM and call(g=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(mid=0) == BAD_PARAM and call(ip=26) == BAD_PARAM
    assert call(v=p + 2) == BAD_PARAM and call(pk=p + 1025) == BAD_PARAM and call(g=p + 4098) == BAD_PARAM
    assert call(ip=26, mid=12) == BAD_PARAM                                  # before the domain checks
    assert call(mid=12) == NOT_SUPPORTED and call(mid=4) == NOT_SUPPORTED and call(mid=520) == NOT_SUPPORTED
    assert call(n=0, mid=12) == NOT_SUPPORTED
    assert call(n=0) == SUCCESS and call(n=0, mid=8) == SUCCESS and call(n=0, mid=512, ip=51) == SUCCESS
    assert lib.bevops_lss_camera_gate_packed_size(256) == 2 * 256 * (3 * 256 + 31) * 4
    assert lib.bevops_lss_camera_gate_packed_size(8) == 2 * 8 * 55 * 4
    assert lib.bevops_lss_camera_gate_packed_size(12) == 0 and lib.bevops_lss_camera_gate_packed_size(520) == 0


def test_se_gate2_status_codes(lib, p):
    p = p[0]

    def call(x=p, xp=8, g=p + 256, a=p + 512, ap=8, b=p + 768, bp=8, n=1, hw=4, c=8):
        return lib.bevops_se_gate2_nhwc(x, xp, g, a, ap, b, bp, n, hw, c, None)

    assert call(x=None) == BAD_PARAM and call(g=None) == BAD_PARAM and call(a=None) == BAD_PARAM and call(b=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(hw=0) == BAD_PARAM and call(c=0) == BAD_PARAM
    assert call(xp=0) == BAD_PARAM and call(ap=4) == BAD_PARAM and call(bp=12) == BAD_PARAM and call(xp=20, c=16) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(g=p + 260) == BAD_PARAM and call(a=p + 514) == BAD_PARAM
    assert call(b=p + 776) == BAD_PARAM
    assert call(c=12, xp=16, ap=16, bp=16) == NOT_SUPPORTED and call(c=4) == NOT_SUPPORTED
    assert call(c=12, xp=16, ap=16, bp=16, n=0) == NOT_SUPPORTED
    assert call(n=0) == SUCCESS and call(n=0, xp=72, ap=24, bp=16) == SUCCESS


def test_global_avgpool_status_codes(lib, p):
    p = p[0]

    def call(x=p, xp=8, o=p + 512, op=8, n=1, hw=4, c=8):
        return lib.bevops_global_avgpool_nhwc(x, xp, o, op, n, hw, c, None)

    assert call(x=None) == BAD_PARAM and call(o=None) == BAD_PARAM
    assert call(n=-1) == BAD_PARAM and call(hw=0) == BAD_PARAM and call(c=0) == BAD_PARAM
    assert call(xp=4) == BAD_PARAM and call(xp=12) == BAD_PARAM and call(op=4) == BAD_PARAM
    assert call(x=p + 8) == BAD_PARAM and call(o=p + 513) == BAD_PARAM
    assert call(c=12, xp=16, op=12) == NOT_SUPPORTED and call(c=12, xp=16, op=12, n=0) == NOT_SUPPORTED
    assert call(n=0) == SUCCESS and call(n=0, op=9, o=p + 514) == SUCCESS


# ------------------------------------------------------------------------------------------------ pack_camera_gate
def _modules(mid, seed):
    g = torch.Generator().manual_seed(seed)

    def lin(o, i):
        m = torch.nn.Linear(i, o)
        m.weight.data = torch.randn((o, i), generator=g) / i ** 0.5
        m.bias.data = torch.randn((o,), generator=g)
        return m

    def conv(c):
        m = torch.nn.Conv2d(c, c, 1)
        m.weight.data = torch.randn((c, c, 1, 1), generator=g) / c ** 0.5
        m.bias.data = torch.randn((c,), generator=g)
        return m

    bn = torch.nn.BatchNorm1d(27)
    bn.running_mean.data = torch.randn((27,), generator=g) * 100.0
    bn.running_var.data = torch.rand((27,), generator=g) * 1e4 + 0.1
    bn.weight.data = torch.randn((27,), generator=g)
    bn.bias.data = torch.randn((27,), generator=g)
    bn.eval()
    branches = [(types.SimpleNamespace(fc1=lin(mid, 27), fc2=lin(mid, mid)),
                 types.SimpleNamespace(conv_reduce=conv(mid), conv_expand=conv(mid))) for _ in range(2)]
    return bn, branches


@pytest.mark.parametrize("mid", [8, 32, 96])
def test_pack_camera_gate_layout_and_bn_fold(mid):
    from bevformer_tensorrt_amd.functions.lss_depthnet import pack_camera_gate
    bn, ((dm, ds), (cm, cs)) = _modules(mid, mid)
    packed = pack_camera_gate(bn, dm, ds, cm, cs)
    words = mid * (3 * mid + 31)
    assert packed.dtype == torch.float32 and packed.is_contiguous() and packed.numel() == 2 * words
    r = np.random.default_rng(mid)
    v = np.concatenate([r.standard_normal((5, 27)) * 100.0, [[1266.4] * 27], [[0.0] * 27]]).astype(np.float32).astype(np.float64)
    s = bn.weight.detach().double().numpy() / np.sqrt(bn.running_var.double().numpy() + bn.eps)
    normed = (v - bn.running_mean.double().numpy()) * s + bn.bias.detach().double().numpy()          # BN, then fc1: float64
    for br, (mlp, se) in enumerate(((dm, ds), (cm, cs))):
        q = packed[br * words:(br + 1) * words].double().numpy()
        w1, b1 = q[:27 * mid].reshape(27, mid), q[27 * mid:28 * mid]
        at = 28 * mid
        want = normed @ mlp.fc1.weight.double().detach().numpy().T + mlp.fc1.bias.double().detach().numpy()
        got = v @ w1 + b1
        # the packed operands are the float64 fold rounded ONCE to fp32: 2^-24 relative on each of the 28 terms
        bound = 2.0 ** -24 * (np.abs(v) @ np.abs(w1) + np.abs(b1)) + 1e-12
        assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))
        for lay_w, lay_b in ((mlp.fc2.weight, mlp.fc2.bias), (se.conv_reduce.weight, se.conv_reduce.bias),
                             (se.conv_expand.weight, se.conv_expand.bias)):
            wk = torch.from_numpy(q[at:at + mid * mid].reshape(mid, mid)).float()
            assert torch.equal(wk.t(), lay_w.detach().reshape(mid, mid))                    # k-major: [input][output]
            assert torch.equal(torch.from_numpy(q[at + mid * mid:at + mid * mid + mid]).float(), lay_b.detach())
            at += mid * mid + mid
        assert at == words


def test_camera_gate_packed_is_cached_per_stamp_and_rebuilt():
    from bevformer_tensorrt_amd.functions.lss_depthnet import camera_gate_packed
    bn, ((dm, ds), (cm, cs)) = _modules(8, 1)
    assert camera_gate_packed(bn, dm, ds, cm, cs, build=False) is None
    a = camera_gate_packed(bn, dm, ds, cm, cs)
    assert camera_gate_packed(bn, dm, ds, cm, cs) is a
    with torch.no_grad():
        cs.conv_expand.bias.add_(1.0)                                       # the LAST tensor of the block changes
    assert camera_gate_packed(bn, dm, ds, cm, cs, build=False) is None
    b = camera_gate_packed(bn, dm, ds, cm, cs)
    assert b is not a and torch.equal(b[-8:], a[-8:] + 1.0) and torch.equal(b[:-8], a[:-8])


def test_wrappers_refuse_what_is_outside_their_domain_without_a_device():
    import bevformer_tensorrt_amd as bev
    with pytest.raises(ValueError):
        bev.lss_camera_gate(torch.zeros((2, 27)), torch.zeros(10), 32)
    with pytest.raises(ValueError):
        bev.se_gate2_nhwc(torch.zeros((1, 8, 2, 2), dtype=torch.float16), torch.zeros((2, 1, 8)))
    with pytest.raises(ValueError):
        bev.global_avgpool_nhwc(torch.zeros((1, 8, 2, 2), dtype=torch.float16))
