"""CPU-only: the operator API's last three reference functions (qkv, qkv2, inverse) -- the registry, the plugin names of
bevops_query, the argument checks that return before any device call, and the golden vectors the reference's own
Python made (tests/golden/make_qkv_inverse_golden.py) against an fp64 evaluation of their inputs."""
import ctypes

import numpy as np
import pytest

from conftest import golden

# det2trt/models/functions/__init__.py:17-35
REFERENCE_REGISTRY = ("grid_sampler", "grid_sampler2", "multi_scale_deformable_attn", "multi_scale_deformable_attn2",
                      "modulated_deformable_conv2d", "modulated_deformable_conv2d2", "rotate", "rotate2", "inverse",
                      "bev_pool_v2", "bev_pool_v2_2", "qkv", "qkv2")
F32, F16, I8 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_registry_holds_every_reference_function():
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    for name in REFERENCE_REGISTRY:
        assert name in bev.TRT_FUNCTIONS, name
        assert bev.TRT_FUNCTIONS.get(name) is getattr(bev, name), name
        assert name in fn.__all__, name


def test_query_resolves_attention_and_inverse_plugins(lib):
    def addr(sym):
        return ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value
    assert lib.bevops_query(b"QKVTRT") == addr("bevops_qkv_forward")
    assert lib.bevops_query(b"QKVTRT2") == addr("bevops_qkv_forward")
    assert lib.bevops_query(b"InverseTRT") == addr("bevops_inverse_forward")
    assert lib.bevops_query(b"bevops_qkv_workspace_size") == addr("bevops_qkv_workspace_size")


def test_status_codes_without_gpu(lib):
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned host address: never dereferenced

    def qkv(dt, q=p, k=p, v=p, o=p, B=2, Lq=33, Lkv=47, E=32, ws=None, nws=0):
        return lib.bevops_qkv_forward(dt, q, k, v, o, B, Lq, Lkv, E, 1.0, 1.0, 1.0, 1.0, ws, nws, None)

    assert qkv(F32, q=None) == 2 and qkv(F16, v=None) == 2 and qkv(F32, o=None) == 2
    assert qkv(F32, B=0) == 2 and qkv(F32, Lq=0) == 2 and qkv(F32, Lkv=-1) == 2
    assert qkv(F32, E=24) == 3 and qkv(F16, E=256) == 3 and qkv(F32, E=8) == 3
    assert qkv(I8) == 3
    assert qkv(F32, k=p + 4) == 2 and qkv(F16, o=p + 8) == 2
    # a long-key, small-batch call splits its keys across blocks: it needs the workspace it asks for
    need = lib.bevops_qkv_workspace_size(F16, 2, 64, 40000, 32)
    assert need > 0 and qkv(F16, B=2, Lq=64, Lkv=40000, E=32) == 2
    assert qkv(F16, B=2, Lq=64, Lkv=40000, E=32, ws=p, nws=need - 1) == 2
    assert lib.bevops_qkv_workspace_size(F16, 8, 900, 900, 32) == 0       # enough query tiles: no split
    assert lib.bevops_qkv_workspace_size(I8, 2, 64, 40000, 32) == 0
    assert lib.bevops_qkv_workspace_size(F32, 2, 64, 40000, 24) == 0

    inv = lib.bevops_inverse_forward
    assert inv(F32, None, p, 4, 3, None) == 2 and inv(F32, p, None, 4, 3, None) == 2
    assert inv(F32, p, p, 0, 3, None) == 2 and inv(F32, p, p, 4, 0, None) == 2
    assert inv(F32, p, p, 4, 33, None) == 3
    assert inv(F16, p, p, 4, 3, None) == 3 and inv(I8, p, p, 4, 3, None) == 3
    assert inv(F32, p + 4, p, 4, 3, None) == 2


def _attention64(q, k, v):
    s = np.einsum("bie,bje->bij", q, k) / np.sqrt(q.shape[-1])
    s = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bij,bje->bie", s / s.sum(-1, keepdims=True), v)


def test_fixtures_agree_with_fp64():
    g = golden("qkv")
    for i, (B, Lq, Lkv, E) in enumerate(g["shapes"]):
        q, k, v = (g[f"{n}{i}"].astype(np.float64) for n in "qkv")
        assert q.shape == (B, Lq, E) and k.shape == v.shape == (B, Lkv, E)
        err = np.abs(g[f"out{i}"] - _attention64(q, k, v))
        assert err.max() <= 1e-5 and err.mean() <= 1e-6, (i, err.max(), err.mean())
    g = golden("inverse")
    for name in [k[2:] for k in g if k.startswith("a_")]:
        a, x = g["a_" + name].astype(np.float64), g["x_" + name]
        want = np.linalg.inv(a)
        assert np.abs(x - want).max() <= 1e-4 * max(1.0, np.abs(want).max()), name
