"""CPU-only: where the merged projection launches of bevformer.py must NOT run -- a model that holds a LinearQ layer,
an operator set without the grouped / destination-table entries (the reference operators), tensors that are not fp16 on
the GPU, the switch off, the own-kernel dispatch off, problems of the few-row kernel -- the per-layer path runs and no
new entry is called; and the new C entries reject their domain borders before touching a device."""
import ctypes
import types

import pytest
import torch


class _FakeRows:
    """What the guards look at of an fp16 GPU tensor, without a GPU."""
    dtype, is_cuda, device = torch.float16, True, "cuda:0"

    def __init__(self, m, k=256):
        self.shape = (m, k)

    def numel(self):
        return self.shape[0] * self.shape[1]


def _boom(*a, **k):
    raise AssertionError("a merged entry was called")


def _ops():
    return types.SimpleNamespace(tsgemm_grouped=_boom, tile_gemm_dst=_boom, small_gemm_dst=_boom, dense_auto=_boom, linear_bias_act=_boom)


@pytest.fixture()
def own_kernels():
    from bevformer_tensorrt_amd.functions.linear import OWN_KERNELS
    was, OWN_KERNELS["enabled"] = OWN_KERNELS["enabled"], True
    yield
    OWN_KERNELS["enabled"] = was


def test_guard_accepts_plain_fp16_layers_and_nothing_else(own_kernels):
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.quantization import LinearQ
    plain = [torch.nn.Linear(256, 256).half() for _ in range(2)]
    x = _FakeRows(40000)
    assert B._merge_ok(_ops(), x, plain, False)
    assert not B._merge_ok(_ops(), x, [plain[0], LinearQ(256, 256)], False)              # the INT8 engine's layer
    assert not B._merge_ok(_ops(), x, [plain[0], torch.nn.Linear(256, 256)], False)      # fp32 parameters
    assert not B._merge_ok(_ops(), x, [torch.nn.Linear(256, 256, bias=False).half()], False)
    assert not B._merge_ok(types.SimpleNamespace(tsgemm_grouped=_boom), x, plain, False)    # no dispatch: not the HIP set
    assert not B._merge_ok(_ops(), _FakeRows(300), plain, False)                         # the few-row kernel's problem
    assert not B._merge_ok(_ops(), _FakeRows(2500), [torch.nn.Linear(256, 192).half()], True)
    for flag in (B._MERGED_PROJ, B._R3, B._FUSED_LINEAR):
        flag["enabled"] = False
        try:
            assert not B._merge_ok(_ops(), x, plain, False)
        finally:
            flag["enabled"] = True


def test_guard_needs_the_own_kernel_dispatch():
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.functions.linear import OWN_KERNELS
    assert not OWN_KERNELS["enabled"]
    assert not B._merge_ok(_ops(), _FakeRows(40000), [torch.nn.Linear(256, 256).half()], False)


def test_cpu_and_quantised_layers_take_the_per_layer_path(own_kernels):
    """The helpers return None -- the caller's per-layer path -- and never reach an entry."""
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.quantization import LinearQ
    owner = torch.nn.Module()
    plain = [torch.nn.Linear(256, 256).half() for _ in range(2)]
    for x in (torch.zeros(4096, 256), torch.zeros(4096, 256, dtype=torch.float16)):       # CPU tensors
        assert B._merged_value_proj(_ops(), owner, "_v", plain, x) is None
        assert B._merged_pair(_ops(), owner, "_p", plain[0], plain[1], x) is None
    x = _FakeRows(40000)
    assert B._merged_value_proj(_ops(), owner, "_v", [plain[0], LinearQ(256, 256)], x) is None
    assert B._merged_pair(_ops(), owner, "_p", LinearQ(256, 512), plain[1], x) is None
    assert B._merged_value_proj(types.SimpleNamespace(dense_auto=_boom), owner, "_v", plain, x) is None   # no grouped entry
    tsa = B.TemporalSelfAttention(_ops())
    tsa.sampling_offsets = LinearQ(512, 128)
    assert B._merged_prev_terms(_ops(), owner, "_t", [tsa], x, x, x) is None
    assert not hasattr(owner, "_v") and not hasattr(owner, "_p") and not hasattr(owner, "_t")


def test_reference_operator_set_has_no_merged_entries():
    from oracle.ref_ops import TorchRefOps
    assert not any(hasattr(TorchRefOps, n) for n in ("tsgemm_grouped", "tile_gemm_dst", "small_gemm_dst"))


def test_tiny_encoder_layer_on_the_reference_operators_runs_per_layer(monkeypatch):
    """A frame-level call on the CPU with the reference operators: TemporalSelfAttention evaluates its own projections,
    the HIP entries are never looked up."""
    import bevformer_tensorrt_amd.functions as hip_ops
    from bevformer_tensorrt_amd import bevformer as B
    from oracle.ref_ops import TorchRefOps
    monkeypatch.setattr(hip_ops, "tsgemm_grouped", _boom)
    monkeypatch.setattr(hip_ops, "tile_gemm_dst", _boom)
    torch.manual_seed(0)
    ops = TorchRefOps()
    tsa = B.TemporalSelfAttention(ops)
    nq = 64
    q, pos = torch.randn(1, nq, 256), torch.randn(1, nq, 256)
    prev = torch.randn(2, nq, 256)
    assert B._merged_value_proj(ops, tsa, "_v", [tsa.value_proj], prev[0]) is None
    assert B._merged_prev_terms(ops, tsa, "_t", [tsa], q, prev[0], pos) is None
    out = tsa(q, prev, pos, torch.rand(2, nq, 1, 2), torch.tensor([[8, 8]]))
    assert out.shape == (1, nq, 256) and bool(torch.isfinite(out).all())


def test_new_entries_reject_bad_params_without_gpu():
    from bevformer_tensorrt_amd.utils import lib as L
    from bevformer_tensorrt_amd.functions.linear import _GemmDst
    lib = L.load_library()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ll = ctypes.c_longlong
    assert lib.bevops_tsgemm_f16_grouped(p, p, None, p, ll(64 * 256), ll(64), 2, 320, None) == L.NOT_SUPPORTED    # K > 256
    assert lib.bevops_tsgemm_f16_grouped(p, p, None, p, ll(64 * 256), ll(64), 2, 96, None) == L.NOT_SUPPORTED     # K % 64
    assert lib.bevops_tsgemm_f16_grouped(p, p, None, p, ll(63 * 256), ll(64), 2, 256, None) == L.BAD_PARAM       # overlap
    assert lib.bevops_tsgemm_f16_grouped(p, p, None, p + 2, ll(64 * 256), ll(64), 2, 256, None) == L.BAD_PARAM
    assert lib.bevops_tsgemm_f16_grouped(None, p, None, p, ll(64 * 256), ll(64), 2, 256, None) == L.BAD_PARAM
    assert lib.bevops_tsgemm_f16_grouped(p, p, None, p, ll(64 * 256), ll(64), 0, 256, None) == L.BAD_PARAM

    def dst(ranges, n=512, k=256):
        tab = (_GemmDst * len(ranges))()
        for i, (c0, c1, off, pitch) in enumerate(ranges):
            tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = c0, c1, p + off, pitch
        return lib.bevops_tile_gemm_f16_dst(p, p, None, ctypes.addressof(tab), len(ranges), ll(64), n, k, 0, None)

    assert dst([(0, 96, 0, 256)]) == L.BAD_PARAM                           # bound off the 64-column grid
    assert dst([(0, 256, 0, 256), (192, 512, 0, 320)]) == L.BAD_PARAM      # overlapping ranges
    assert dst([(0, 256, 0, 192)]) == L.BAD_PARAM                          # pitch below the width
    assert dst([(0, 256, 2, 256)]) == L.BAD_PARAM                          # unaligned destination
    assert dst([(0, 64, 0, 64)], n=64) == L.NOT_SUPPORTED
    assert dst([(0, 256, 0, 256)], k=100) == L.NOT_SUPPORTED
    assert lib.bevops_tile_gemm_f16_dst(p, p, None, None, 1, ll(64), 512, 256, 0, None) == L.BAD_PARAM


def test_original_tsgemm_kernel_switches_the_tiled_merges_off(own_kernels):
    """Under bevops_tsgemm_set_variant(1) a per-layer GEMM on tsgemm rotates its k start by block index: tile_gemm_dst has
    other bits, so the merge of such a layer is refused; layers on tile_gemm alone still merge, the grouped entry follows
    the variant itself."""
    from bevformer_tensorrt_amd import bevformer as B
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    assert B._per_layer_kernels("cuda:0", 40000, [512, 256], 256, True, False) == "tiled"     # tile_gemm + tsgemm
    assert B._per_layer_kernels("cuda:0", 900, [64, 32], 256, False, True) == "small"
    assert B._per_layer_kernels("cuda:0", 3000, [64, 512], 256, True, False) is None          # few-row + tiled: no common kernel
    prev = handle.bevops_tsgemm_set_variant(1)
    try:
        assert B._per_layer_kernels("cuda:0", 40000, [512, 256], 256, True, False) is None
        assert B._per_layer_kernels("cuda:0", 40000, [192] * 6, 256, False, True) == "tiled"  # tile_gemm only
        assert not B._merge_ok(_ops(), _FakeRows(40000), [torch.nn.Linear(256, 256).half()], False)
    finally:
        handle.bevops_tsgemm_set_variant(prev)
    assert B._merge_ok(_ops(), _FakeRows(40000), [torch.nn.Linear(256, 256).half()], False)
