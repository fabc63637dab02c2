"""tsgemm_s8_kernel (csrc/tsgemm.hip, the persistent int8 GEMM) bit for bit against the float64 reference of
tests/util_exact_dense.py and against the tiled int8 GEMM on the same operands: every k-step count (one step, two
stages, the bi % nk rotation, the stage ring wrapping), every kloop<G> instantiation (G = 1 .. 5 row units at a time,
reached through row counts computed from the device's CU count), a second pass of a block's unit loop (the epilogue
staging overlays stage buffers 0 and 1 and the next tile's DMA starts right behind it), ragged last units, both identity
and output types.  With power-of-two scales the ONE-step allowance of test_int8_chain_gpu.py is not needed: equality
is exact."""
import numpy as np
import pytest
import torch

import util_exact_dense as X

pytestmark = pytest.mark.gpu


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_both(c, o):
    """(tsgemm_s8, tiled int8 GEMM) on the case's operands through linear_int8_chain."""
    from bevformer_tensorrt_amd.functions import int8_chain as C
    assert c["N"] % 256 == 0 and c["K"] % 128 == 0            # inside the persistent kernel's domain: it IS what runs
    sw = o["s_w"] if np.isscalar(o["s_w"]) else _dev(o["s_w"])
    args = (_dev(o["a"]), o["s_a"], _dev(o["w"]), sw, _dev(o["bias"]), _dev(o["res"]), o["s_res"], c["relu"],
            torch.int8 if c["out"] == "int8" else torch.float16, o["s_out"])
    prev = C._TS_S8["enabled"]
    C._TS_S8["enabled"] = True
    try:
        got = C.linear_int8_chain(*args)
        C._TS_S8["enabled"] = False
        tiled = C.linear_int8_chain(*args)
        torch.cuda.synchronize()
    finally:
        C._TS_S8["enabled"] = prev
    return got.cpu().numpy(), tiled.cpu().numpy()


def _check(c):
    o = X.make_ops(c)
    want = X.reference(c, o)
    got, tiled = _run_both(c, o)
    for name, y in (("tsgemm_s8", got), ("tiled int8 GEMM", tiled)):
        assert y.dtype == want.dtype and y.shape == want.shape
        if not np.array_equal(y, want):
            bad = np.argwhere(y != want)
            m, n = bad[0]
            raise AssertionError(f"{c['id']} {name}: {len(bad)} of {want.size} outputs differ, first at [{m}, {n}]: got "
                                 f"{y[m, n]!r}, want {want[m, n]!r}; rows {sorted(set(bad[:, 0]))[:8]} "
                                 f"(units {sorted(set(bad[:, 0] // 32))[:8]})")
    assert np.array_equal(got, tiled)


@pytest.mark.parametrize("c", X.ts_small_cases(), ids=lambda c: c["id"])
def test_small_row_counts(c):
    _check(c)


@pytest.mark.parametrize("j", range(X.TS_LARGE))
def test_every_unit_count_and_a_second_pass(j):
    """Row counts computed from the CU count.  The partition the kernel will use is asserted BEFORE the launch: on a
    device with another CU count the test fails here instead of silently losing a kloop<G> instantiation."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = X.ts_large_case(j, cus)
    assert c["M"] % 32 != 0
    passes = X.ts_block_passes(c["M"], cus)
    assert passes == X.ts_expected_partition(cus)[j], (cus, c["M"], sorted(passes))
    if j == 0:                                                 # all four together: every G alone, and a second pass
        seen = set().union(*(X.ts_block_passes(m, cus) for m in X.ts_large_m(cus)))
        assert {(1,), (2,), (3,), (4,), (5,)} <= seen and any(len(p) == 2 for p in seen)
    _check(c)


@pytest.mark.parametrize("c", [c for c in X.saturated_cases() if c["N"] % 256 == 0], ids=lambda c: c["id"])
def test_saturated_accumulators(c):
    """K = 2 048, |acc| up to 33 032 192 > 2^24: sixteen k-steps of int32 sums, (float)acc rounded to nearest even."""
    _check(c)
