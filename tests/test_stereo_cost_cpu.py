"""CPU-only: the BEVStereo cost volume's torch statements (bevformer_tensorrt_amd/functions/stereo.py) against the
fixture tests/golden/bevstereo.npz, which tests/golden/make_bevstereo_golden.py records by EXECUTING the reference's
gen_grid and calculate_cost_volumn (lifted by AST) in fp32 -- bit for bit, in a child interpreter with the CPU kernel
choice pinned as the recording had it; every status of the two C entries in the documented order (they return before
any device call); the float64 statement of the GPU tests against the torch statement; and the GPU tests' premises."""
import ctypes

import pytest
import torch

import util_stereo as U
from conftest import golden, run_pinned


def _fixture():
    G = golden("bevstereo")
    return G, (lambda k: torch.from_numpy(G[k]))


def grid_and_cost_volume_bit_for_bit():
    """(runs under conftest.PINNED_CPU_ENV) the statements reproduce the reference's ops one for one."""
    from bevformer_tensorrt_amd.functions import (stereo_calibration, stereo_cost_volume, stereo_frustum_tables,
                                                  stereo_grid)
    G, t = _fixture()
    consts = stereo_calibration(t("k2s_sensor"), t("intrins"), t("post_rots"), t("post_trans"))
    assert consts.shape == (2, 40) and consts.dtype == torch.float32 and not consts.is_cuda
    tables = stereo_frustum_tables(t("cv_frustum"))
    grid = stereo_grid(consts, tables)
    assert grid.shape == (2, 6, 8, 12, 2)
    assert torch.equal(grid.view(torch.int32), t("grid").view(torch.int32))
    for tag, bias in (("b5", 5.0), ("b0", 0.0)):
        for g in (grid, consts):                       # the explicit grid, and the constants with the tables
            cv = stereo_cost_volume(t("prev"), t("curr"), g, 6, bias, frustum_tables=tables)
            assert cv.shape == (2, 6, 8, 12)
            assert torch.equal(cv.view(torch.int32), t("cv_" + tag).view(torch.int32)), tag
    assert not torch.equal(t("cv_b5"), t("cv_b0"))
    first = stereo_cost_volume(None, t("curr"), grid, 6, 5.0)
    assert first.shape == (2, 6, 8, 12) and not bool(first.any())


def test_statements_equal_the_reference_bit_for_bit():
    run_pinned("test_stereo_cost_cpu", "grid_and_cost_volume_bit_for_bit")


def test_fixture_shows_something():
    G, t = _fixture()
    grid, cv = t("grid"), t("cv_b5")
    inside = (grid.abs() <= 1).all(-1)
    assert inside[0].float().mean() > 0.5 and 0.05 < inside[1].float().mean() < 0.95
    assert bool((grid[1] == -2).all(-1).any()) and not bool((grid[0] == -2).any())        # behind the plane: camera 1 only
    assert t("near_plane").float().mean().item() <= 0.01
    assert cv.max(1).values.mean().item() < 0.9                                           # not one-hot
    assert torch.allclose(cv.sum(1), torch.ones(2, 8, 12), atol=1e-5)
    for k in ("prev", "curr"):
        z = (t(k) == 0).float().mean().item()
        assert 0.3 < z < 0.7 and bool((t(k) >= 0).all()), (k, z)
    assert float(G["grid_err"]) < 1e-3 and float(G["cv_err_b5"]) < 1e-5 and float(G["cv_err_b0"]) < 1e-5


def test_float64_statement_of_the_gpu_tests_within_the_references_own_error():
    """tests/util_stereo.py's statement against the fixture: within the fp32 error the fixture script measured for the
    reference itself against float64 on the same fp32 grid (twice it: two fp32 evaluations may differ by both)."""
    G, t = _fixture()
    for tag, bias in (("b5", 5.0), ("b0", 0.0)):
        ref = U.ref_cost_volume(t("prev"), t("curr"), t("grid"), bias)
        err = (ref["prob"] - t("cv_" + tag).double()).abs().max().item()
        print(f"bias {bias}: float64 statement vs the reference's fp32 {err:.3e} (its recorded error {float(G['cv_err_' + tag]):.3e})")
        assert err <= 2 * float(G["cv_err_" + tag])
    inside = (t("grid").abs() <= 1).all(-1)
    gate = U.ref_cost_volume(t("prev"), t("curr"), t("grid"), 5.0)["gate"]
    frac = (gate & inside).float().sum().item() / inside.float().sum().item()
    assert 0.05 < frac < 0.95                           # gate == 0 fires INSIDE the image too


def test_premises_of_the_gpu_tests():
    import test_stereo_cost_gpu as T
    assert T.SHAPES[:4] == [(1, 1, 1, 8, 1), (2, 5, 7, 8, 6), (1, 9, 33, 264, 59), (2, 4, 70, 256, 128)]
    n, H, W, C, D = T.SHAPES[4]
    assert (n * H * W) % 4 == 0 and W == 4                      # rows of exactly one 4-pixel tile
    assert any(s[2] % 4 for s in T.SHAPES) and any(s[3] > 256 and s[3] % 256 for s in T.SHAPES)
    for shape in (T.SHAPES[1], T.SHAPES[2]):
        prev, curr, grid, ref = T.gaussian_case(shape)
        inside = (grid.abs() <= 1).all(-1)
        frac = (ref["gate"] & inside).float().sum().item() / inside.float().sum().item()
        print(f"{shape}: gate == 0 at {100 * frac:.1f} % of the in-image positions, "
              f"{100 * inside.float().mean().item():.1f} % of the positions in the image")
        assert 0.05 < frac < 0.95 and 0.3 < inside.float().mean().item() < 0.95
        assert bool((prev >= 0).all()) and 0.3 < (prev == 0).float().mean().item() < 0.7
        assert ref["prob"].max(1).values.mean().item() < 0.9
        # the derived bound is far below the quantity it guards: a wrong corner or weight cannot hide in it
        assert U.general_bound(ref["prob"], ref["mag"]).max().item() < 2e-3
    prev, curr, grid, want = T.lattice_case(T.SHAPES[1])
    assert 0.05 < want[5.0]["gate"].float().mean().item() < 0.95
    # the lattice generator hits most of its targets (near g = -1 the fp32 grid is too coarse for some: those become
    # pixel 0, on the lattice too); the GPU test asserts for every shape that all positions are on the lattice
    tx = torch.arange(-4, 4 * 70 + 1).float() / 4
    ix, _ = U.source_pos(U.lattice_grid(tx, torch.zeros_like(tx), 4, 70), 4, 70)
    assert ((ix == tx) | (ix == 0)).all() and (ix == tx).float().mean().item() > 0.6
    assert len(set((ix[ix == tx] % 1).tolist())) == 4 and bool((ix > 69).any())


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_every_status_in_the_documented_order(lib):
    """include/bevops.h: BAD_PARAM (2) checks in bevops_conv_slice_f16's order -- NULL / sizes, pitches below the
    channel count, pitches that are no multiple of 8, alignment -- then NOT_SUPPORTED (3), then n == 0.  No call here
    reaches a launch."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    f = ctypes.c_float

    def cost(**kw):
        a = dict(prev=p, pp=8, curr=p, cp=8, grid=p, consts=None, xs=None, ys=None, ds=None, out=p, op=8, n=0, H=2, W=3,
                 C=8, D=6, Dpad=8, bias=5.0)
        a.update(kw)
        return lib.bevops_stereo_cost_volume_f16(a["prev"], a["pp"], a["curr"], a["cp"], a["grid"], a["consts"], a["xs"],
                                                 a["ys"], a["ds"], a["out"], a["op"], a["n"], a["H"], a["W"], a["C"], a["D"],
                                                 a["Dpad"], f(a["bias"]), None)

    assert cost() == 0                                                       # n == 0: success without a launch
    assert cost(grid=None, consts=p, xs=p, ys=p, ds=p) == 0
    for bad in (dict(prev=None), dict(curr=None), dict(out=None), dict(n=-1), dict(H=0), dict(W=0), dict(C=0), dict(D=0),
                dict(Dpad=0), dict(grid=None), dict(grid=None, consts=p, xs=p, ys=p), dict(pp=0, C=16), dict(cp=8, C=16, pp=16),
                dict(op=0), dict(Dpad=0, D=6), dict(D=9), dict(pp=12), dict(cp=20), dict(op=12), dict(prev=p + 8),
                dict(curr=p + 2), dict(out=p + 8), dict(grid=p + 4), dict(grid=None, consts=p + 2, xs=p, ys=p, ds=p),
                dict(grid=None, consts=p, xs=p, ys=p, ds=p + 1), dict(bias=float("nan"))):
        assert cost(**bad) == 2, bad
    for unsupported in (dict(C=12, pp=16, cp=16), dict(C=4), dict(D=129, Dpad=136, op=136), dict(Dpad=12, op=16),
                        dict(H=0x1000000), dict(W=0x1000000), dict(n=0x4000, H=0x4000, W=0x4000)):
        assert cost(**unsupported) == 3, unsupported
    # the order: a BAD_PARAM condition wins over a NOT_SUPPORTED one, a pitch below the channels over its alignment
    assert cost(prev=None, C=12, pp=16, cp=16) == 2
    assert cost(C=12, pp=16, cp=16, out=p + 8) == 2
    assert cost(D=129, Dpad=136, op=136, grid=p + 4) == 2
    assert cost(D=129, Dpad=136, op=128) == 2
    assert cost(C=12, pp=8, cp=16) == 2
    assert cost(C=4, D=129, Dpad=136, op=136, n=1) == 3                      # refused with n > 0 too, before any launch

    def grid(**kw):
        a = dict(consts=p, xs=p, ys=p, ds=p, grid=p, n=0, D=6, H=2, W=3)
        a.update(kw)
        return lib.bevops_stereo_grid(a["consts"], a["xs"], a["ys"], a["ds"], a["grid"], a["n"], a["D"], a["H"], a["W"], None)

    assert grid() == 0
    for bad in (dict(consts=None), dict(xs=None), dict(ys=None), dict(ds=None), dict(grid=None), dict(n=-1), dict(D=0),
                dict(H=0), dict(W=-1), dict(consts=p + 2), dict(ds=p + 1), dict(grid=p + 4)):
        assert grid(**bad) == 2, bad
    for unsupported in (dict(D=129), dict(H=0x1000000), dict(n=0x10000, D=128, H=0x8000, W=0x8000)):
        assert grid(**unsupported) == 3, unsupported
    assert grid(D=129, grid=p + 4) == 2 and grid(D=129, n=1) == 3
    assert lib.bevops_query(b"bevops_stereo_cost_volume_f16") and lib.bevops_query(b"bevops_stereo_grid")


def test_wrapper_arguments():
    from bevformer_tensorrt_amd.functions import stereo_cost_volume, stereo_grid
    G, t = _fixture()
    with pytest.raises(ValueError, match="frustum_tables"):
        stereo_cost_volume(t("prev"), t("curr"), torch.zeros(2, 40), 6, 5.0)
    with pytest.raises(ValueError, match="grid"):
        stereo_cost_volume(t("prev"), t("curr"), torch.zeros(2, 5, 8, 12, 2), 6, 5.0)
    with pytest.raises(ValueError, match="one shape"):
        stereo_cost_volume(t("prev")[:, :4], t("curr"), t("grid"), 6, 5.0)
    with pytest.raises(ValueError, match="consts"):
        stereo_grid(torch.zeros(2, 39), (torch.zeros(3), torch.zeros(2), torch.zeros(6)))
