"""CPU side of BEVDet's device index build (csrc/lss_prepare.hip): the torch statements of its semantics
(LSSViewTransformer.calibration_matrices / lidar_coor_plain / prepare_stable) against the fixture recorded from the
reference's own methods, their relation to the existing voxel_pooling_prepare_v2, and the argument checks of the new
C-ABI entries, which return before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import run_pinned
from util_lss import check_arrays, digest, fixture, inputs, view_for


def statements_match_fixture():
    g, cases = fixture()
    assert len(cases) >= 10
    for case in cases:
        vt = view_for(g, case)
        calib = vt.calibration_matrices(*inputs(g, case))
        assert calib.dtype == torch.float32 and np.array_equal(calib.numpy().view(np.int32), g[case + ".calib"].view(np.int32)), case
        coor = vt.lidar_coor_plain(calib)
        assert np.array_equal(coor[0, :, ::7, ::3, ::5].numpy(), g[case + ".coor_sample"]), case
        assert digest(coor.numpy()) == str(g[case + ".coor_sha256"]), case
        ref_coor = vt.get_lidar_coor(*inputs(g, case))
        assert np.array_equal(coor.numpy().view(np.int32), ref_coor.numpy().view(np.int32)), case
        ranks = vt.prepare_stable(coor)
        if int(g[case + ".counts"][1]) == 0:
            assert all(r is None for r in ranks), case
            continue
        check_arrays(g, case, *(r.numpy() for r in ranks))


def test_statements_match_fixture_bit_exact():
    """calibration_matrices, lidar_coor_plain (= get_lidar_coor, bit for bit) and prepare_stable on every fixture
    case, digests exact; CPU kernel choice pinned as when the fixture was recorded."""
    run_pinned("test_lss_prepare_cpu", "statements_match_fixture")


@pytest.mark.parametrize("case", ["ref_r50", "jitter2", "z_cells", "small_grid", "one_cell"])
def test_prepare_stable_is_an_interval_permutation_of_the_reference_order(case):
    g, _ = fixture()
    vt = view_for(g, case)
    coor = vt.lidar_coor_plain(torch.from_numpy(g[case + ".calib"]))
    a = [r.numpy() for r in vt.voxel_pooling_prepare_v2(coor)]
    b = [r.numpy() for r in vt.prepare_stable(coor)]
    for i in (0, 3, 4):                      # ranks_bev, interval_starts, interval_lengths: order-free
        assert np.array_equal(a[i], b[i])
    D, H, W = vt.frustum.shape[:3]
    for rd_ref, rd, rf in ((a[1], b[1], b[2]),):
        assert np.array_equal(rf, (rd // (D * H * W)) * (H * W) + rd % (H * W))
        # stable = ascending point index inside every interval, and the same SET of points as the reference's order
        inside = np.ones(rd.size, bool)
        inside[b[3]] = False
        assert (np.diff(rd)[inside[1:]] > 0).all()
        key = b[0].astype(np.int64) * (1 << 32)
        assert np.array_equal(np.sort(key + rd_ref), key + rd)


def test_jittered_rigs_differ_and_are_deterministic():
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    g, _ = fixture()
    vt = view_for(g, "rig")
    a, b, a2 = (vt.calibration_matrices(*jittered_rig(vt, s)) for s in (1, 2, 1))
    assert torch.equal(a, a2) and not torch.equal(a, b) and a.numel() == 6 * 24 + 9


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_new_entries_reject_bad_params_without_gpu(lib):
    f32x9 = ctypes.c_float * 9
    good = f32x9(-51.2, -51.2, -5, 0.8, 0.8, 8, 128, 128, 1)
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    grid = lambda *v: ctypes.cast(f32x9(*v), ctypes.c_void_p)
    size = lib.bevops_lss_voxel_prepare_workspace_size
    need = size(6, 59, 16, 44)
    n, blocks = 6 * 59 * 16 * 44, -(-6 * 59 * 16 * 44 // 2048)
    r64 = lambda v: (v + 63) // 64 * 64
    assert need == 4 * (4 * r64(n) + r64(256 * blocks) + 256 + r64(blocks))
    assert size(0, 59, 16, 44) == 0 and size(6, 59, 16, -1) == 0
    assert size(64, 1024, 16, 44) == 0                                   # beyond 2^22 points
    assert size(1, 1, 1, 1) > 0 and size(1, 64, 256, 256) > 0            # exactly 2^22 points

    def call(frustum=p, calib=p, g=ctypes.cast(good, ctypes.c_void_p), outs=(p,) * 6, coor=None, batch=1, n=6, d=59,
             h=16, w=44, ws=p, ws_bytes=need):
        return lib.bevops_lss_voxel_prepare(frustum, calib, g, *outs, coor, batch, n, d, h, w, ws,
                                            ctypes.c_size_t(ws_bytes), None)
    assert call(frustum=None) == 2 and call(calib=None) == 2 and call(g=None) == 2 and call(ws=None) == 2
    for i in range(6):
        assert call(outs=(p,) * i + (None,) + (p,) * (5 - i)) == 2                   # every output is required
    assert call(n=0) == 2 and call(d=-1) == 2 and call(h=0) == 2 and call(w=0) == 2 and call(batch=0) == 2
    assert call(ws_bytes=need - 1) == 2 and call(ws=p + 4) == 2                       # short / misaligned workspace
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.0, 8, 128, 128, 1)) == 2              # zero interval
    assert call(g=grid(-51.2, -51.2, -5, 0.8, -0.8, 8, 128, 128, 1)) == 2             # negative interval
    assert call(g=grid(-51.2, -51.2, -5, float("nan"), 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, float("inf"), 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(float("nan"), -51.2, -5, 0.8, 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 128, 0, 1)) == 2                # empty grid
    assert call(batch=2) == 3                                                          # batch 1 only
    assert call(n=64, d=1024) == 3                                                     # beyond 2^22 points
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 127.5, 128, 1)) == 3            # non-integral size
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 8192, 8192, 1)) == 3            # beyond 2^24 cells
    f = ctypes.c_float
    pool = lib.bevops_bev_pool_v2_forward_indirect
    assert pool(1, p, p, p, p, p, p, p, None, p, 64, 100, 128, 128, f(1), f(1), f(1), None) == 2     # no device count
    assert pool(1, p, p, p, p, p, p, p, p, None, 64, 100, 128, 128, f(1), f(1), f(1), None) == 2     # no output
    assert pool(1, p, p, None, p, p, p, p, p, p, 64, 100, 128, 128, f(1), f(1), f(1), None) == 2     # no ranks
    assert pool(1, p, p, p, p, p, p, p, p, p, 64, -1, 128, 128, f(1), f(1), f(1), None) == 2
    assert pool(1, p, p, p, p, p, p, p, p, p, 0, 100, 128, 128, f(1), f(1), f(1), None) == 2
    assert pool(3, p, p, p, p, p, p, p, p, p, 64, 100, 128, 128, f(1), f(1), f(1), None) == 3        # uint8


def test_python_wrappers_are_exported_and_not_registered():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as F
    for name in ("lss_voxel_prepare", "lss_lidar_coor", "bev_pool_v2_indirect"):
        assert name in F.__all__ and callable(getattr(F, name))
        assert name not in bev.TRT_FUNCTIONS
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDetRunner, LSSViewTransformer
    assert callable(BEVDet.forward_calibrated) and callable(LSSViewTransformer.view_transform_calibrated)
    with pytest.raises(ValueError):
        BEVDetRunner(None, None, post="nms")
    with pytest.raises(AssertionError):
        F.lss_voxel_prepare(torch.zeros(2, 2, 2, 3), torch.zeros(33), [0, 0, 0], [1, 1, 1], [4, 4, 1])
