"""CPU side of the batched BEVDet index build: the torch statements at B > 1 (calibration_matrices_batched,
lidar_coor_plain on the 2-D buffer, prepare_stable) against the fixture recorded from the reference's own methods, and
every host-side answer of bevops_lss_voxel_prepare_batched and bevops_centerpoint_decode_ex, which return before any
device call."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import run_pinned
from util_lss_batched import check_arrays, digest, fixture, inputs, view_for


def statements_match_fixture():
    g, cases = fixture()
    assert cases == ["two_rigs", "empty_middle", "one_camera", "two_z_cells", "four_r50"]
    for case in cases:
        vt = view_for(g, case)
        args = inputs(g, case)
        B, N = args[0].shape[:2]
        calib = vt.calibration_matrices_batched(*args)
        assert calib.dtype == torch.float32 and tuple(calib.shape) == (B, N * 24 + 9), case
        assert np.array_equal(calib.numpy().view(np.int32), g[case + ".calib"].view(np.int32)), case
        for b in range(B):        # a row is that sample's own packed buffer
            one = vt.calibration_matrices(*(None if t is None else t[b:b + 1] for t in args))
            assert torch.equal(one, calib[b]), (case, b)
        coor = vt.lidar_coor_plain(calib)
        assert tuple(coor.shape[:2]) == (B, N), case
        assert np.array_equal(coor[:, :, ::7, ::3, ::5].numpy(), g[case + ".coor_sample"]), case
        assert digest(coor.numpy()) == str(g[case + ".coor_sha256"]), case
        ranks = vt.prepare_stable(coor)
        check_arrays(g, case, *(r.numpy() for r in ranks))
    mid = g["empty_middle.counts_per_sample"]
    assert mid[1].tolist() == [0, 0] and mid[0, 0] > 0 and mid[2, 0] > 0


def test_batched_statements_match_fixture_bit_exact():
    run_pinned("test_lss_prepare_batched_cpu", "statements_match_fixture")


def test_row_zero_at_batch_one_is_calibration_matrices():
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, LSSViewTransformer, jittered_rig
    vt = LSSViewTransformer(**BEVDET_R50, ops=object())
    rig = jittered_rig(vt, 3)
    one = vt.calibration_matrices(*rig)
    rows = vt.calibration_matrices_batched(*rig)
    assert tuple(rows.shape) == (1, 6 * 24 + 9) and torch.equal(rows[0], one)
    assert torch.equal(vt.lidar_coor_plain(rows), vt.lidar_coor_plain(one))
    with pytest.raises(ValueError):
        vt.calibration_matrices_batched(rig[0], None, rig[2], rig[3], rig[4], rig[5].repeat(2, 1, 1))


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def _aligned(nbytes=256):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16


def test_batched_prepare_answers_every_status_without_gpu(lib):
    f32x9 = ctypes.c_float * 9
    good = f32x9(-51.2, -51.2, -5, 0.8, 0.8, 8, 128, 128, 1)
    _keep, p = _aligned()
    grid = lambda *v: ctypes.cast(f32x9(*v), ctypes.c_void_p)
    size = lib.bevops_lss_voxel_prepare_batched_workspace_size
    r64 = lambda v: (v + 63) // 64 * 64
    for B in (1, 2, 16):
        n = B * 6 * 59 * 16 * 44
        blocks = -(-n // 2048)
        assert size(B, 6, 59, 16, 44) == 4 * (4 * r64(n) + r64(256 * blocks) + 256 + r64(blocks))
    assert size(1, 6, 59, 16, 44) == lib.bevops_lss_voxel_prepare_workspace_size(6, 59, 16, 44)
    assert size(0, 6, 59, 16, 44) == 0 and size(-1, 6, 59, 16, 44) == 0 and size(2, 6, 59, 16, 0) == 0
    assert size(17, 6, 59, 16, 44) == 0                                   # 17 x 249 216 points > 2^22
    assert size(4, 1, 64, 128, 128) > 0 and size(4, 1, 64, 128, 129) == 0  # exactly 2^22 points, and beyond
    assert size(2, 2, 1 << 15, 1 << 15, 1 << 15) == 0                      # (no overflow on the way)
    need = size(2, 6, 59, 16, 44)

    def call(frustum=p, calib=p, g=ctypes.cast(good, ctypes.c_void_p), outs=(p,) * 6, coor=None, batch=2, n=6, d=59,
             h=16, w=44, ws=p, ws_bytes=need):
        return lib.bevops_lss_voxel_prepare_batched(frustum, calib, g, *outs, coor, batch, n, d, h, w, ws,
                                                    ctypes.c_size_t(ws_bytes), None)
    assert call(frustum=None) == 2 and call(calib=None) == 2 and call(g=None) == 2 and call(ws=None) == 2
    for i in range(6):
        assert call(outs=(p,) * i + (None,) + (p,) * (5 - i)) == 2                   # every output is required
    assert call(batch=0) == 2 and call(batch=-3) == 2
    assert call(n=0) == 2 and call(d=-1) == 2 and call(h=0) == 2 and call(w=0) == 2
    assert call(ws_bytes=need - 1) == 2 and call(ws=p + 4) == 2                       # short / misaligned workspace
    assert call(ws_bytes=lib.bevops_lss_voxel_prepare_workspace_size(6, 59, 16, 44)) == 2   # the one-sample size is short
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.0, 8, 128, 128, 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, float("nan"), 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, float("inf"), 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(float("nan"), -51.2, -5, 0.8, 0.8, 8, 128, 128, 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 128, float("inf"), 1)) == 2
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 128, 0, 1)) == 2
    assert call(batch=17) == 3                                                          # beyond 2^22 points
    assert call(batch=2, n=64, d=1024) == 3
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 127.5, 128, 1)) == 3             # non-integral size
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 4096, 4096, 1)) == 3             # 2 x 2^24 cells
    # 2 x 2^23 cells = 2^24 passes the cell limit: the next check (the workspace) answers
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 4096, 2048, 1), ws_bytes=0) == 2
    assert call(g=grid(-51.2, -51.2, -5, 0.8, 0.8, 8, 4096, 2048, 1), batch=3, ws_bytes=0) == 3
    # the one-sample entry keeps its answer
    one = lib.bevops_lss_voxel_prepare(p, p, ctypes.cast(good, ctypes.c_void_p), *(p,) * 6, None, 2, 6, 59, 16, 44, p,
                                       ctypes.c_size_t(need), None)
    assert one == 3


def test_decode_ex_rejects_bad_params_without_gpu(lib):
    _keep, p = _aligned()
    f = ctypes.c_float
    rng = (f * 6)(-61.2, -61.2, -10, 61.2, 61.2, 10)
    dense = [1, 32, 16 * 16 * 32] * 6

    def call(strides=dense, maps=(p,) * 6, outs=(p,) * 4, batch=2, nc=10, h=16, w=16, k=50, r=rng, thr=0.1, dtype=1):
        s = None if strides is None else (ctypes.c_int64 * 18)(*strides)
        return lib.bevops_centerpoint_decode_ex(dtype, *maps, s, *outs, batch, nc, h, w, k, f(8), f(0.1), f(0.1),
                                                f(-51.2), f(-51.2), r, f(thr), 1, 0, None, 0, None)
    for i in range(18):                                                  # every stride is at least 1
        for bad in (0, -1):
            assert call(strides=dense[:i] + [bad] + dense[i + 1:]) == 2, i
    assert call(strides=[1 << 31, 32, 100] + dense[3:]) == 2             # channel / pixel strides are int32 values
    assert call(strides=None) == 2
    for i in (1, 2, 3, 5):                                               # height, dim, rot, heatmap are required
        assert call(maps=(p,) * i + (None,) + (p,) * (5 - i)) == 2
    for i in range(4):
        assert call(outs=(p,) * i + (None,) + (p,) * (3 - i)) == 2
    assert call(batch=0) == 2 and call(nc=0) == 2 and call(h=0) == 2 and call(k=0) == 2 and call(r=None) == 2
    assert call(k=10 * 16 * 16 + 1) == 2 and call(thr=float("nan")) == 2
    assert call(dtype=2) == 3                                            # int8 maps
    assert call(k=5000, nc=40) == 3                                      # beyond 4 096 winners
    # the plain entry answers the same way
    s12 = (ctypes.c_int32 * 12)(*[1, 32] * 6)
    plain = lambda s, k=50: lib.bevops_centerpoint_decode(1, *(p,) * 6, s, *(p,) * 4, 2, 10, 16, 16, k, f(8), f(0.1),
                                                          f(0.1), f(-51.2), f(-51.2), rng, f(0.1), 1, 0, None, 0, None)
    assert plain(None) == 2 and plain(s12, k=0) == 2 and plain((ctypes.c_int32 * 12)(*[1, 0] * 6)) == 2


def test_wrappers_are_exported_and_not_registered():
    import inspect
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as F
    for name in ("lss_voxel_prepare_batched", "lss_lidar_coor_batched"):
        assert name in F.__all__ and callable(getattr(F, name))
        assert name not in bev.TRT_FUNCTIONS
    assert inspect.signature(F.bev_pool_v2_indirect).parameters["batch"].default == 1
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner, LSSViewTransformer
    assert callable(LSSViewTransformer.calibration_matrices_batched)
    assert inspect.signature(BEVDetRunner.__init__).parameters["batch"].default == 1
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            BEVDetRunner(None, None, batch=bad)
    with pytest.raises(AssertionError):
        F.lss_voxel_prepare_batched(torch.zeros(2, 2, 2, 3), torch.zeros(2, 33), [0, 0, 0], [1, 1, 1], [4, 4, 1])
