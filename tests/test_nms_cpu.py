"""CPU-only checks of the BEV NMS: the tests' own fp64 IoU against closed forms, the package's CPU statement
(`bev_nms_torch`) against the fixtures the reference's Python made (tests/golden/make_nms_golden.py), the tie rule, the
reference-signature wrappers and the argument checks of the C entries.  The kernels are checked by test_nms_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import util_nms as U

ROTATE, CIRCLE = U.cases("rotate"), U.cases("circle")
ALL = ROTATE + CIRCLE
ids = lambda cs: [c["name"] for c in cs]


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_fp64_iou_closed_forms():
    U.closed_form_checks()


def test_fp64_iou_against_point_count():
    pairs = [([3.0, -2.0, 4.0, 2.0, 0.7], [3.5, -1.5, 3.0, 1.5, -0.4]),
             ([-20.0, 11.0, 12.3, 2.9, 2.2], [-18.0, 12.0, 4.6, 1.95, 0.3]),
             ([0.5, 0.5, 1.0, 1.0, math.pi / 4], [0.9, 0.2, 1.4, 0.6, -1.0])]
    for a, b in pairs:
        counted, resolution = U.point_count_iou(a, b, 2000)
        exact = U.iou_pair(a, b)
        assert 0.02 < exact < 0.98
        assert abs(counted - exact) <= resolution, (a, b, counted, exact, resolution)


def test_package_fp64_iou_agrees_with_the_tests_own():
    """Two fp64 implementations written separately (box frame, vectorised / absolute coordinates, per pair)."""
    from bevformer_tensorrt_amd.postprocess import bev_iou_fp64
    c = ROTATE[0]
    bev = U.bev_of(c["boxes"][0], c["labels"][0], c["factors"])[:200]
    ours = bev_iou_fp64(torch.from_numpy(bev), torch.from_numpy(bev)).numpy()
    want = U.iou_matrix(bev)
    assert np.abs(ours - want).max() <= 1e-9
    U.closed_form_checks(lambda a, b: float(bev_iou_fp64(torch.tensor([a], dtype=torch.float64),
                                                         torch.tensor([b], dtype=torch.float64))[0, 0]), tol=1e-12)


# ------------------------------------------------------------------------------------------------ fixtures
def _torch_inputs(c, device=None):
    t = lambda a: torch.from_numpy(a.copy()) if device is None else torch.from_numpy(a.copy()).to(device)
    return t(c["boxes"]), t(c["scores"]), t(c["labels"]), t(c["count"])


@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_cpu_statement_reproduces_the_fixture_bits(case):
    from bevformer_tensorrt_amd.postprocess import bev_nms_torch
    out = bev_nms_torch(*_torch_inputs(case), **U.kwargs_of(case))
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.int32]
    assert out[0].shape == (case["boxes"].shape[0], case["post"], 9)
    U.check_against_fixture(case, [o.numpy() for o in out], "bev_nms_torch")


def test_fixtures_are_what_the_generator_promises():
    """The properties the generator asserted, re-read from the committed files (cheap ones only)."""
    names = {c["name"] for c in ALL}
    assert {"rot_r50", "rot_b2", "rot_n1", "rot_n63", "rot_n64", "rot_n65", "rot_n1000", "rot_scalar", "rot_nofactor",
            "rot_thr", "rot_postmax", "rot_premax"} <= names
    assert sum(n.startswith("cir_") for n in names) == 12
    for c in ALL:
        for b, it in enumerate(c["items"]):
            n = int(c["count"][b])
            k = it["keep"].shape[0]
            assert np.unique(c["scores"][b, :n]).size == n
            assert 0 < k <= c["post"] and (n == 1 or k < n)
            if c["factors"]:
                changed = it["bboxes"][:, 3:6].view(np.uint32) != c["boxes"][b][it["keep"]][:, 3:6].view(np.uint32)
                assert n == 1 or changed.any(), f"{c['name']}: the divide-back is not exercised"
    b2 = next(c for c in ROTATE if c["name"] == "rot_b2")
    assert np.isnan(b2["boxes"][0, int(b2["count"][0]):]).any()          # garbage behind the count
    assert next(c for c in ROTATE if c["name"] == "rot_postmax")["items"][0]["keep"].shape[0] == 60
    assert next(c for c in ROTATE if c["name"] == "rot_premax")["boxes"].shape[1] == 1300


def test_equal_scores_rank_by_lower_row():
    from bevformer_tensorrt_amd.postprocess import bev_nms_torch
    # rows 0..5: three disjoint pairs of identical boxes, all scores equal -> the lower row of each pair survives, in
    # row order; then a score of -0.0 ties with +0.0
    boxes = torch.zeros(1, 8, 9)
    for i in range(8):
        boxes[0, i, :7] = torch.tensor([10.0 * (i // 2), 0.0, 0.0, 2.0, 4.0, 1.5, 0.3])
    scores = torch.tensor([[0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -0.0, 0.0]])
    labels = torch.zeros(1, 8, dtype=torch.int32)
    out = bev_nms_torch(boxes, scores, labels, threshold=0.2, post_max_size=8)
    assert int(out[3][0]) == 4 and out[4][0, :4].tolist() == [0, 2, 4, 6]
    out = bev_nms_torch(boxes, scores, labels, threshold=0.2, post_max_size=8, pre_max_size=3)
    assert int(out[3][0]) == 2 and out[4][0, :2].tolist() == [0, 2]      # the cut takes rows 0, 1, 2
    out = bev_nms_torch(boxes, scores, labels, nms_type="circle", threshold=1.0, post_max_size=2)
    assert int(out[3][0]) == 2 and out[4][0, :2].tolist() == [0, 2]


def test_circle_compares_the_squared_distance():
    from bevformer_tensorrt_amd.postprocess import bev_nms_torch
    boxes = torch.zeros(1, 2, 9)
    boxes[0, 1, 0] = 3.0                                # distance 3, squared 9
    scores, labels = torch.tensor([[0.9, 0.8]]), torch.zeros(1, 2, dtype=torch.int32)
    assert int(bev_nms_torch(boxes, scores, labels, nms_type="circle", threshold=4.0, post_max_size=2)[3][0]) == 2
    assert int(bev_nms_torch(boxes, scores, labels, nms_type="circle", threshold=9.0, post_max_size=2)[3][0]) == 1


def test_reference_signature_wrappers_on_cpu_tensors():
    import bevformer_tensorrt_amd as bev
    for c in (ROTATE[0], next(c for c in ROTATE if c["name"] == "rot_premax")):
        n = int(c["count"][0])
        xywhr = torch.from_numpy(U.bev_of(c["boxes"][0, :n], c["labels"][0, :n], c["factors"]))
        scores = torch.from_numpy(c["scores"][0, :n].copy())
        keep = bev.nms_bev(xywhr, scores, c["threshold"], c["pre"], c["post"], xyxyr2xywhr=False)
        assert keep.dtype == torch.int64 and keep.tolist() == c["items"][0]["keep"].tolist()
    # corner form: axis-aligned boxes given as (x1, y1, x2, y2, 0)
    x = torch.tensor([[0.0, 0.0, 2.0, 2.0, 0.0], [0.5, 0.0, 2.5, 2.0, 0.0], [5.0, 5.0, 6.0, 6.0, 0.0]])
    assert bev.nms_bev(x, torch.tensor([0.3, 0.9, 0.5]), 0.5).tolist() == [1, 2]          # IoU 0.6 > 0.5
    assert bev.nms_bev(x, torch.tensor([0.3, 0.9, 0.5]), 0.7).tolist() == [1, 2, 0]
    for c in (CIRCLE[0], CIRCLE[-1]):
        dets = np.concatenate([c["boxes"][0][:, :2], c["scores"][0][:, None]], 1)
        keep = bev.circle_nms(dets, c["threshold"], post_max_size=c["post"])
        assert isinstance(keep, list) and keep == c["items"][0]["keep"].tolist()
        keep_t = bev.circle_nms(torch.from_numpy(dets), c["threshold"], post_max_size=c["post"])
        assert keep_t.tolist() == keep
    iou = bev.bev_iou(torch.tensor([[0.0, 0.0, 4.0, 2.0, 0.0]]), torch.tensor([[1.0, 0.0, 4.0, 2.0, 0.0]]))
    assert iou.dtype == torch.float32 and abs(float(iou[0, 0]) - 6.0 / 10.0) < 1e-6


def test_bevdet_test_cfg_and_exports():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import bevdet
    from bevformer_tensorrt_amd.utils.register import TRT_FUNCTIONS
    cfg = bevdet.CENTERPOINT_TEST_CFG_R50
    assert cfg["nms_type"] == "rotate" and cfg["nms_thr"] == 0.2 and cfg["pre_max_size"] == 1000
    assert cfg["post_max_size"] == 500 and cfg["nms_rescale_factor"] == U.R50_FACTORS
    assert cfg["min_radius"] == U.R50_MIN_RADIUS
    assert callable(bevdet.BEVDet.get_bboxes)
    for name in ("bev_nms", "nms_bev", "circle_nms", "bev_iou"):
        assert callable(getattr(bev, name))
        assert name not in TRT_FUNCTIONS


# ------------------------------------------------------------------------------------------------ C ABI
def test_nms_entries_reject_bad_params_without_gpu():
    """Argument checks that return before any device call: 2 = BAD_PARAM, 3 = NOT_SUPPORTED (helper.h:19-25)."""
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    f, sz = ctypes.c_float, ctypes.c_size_t
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    fac = (ctypes.c_float * 10)(*U.R50_FACTORS)
    need = lib.bevops_bev_nms_workspace_size(1, 500)
    assert need >= 500 * 8 * 8                                    # at least the 500 x 8 words of the matrix
    assert lib.bevops_bev_nms_workspace_size(2, 500) >= 2 * 500 * 8 * 8
    assert lib.bevops_bev_nms_workspace_size(1, 4096) >= 4096 * 64 * 8
    assert lib.bevops_bev_nms_workspace_size(0, 500) == 0 and lib.bevops_bev_nms_workspace_size(1, 0) == 0
    assert lib.bevops_bev_nms_workspace_size(1, 4097) == 0
    big = sz(1 << 30)

    def call(mode=0, boxes=p, out=p, index=p, num=500, post=500, thr=0.2, factors=fac, nf=10, ws=p, wsb=big, pre=1000,
             batch=1):
        return lib.bevops_bev_nms(mode, boxes, p, p, p, out, p, p, p, index, batch, num, pre, post, f(thr), factors, nf,
                                  1, ws, wsb, None)

    assert call(boxes=None) == 2 and call(out=None) == 2 and call(ws=None) == 2          # NULL
    assert call(num=4097, post=500) == 3                                                   # beyond 4 096 rows
    assert call(post=0) == 2 and call(post=501) == 2 and call(num=0) == 2 and call(batch=0) == 2
    assert call(thr=float("nan")) == 2 and call(thr=float("inf")) == 2
    assert call(mode=2) == 2
    zero = (ctypes.c_float * 10)(*([1.0] * 9 + [0.0]))
    assert call(factors=zero) == 2                                                         # factor 0
    assert call(factors=(ctypes.c_float * 10)(*([1.0] * 9 + [-1.0]))) == 2
    assert call(factors=(ctypes.c_float * 10)(*([1.0] * 9 + [float("nan")]))) == 2
    assert call(factors=None, nf=3) == 2 and call(nf=-1) == 2
    assert call(wsb=sz(need - 1)) == 2                                                     # short workspace
    assert call(ws=p + 4) == 2                                                             # misaligned workspace
    assert lib.bevops_bev_iou(None, 1, p, 1, p, None) == 2
    assert lib.bevops_bev_iou(p, 0, p, 1, p, None) == 2 and lib.bevops_bev_iou(p, 1, p, 1, None, None) == 2
    assert lib.bevops_bev_iou(p, 1 << 20, p, 1 << 20, p, None) == 3


def test_nms_entries_are_in_the_registry():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    for sym in ("bevops_bev_nms", "bevops_bev_nms_workspace_size", "bevops_bev_iou"):
        assert lib.bevops_query(sym.encode()) == ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value
