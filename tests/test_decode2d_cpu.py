"""CPU: the 2-D heads' torch statements (bevformer_tensorrt_amd/postprocess.py) against the fixtures of
tests/golden/make_decode2d_golden.py (an independent numpy / float32 statement), the conditions those fixtures must
meet, the status codes and size queries of the three C-ABI entries (every call below returns before a device call), and
the two mmdet-shaped entry points on CPU tensors.

CenterNet and the NMS contain only +, -, x, / and comparisons: bit for bit.  YOLOX: labels, prior order and the rows
whose log sizes are 0 (w = h = stride exactly: their corners are cx, cy plus or minus an exact half stride, so they pin
cx and cy) exact; the columns that go through exp or the sigmoid against float64 at util_decode2d.BAR_ULP -- twice the
larger of the measured errors of torch's fp32 CPU ops and of the kernel, rounded up to a whole ulp."""
import ctypes
import math

import numpy as np
import pytest
import torch

import util_decode2d as U

BAD_PARAM, NOT_SUPPORTED = 2, 3
F32, F16, I8 = 0, 1, 2
T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------ fixture conditions
def test_bars_follow_the_measurements():
    for col in ("corner", "score"):
        assert U.BAR_ULP[col] == math.ceil(2 * max(U.MEASURED_ULP[col].values()))


@pytest.mark.parametrize("case", U.yx_cases(), ids=lambda c: c["name"])
def test_yolox_fixture_conditions(case):
    U.check_logits(case["cls"], case["top2"], case["name"])
    again = U.np_yolox(case["cls"], case["box"], case["obj"], case["strides"], case["scale"])
    for key in ("boxes", "scores", "labels", "boxes64", "scores64", "exact", "top2"):
        assert U.bits_equal(again[key], case[key]), key          # the stored columns are the statement's
    P = case["scores"].shape[1]
    for b in range(case["scores"].shape[0]):
        U.check_scores(case["scores64"][b], case["score_thr"], case["name"])
        cand = U.candidates(case["scores"][b], P, case["score_thr"])
        assert np.array_equal(np.sort(cand), np.nonzero(case["scores64"][b] >= case["score_thr"])[0])
        U.check_iou_band(case["boxes64"][b], cand, case["iou_thr"], case["name"])      # all pairs: both NMS flavours
    assert case["exact"].any()
    for a in (0, 1):
        want = U.np_box_nms(case["boxes"], case["scores"], case["labels"], None, case["score_thr"], case["iou_thr"], a,
                            case["max_out"])
        assert all(U.bits_equal(w, s) for w, s in zip(want, case["nms"][a]))


@pytest.mark.parametrize("case", U.cn_cases(), ids=lambda c: c["name"])
def test_centernet_fixture_conditions(case):
    heat = case["heat"]
    ties_wanted = case["name"] in ("cn_constant", "cn_plateau", "cn_few_peaks", "cn_borders")
    nz = heat[heat != 0]
    if not ties_wanted:
        assert np.unique(nz).size == heat.size, "equal values in a map whose case is not about ties"
    again = U.np_centernet(heat, case["wh"], case["off"], case["k"], case["kernel"], case["inp"], case["border"],
                           case["scale"])
    for got, key in zip(again, ("boxes", "scores", "labels", "count", "index")):
        assert U.bits_equal(got, case[key]), key
    if case["f16"]:
        for key in ("heat", "wh", "off"):
            assert U.bits_equal(case[key].astype(np.float16).astype(np.float32), case[key])


def test_fixture_cases_cover_the_list():
    cn = {c["name"]: c for c in U.cn_cases()}
    assert cn["cn_3x8x12"]["heat"].shape == (1, 3, 8, 12) and cn["cn_3x8x12"]["k"] == 10
    assert cn["cn_1x1x1"]["heat"].shape == (1, 1, 1, 1) and cn["cn_1x1x1"]["k"] == 1
    assert (cn["cn_3x8x12"]["scores"] > 0).all() and (cn["cn_few_peaks"]["scores"] == 0).sum() == 6
    assert np.array_equal(cn["cn_constant"]["index"][0], np.arange(12))
    assert cn["cn_plateau"]["index"][0, :2].tolist() == [12, 13]
    assert cn["cn_kernel1"]["kernel"] == 1 and cn["cn_meta"]["inp"] == (511, 509)
    assert cn["cn_meta"]["heat"].shape[-2:] == (128, 128) and cn["cn_meta"]["border"] is not None
    assert cn["cn_b2"]["heat"].shape[0] == 2 and not np.array_equal(cn["cn_b2"]["scale"][0], cn["cn_b2"]["scale"][1])
    assert cn["cn_f16"]["f16"]
    rows, cols = np.divmod(cn["cn_borders"]["index"][0], 11)
    assert {(0, 0), (0, 10), (8, 0), (8, 10)} <= set(zip(rows.tolist(), cols.tolist()))
    yx = {c["name"]: c for c in U.yx_cases()}
    assert yx["yx_base"]["levels"].tolist() == [[8, 8, 8], [4, 4, 16], [2, 2, 32]] and yx["yx_base"]["cls"][0].shape[1] == 3
    assert yx["yx_ragged"]["levels"][:, :2].tolist() == [[5, 7], [3, 4], [2, 2]] and len(yx["yx_l1"]["cls"]) == 1
    assert yx["yx_b2"]["scores"].shape[0] == 2 and yx["yx_norescale"]["scale"] is None
    assert yx["yx_none"]["nms"][1][3].tolist() == [0]
    assert (yx["yx_all"]["scores"] >= yx["yx_all"]["score_thr"]).all()
    tw = yx["yx_twoclass"]
    kept = lambda a: set(tw["nms"][a][4][0, :tw["nms"][a][3][0]].tolist())
    assert U.bits_equal(tw["boxes"][0, 0], tw["boxes"][0, 1]) and {0, 1} <= kept(1) and 1 not in kept(0)
    neg = yx["yx_negative"]["nms"][1]
    assert (neg[0][0, :neg[3][0]] < 0).any()
    assert yx["yx_maxout"]["nms"][1][3][0] == yx["yx_maxout"]["max_out"] == 5


# ------------------------------------------------------------------------------------------------ torch statements
@pytest.mark.parametrize("case", U.cn_cases(), ids=lambda c: c["name"])
def test_centernet_torch_equals_fixture(case):
    from bevformer_tensorrt_amd.postprocess import centernet_decode_torch
    dt = torch.float16 if case["f16"] else torch.float32
    out = centernet_decode_torch(T(case["heat"]).to(dt), T(case["wh"]).to(dt), T(case["off"]).to(dt), case["k"],
                                 case["inp"], case["kernel"], case["border"], case["scale"], return_index=True)
    for got, key in zip(out[:5], ("boxes", "scores", "labels", "count", "index")):
        assert U.bits_equal(got.numpy(), case[key]), key
    # the optional score test: kept rows first, zeros behind
    thr = float(np.median(case["scores"]))
    got = centernet_decode_torch(T(case["heat"]), T(case["wh"]), T(case["off"]), case["k"], case["inp"], case["kernel"],
                                 case["border"], case["scale"], score_threshold=thr)
    want = U.np_centernet(case["heat"], case["wh"], case["off"], case["k"], case["kernel"], case["inp"], case["border"],
                          case["scale"], thr)
    assert all(U.bits_equal(g.numpy(), w) for g, w in zip(got, want[:4]))


@pytest.mark.parametrize("case", U.nm_cases(), ids=lambda c: c["name"])
def test_box_nms_torch_equals_fixture(case):
    from bevformer_tensorrt_amd.postprocess import box_nms_torch
    got = box_nms_torch(T(case["boxes"]), T(case["scores"]), T(case["labels"]), T(case["count"]),
                        score_threshold=case["score_thr"], iou_threshold=case["iou_thr"], class_aware=case["aware"],
                        max_out=case["max_out"])
    for g, w in zip(got, case["want"]):
        assert U.bits_equal(g.numpy(), w)


@pytest.mark.parametrize("case", U.yx_cases(), ids=lambda c: c["name"])
def test_yolox_torch_against_fixture(case):
    from bevformer_tensorrt_amd.postprocess import box_nms_torch, yolox_decode_torch
    cls, box, obj = U.yx_levels(case)
    boxes, scores, labels = yolox_decode_torch(cls, box, obj, case["strides"], case["scale"])
    assert U.bits_equal(labels.numpy(), case["labels"])
    ex = case["exact"]
    assert U.bits_equal(boxes.numpy()[ex], case["boxes"][ex]), "rows without a transcendental: cx, cy, corners exact"
    corner, score = U.yolox_errors(boxes.numpy(), scores.numpy(), case)
    print(f"{case['name']}: torch fp32 CPU ops against float64: corners {corner:.3f} ulp, score {score:.3f} ulp")
    assert corner <= U.BAR_ULP["corner"] and score <= U.BAR_ULP["score"]
    # the NMS on the fixture's own decode output (same input bits): bit for bit, both flavours
    for a in (0, 1):
        got = box_nms_torch(T(case["boxes"]), T(case["scores"]), T(case["labels"]), score_threshold=case["score_thr"],
                            iou_threshold=case["iou_thr"], class_aware=bool(a), max_out=case["max_out"])
        for g, w in zip(got, case["nms"][a]):
            assert U.bits_equal(g.numpy(), w)


def _metas(case, b_count, with_border=True):
    metas = []
    for b in range(b_count):
        m = {"batch_input_shape": case.get("inp", (64, 64))}
        if case.get("scale") is not None:
            m["scale_factor"] = np.asarray(case["scale"][b], np.float32)
        if with_border and case.get("border") is not None:
            bx, by = case["border"][b]
            m["border"] = np.array([by, 0.0, bx, 0.0], np.float32)       # mmdet: (top, bottom, left, right)
        metas.append(m)
    return metas


def test_get_bboxes_on_cpu_tensors_return_mmdet_tuples():
    from bevformer_tensorrt_amd.postprocess import centernet_get_bboxes, yolox_get_bboxes
    cn = {c["name"]: c for c in U.cn_cases()}
    for name in ("cn_b2", "cn_meta", "cn_3x8x12"):
        c = cn[name]
        B = c["heat"].shape[0]
        metas = _metas(c, B)
        for m in metas:
            m.setdefault("scale_factor", np.ones(4, np.float32))
        res = centernet_get_bboxes([T(c["heat"])], [T(c["wh"])], [T(c["off"])], metas, rescale=c["scale"] is not None,
                                   topk=c["k"], local_maximum_kernel=c["kernel"])
        assert len(res) == B
        for b, (det, lab) in enumerate(res):
            assert det.shape == (c["k"], 5) and lab.shape == (c["k"],) and lab.dtype == torch.int64
            assert U.bits_equal(det[:, :4].numpy(), c["boxes"][b]) and U.bits_equal(det[:, 4].numpy(), c["scores"][b])
            assert np.array_equal(lab.numpy(), c["labels"][b])
    for c in U.yx_cases():
        cls, box, obj = U.yx_levels(c)
        B = cls[0].shape[0]
        metas = [{"scale_factor": np.asarray(c["scale"][b], np.float32) if c["scale"] is not None else np.ones(4, np.float32)}
                 for b in range(B)]
        res = yolox_get_bboxes(cls, box, obj, metas, rescale=c["scale"] is not None, score_thr=c["score_thr"],
                               iou_threshold=c["iou_thr"], strides=c["strides"], max_out=c["max_out"])
        want = c["nms"][1]
        assert len(res) == B
        for b, (det, lab) in enumerate(res):
            n = int(want[3][b])
            assert det.shape == (n, 5) and lab.shape == (n,) and lab.dtype == torch.int64
            assert np.array_equal(lab.numpy(), want[2][b, :n])          # the kept set, in order (labels identify it with
            rows = want[4][b, :n]                                         # the boxes below)
            assert np.allclose(det[:, :4].numpy(), c["boxes"][b][rows], rtol=1e-5, atol=1e-5)
            assert np.allclose(det[:, 4].numpy(), c["scores"][b][rows], rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


@pytest.fixture(scope="module")
def mem():
    buf = (ctypes.c_char * 4096)()
    return buf, ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 128


def test_centernet_status_codes(lib, mem):
    _, p = mem
    f = ctypes.c_float
    st6 = (ctypes.c_int32 * 6)(96, 1, 96, 1, 96, 1)
    big = ctypes.c_size_t(1 << 40)

    def call(dtype=F32, heat=p, wh=p, off=p, strides=st6, boxes=p, B=1, C=3, H=8, W=12, k=10, kernel=3, inp=(32, 48),
             border=None, scale=None, thr=-1.0, ws=p, nbytes=big):
        return lib.bevops_centernet_decode(dtype, heat, wh, off, strides, boxes, p, p, p, B, C, H, W, k, kernel, inp[0],
                                           inp[1], border, scale, f(thr), ws, nbytes, None)
    assert call(heat=None) == BAD_PARAM and call(wh=None) == BAD_PARAM and call(off=None) == BAD_PARAM
    assert call(strides=None) == BAD_PARAM and call(boxes=None) == BAD_PARAM
    assert call(B=0) == BAD_PARAM and call(C=0) == BAD_PARAM and call(inp=(0, 48)) == BAD_PARAM
    assert call(dtype=I8) == NOT_SUPPORTED and call(dtype=7) == BAD_PARAM
    assert call(k=0) == NOT_SUPPORTED and call(k=289) == NOT_SUPPORTED                 # 1 <= k <= C H W = 288
    assert call(C=80, H=128, W=128, k=4097) == NOT_SUPPORTED                           # k <= 4 096
    assert call(C=2, H=4096, W=4096, k=100) == NOT_SUPPORTED                           # C H W <= 2^24
    assert call(C=1 << 20, H=1 << 20, W=1 << 20, k=100) == NOT_SUPPORTED               # (no overflow on the way)
    assert call(kernel=2) == NOT_SUPPORTED and call(kernel=9) == NOT_SUPPORTED and call(kernel=0) == BAD_PARAM
    assert call(B=65) == NOT_SUPPORTED
    assert call(thr=float("nan")) == BAD_PARAM
    assert call(strides=(ctypes.c_int32 * 6)(96, 1, 0, 1, 96, 1)) == BAD_PARAM
    need = lib.bevops_centernet_decode_workspace_size(1, 3, 8, 12, 10)
    assert need == 1 * 1 * 10 * 8
    assert call(ws=None) == BAD_PARAM and call(nbytes=ctypes.c_size_t(need - 1)) == BAD_PARAM
    assert call(ws=p + 4) == BAD_PARAM                                                 # 8-byte alignment
    for bad in (float("nan"), float("inf"), 0.0):
        assert call(scale=(f * 4)(1.0, bad, 1.0, 1.0)) == BAD_PARAM
    assert call(border=(f * 2)(float("inf"), 0.0)) == BAD_PARAM


def test_yolox_status_codes(lib, mem):
    _, p = mem
    f = ctypes.c_float
    ptrs = (ctypes.c_void_p * 9)(*([p] * 9))
    shapes = (ctypes.c_int32 * 27)(*([4, 4, 8] * 9))
    strides = (ctypes.c_int32 * 54)(*([16, 1] * 27))

    def call(dtype=F32, cls=ptrs, box=ptrs, obj=ptrs, shp=shapes, strd=strides, out=p, B=1, L=3, C=3, scale=None):
        return lib.bevops_yolox_decode(dtype, cls, box, obj, shp, strd, out, p, p, B, L, C, scale, None)
    assert call(cls=None) == BAD_PARAM and call(box=None) == BAD_PARAM and call(obj=None) == BAD_PARAM
    assert call(shp=None) == BAD_PARAM and call(strd=None) == BAD_PARAM and call(out=None) == BAD_PARAM
    assert call(B=0) == BAD_PARAM and call(L=0) == BAD_PARAM and call(C=0) == BAD_PARAM
    assert call(L=9) == NOT_SUPPORTED and call(B=65) == NOT_SUPPORTED
    assert call(dtype=I8) == NOT_SUPPORTED and call(dtype=5) == BAD_PARAM
    assert call(cls=(ctypes.c_void_p * 3)(p, None, p)) == BAD_PARAM
    assert call(shp=(ctypes.c_int32 * 9)(4, 4, 8, 0, 4, 16, 2, 2, 32)) == BAD_PARAM
    assert call(shp=(ctypes.c_int32 * 9)(4, 4, 8, 4, 4, 0, 2, 2, 32)) == BAD_PARAM
    assert call(shp=(ctypes.c_int32 * 9)(4096, 4096, 8, 4096, 4096, 16, 2, 2, 32)) == NOT_SUPPORTED     # 2^25 priors
    assert call(strd=(ctypes.c_int32 * 18)(*([16, 1] * 8 + [16, 0]))) == BAD_PARAM
    assert call(scale=(f * 4)(1.0, float("nan"), 1.0, 1.0)) == BAD_PARAM


def test_box_nms_status_codes(lib, mem):
    _, p = mem
    f = ctypes.c_float
    big = ctypes.c_size_t(1 << 40)

    def call(boxes=p, scores=p, labels=p, out=p, count=p, B=1, N=100, thr=0.01, iou=0.65, aware=1, max_out=100, ws=p,
             nbytes=big):
        return lib.bevops_box_nms(boxes, scores, labels, None, out, p, p, count, None, B, N, f(thr), f(iou), aware,
                                  max_out, ws, nbytes, None)
    assert call(boxes=None) == BAD_PARAM and call(scores=None) == BAD_PARAM and call(labels=None) == BAD_PARAM
    assert call(out=None) == BAD_PARAM and call(count=None) == BAD_PARAM and call(ws=None) == BAD_PARAM
    assert call(B=0) == BAD_PARAM and call(N=0) == BAD_PARAM and call(aware=2) == BAD_PARAM
    assert call(N=16385, max_out=10) == NOT_SUPPORTED and call(B=65536) == NOT_SUPPORTED
    assert call(max_out=0) == BAD_PARAM and call(max_out=101) == BAD_PARAM
    assert call(thr=float("nan")) == BAD_PARAM
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(iou=bad) == BAD_PARAM
    need = lib.bevops_box_nms_workspace_size(1, 100)
    assert need == 16 + 400 + 2400 + 100 * 2 * 8
    assert call(nbytes=ctypes.c_size_t(need - 1)) == BAD_PARAM and call(ws=p + 4) == BAD_PARAM
    assert lib.bevops_box_nms_workspace_size(1, 16384) == 16 + 65536 + 393216 + 16384 * 256 * 8     # 32 MiB of words


def test_size_queries_are_zero_exactly_where_the_entries_answer_not_supported(lib, mem):
    """With every pointer valid but NO workspace, a supported shape answers BAD_PARAM (before any device call) and an
    unsupported one NOT_SUPPORTED: the query is 0 for exactly the latter."""
    _, p = mem
    f = ctypes.c_float
    st6 = (ctypes.c_int32 * 6)(1, 1, 1, 1, 1, 1)
    for B, C, H, W, k in ((1, 3, 8, 12, 10), (1, 1, 1, 1, 1), (64, 80, 128, 128, 100), (65, 3, 8, 12, 10),
                          (1, 80, 128, 128, 4096), (1, 80, 128, 128, 4097), (1, 3, 8, 12, 288), (1, 3, 8, 12, 289),
                          (1, 256, 256, 256, 100), (1, 256, 256, 257, 100), (2, 1, 9000, 1, 1500)):
        size = lib.bevops_centernet_decode_workspace_size(B, C, H, W, k)
        st = lib.bevops_centernet_decode(F32, p, p, p, st6, p, p, p, p, B, C, H, W, k, 3, 64, 64, None, None, f(-1.0),
                                         None, 0, None)
        assert st in (BAD_PARAM, NOT_SUPPORTED) and (size == 0) == (st == NOT_SUPPORTED), (B, C, H, W, k, size, st)
        if size:
            assert size == B * ((C * H * W + 8191) // 8192) * k * 8
    for B, N in ((1, 1), (1, 8400), (4, 16384), (1, 16385), (65535, 2), (65536, 2)):
        size = lib.bevops_box_nms_workspace_size(B, N)
        st = lib.bevops_box_nms(p, p, p, None, p, p, p, p, None, B, N, f(0.01), f(0.65), 1, 1, p, 0, None)
        assert st in (BAD_PARAM, NOT_SUPPORTED) and (size == 0) == (st == NOT_SUPPORTED), (B, N, size, st)


def test_wrappers_are_exported_beside_the_registry():
    import bevformer_tensorrt_amd as bev
    for name in ("centernet_decode", "yolox_decode", "box_nms"):
        assert callable(getattr(bev, name)) and name not in bev.TRT_FUNCTIONS
