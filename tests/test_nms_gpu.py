"""GPU: the BEV NMS kernels (csrc/nms.hip) through the C ABI and the Python layer.

  * every fixture of tests/golden/make_nms_golden.py (the reference's own Python; no candidate pair within 1e-3 of the
    threshold, so the reference's answer does not depend on its IoU kernel): count, kept rows, labels, copied columns,
    restored sizes and z equal to the fixture's BITS, zero tail;
  * `bev_iou` against the tests' fp64 oracle (util_nms.py) on the fixtures' boxes and on pairs built to be awkward:
    max |ours - fp64| <= 5e-4, half the fixtures' band -- what selection equality needs, no more.  Measured on one
    MI355X: 6.6e-07 on the fixtures' boxes, 5.9e-07 on the awkward pairs (design/postprocess.md);
  * invariants that hold for any correct NMS on any input, on 20 random scenes without a band guarantee and on
    BEVDet.get_bboxes over the model's own outputs;
  * determinism, indifference to what lies behind count_in, graph capture together with centerpoint_decode."""
import ctypes
import math

import numpy as np
import pytest
import torch

import util_nms as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
IOU_BOUND = 5e-4

ROTATE, CIRCLE = U.cases("rotate"), U.cases("circle")
ALL = ROTATE + CIRCLE
ids = lambda cs: [c["name"] for c in cs]


def _dev(c):
    t = lambda a: torch.from_numpy(a.copy()).to(DEV)
    return t(c["boxes"]), t(c["scores"]), t(c["labels"]), t(c["count"])


def _np(out):
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_fixture_through_bev_nms(case):
    import bevformer_tensorrt_amd as bev
    out = bev.bev_nms(*_dev(case), **U.kwargs_of(case), padded=True)
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.int32]
    assert out[0].shape == (case["boxes"].shape[0], case["post"], 9) and all(o.is_cuda for o in out)
    U.check_against_fixture(case, _np(out), "bev_nms")
    dicts = bev.bev_nms(*_dev(case), **U.kwargs_of(case))
    for b, it in enumerate(case["items"]):
        assert dicts[b]["index"].cpu().tolist() == it["keep"].tolist()
        assert U.bits_equal(dicts[b]["bboxes"].cpu().numpy(), it["bboxes"])


@pytest.mark.parametrize("case", ALL, ids=ids(ALL))
def test_fixture_through_the_c_abi(case):
    from bevformer_tensorrt_amd.utils import lib as L
    lib = L.load_library()
    boxes, scores, labels, count = _dev(case)
    B, N = scores.shape
    post = case["post"]
    out_b = torch.full((B, post, 9), 7.0, device=DEV)
    out_s = torch.full((B, post), 7.0, device=DEV)
    out_l = torch.full((B, post), 7, device=DEV, dtype=torch.int32)
    out_i = torch.full((B, post), 7, device=DEV, dtype=torch.int32)
    out_c = torch.full((B,), 7, device=DEV, dtype=torch.int32)
    need = lib.bevops_bev_nms_workspace_size(B, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    fac = case["factors"]
    fac_c = (ctypes.c_float * max(len(fac), 1))(*fac)
    st = lib.bevops_bev_nms(0 if case["kind"] == "rotate" else 1, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(),
                            count.data_ptr(), out_b.data_ptr(), out_s.data_ptr(), out_l.data_ptr(), out_c.data_ptr(),
                            out_i.data_ptr(), B, N, case["pre"] or 0, post, case["threshold"], fac_c, len(fac),
                            int(case["bottom"]), ws.data_ptr(), need, L.current_stream_ptr(boxes.device))
    assert st == 0
    torch.cuda.synchronize()
    U.check_against_fixture(case, _np((out_b, out_s, out_l, out_c, out_i)), "C ABI")


def test_count_in_null_and_index_null():
    """count_in = NULL means every row; index = NULL is allowed."""
    from bevformer_tensorrt_amd.utils import lib as L
    import bevformer_tensorrt_amd as bev
    lib = L.load_library()
    case = ROTATE[0]
    boxes, scores, labels, _ = _dev(case)
    got = bev.bev_nms(boxes, scores, labels, None, **U.kwargs_of(case), padded=True)
    U.check_against_fixture(case, _np(got), "count=None")
    B, N = scores.shape
    post = case["post"]
    out_b, out_s = torch.empty(B, post, 9, device=DEV), torch.empty(B, post, device=DEV)
    out_l, out_c = torch.empty(B, post, device=DEV, dtype=torch.int32), torch.empty(B, device=DEV, dtype=torch.int32)
    need = lib.bevops_bev_nms_workspace_size(B, N)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    fac_c = (ctypes.c_float * 10)(*case["factors"])
    st = lib.bevops_bev_nms(0, boxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), None, out_b.data_ptr(),
                            out_s.data_ptr(), out_l.data_ptr(), out_c.data_ptr(), None, B, N, case["pre"], post,
                            case["threshold"], fac_c, 10, 1, ws.data_ptr(), need, L.current_stream_ptr(boxes.device))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(out_b, got[0]) and torch.equal(out_c, got[3])


def test_empty_items_and_oversized_counts():
    import bevformer_tensorrt_amd as bev
    case = ROTATE[0]
    boxes, scores, labels, _ = _dev(case)
    boxes, scores, labels = boxes.repeat(3, 1, 1), scores.repeat(3, 1), labels.repeat(3, 1)
    count = torch.tensor([0, 10 ** 6, -4], dtype=torch.int32, device=DEV)
    out = _np(bev.bev_nms(boxes, scores, labels, count, **U.kwargs_of(case), padded=True))
    assert out[3].tolist() == [0, case["items"][0]["keep"].shape[0], 0]
    for b in (0, 2):
        assert not out[0][b].any() and not out[1][b].any() and not out[2][b].any() and not out[4][b].any()
    U.check_against_fixture(case, [o[1:2] for o in out], "count above num")


def test_equal_scores_rank_by_lower_row():
    import bevformer_tensorrt_amd as bev
    boxes = torch.zeros(1, 8, 9)
    for i in range(8):
        boxes[0, i, :7] = torch.tensor([10.0 * (i // 2), 0.0, 0.0, 2.0, 4.0, 1.5, 0.3])
    scores = torch.tensor([[0.5, 0.5, 0.5, 0.5, 0.5, 0.5, -0.0, 0.0]])
    labels = torch.zeros(1, 8, dtype=torch.int32)
    d = lambda: (boxes.to(DEV), scores.to(DEV), labels.to(DEV))
    out = bev.bev_nms(*d(), threshold=0.2, post_max_size=8, padded=True)
    assert int(out[3][0]) == 4 and out[4][0, :4].tolist() == [0, 2, 4, 6]
    out = bev.bev_nms(*d(), threshold=0.2, post_max_size=8, pre_max_size=3, padded=True)
    assert int(out[3][0]) == 2 and out[4][0, :2].tolist() == [0, 2]
    out = bev.bev_nms(*d(), nms_type="circle", threshold=1.0, post_max_size=2, padded=True)
    assert int(out[3][0]) == 2 and out[4][0, :2].tolist() == [0, 2]
    # a row with a NaN in its box neither suppresses nor is suppressed
    boxes[0, 0, 0] = float("nan")
    out = bev.bev_nms(*d(), threshold=0.2, post_max_size=8, padded=True)
    assert out[4][0, :int(out[3][0])].tolist() == [0, 1, 2, 4, 6]


# ------------------------------------------------------------------------------------------------ the pair test
def _awkward_pairs():
    rng = np.random.default_rng(5)
    A, B = [], []

    def base(n, aspect=None):
        a = np.zeros((n, 5))
        a[:, 0:2] = rng.uniform(-60, 60, (n, 2))
        if aspect is None:
            a[:, 2], a[:, 3] = rng.uniform(0.3, 5.0, n), rng.uniform(0.3, 12.0, n)
        else:
            a[:, 2], a[:, 3] = 12.0, 12.0 / aspect
        a[:, 4] = rng.uniform(-math.pi, math.pi, n)
        return a

    def local(a, du, dv):          # a's centre moved by du along its w axis and dv along its l axis
        c, s = np.cos(a[:, 4]), np.sin(a[:, 4])
        out = a.copy()
        out[:, 0] += du * c - dv * s
        out[:, 1] += du * s + dv * c
        return out

    n = 400
    a = base(n)                                                     # nearly identical
    A.append(a), B.append(a + rng.normal(0, 1, (n, 5)) * 10.0 ** rng.uniform(-7, -3, (n, 1)))
    a = base(n)                                                     # shared edge: same size and yaw, shifted along l
    A.append(a), B.append(local(a, 0.0, a[:, 3] * rng.uniform(0.0, 1.2, n)))
    a = base(n)                                                     # side by side, touching along one edge
    A.append(a), B.append(local(a, a[:, 2], a[:, 3] * rng.uniform(-0.5, 0.5, n)))
    a = base(n)                                                     # one corner touching
    b = local(a, a[:, 2], a[:, 3])
    A.append(a), B.append(b)
    a = base(n)                                                     # ... and rotated about the touching corner's box
    b = local(a, a[:, 2], a[:, 3])
    b[:, 4] += rng.uniform(-0.5, 0.5, n)
    A.append(a), B.append(b)
    a = base(n)                                                     # parallel edges 1e-4 apart (inside and outside)
    A.append(a), B.append(local(a, a[:, 2] + rng.choice([-1e-4, 1e-4], n), rng.uniform(-1, 1, n)))
    a = base(n)
    b = a.copy()
    b[:, 2:4] -= 2e-4                                               # inset by 1e-4 on every side
    A.append(a), B.append(b)
    a = base(n, aspect=30.0)                                        # 12 x 0.4 boxes crossing
    b = base(n, aspect=30.0)
    b[:, 0:2] = a[:, 0:2] + rng.uniform(-3, 3, (n, 2))
    A.append(a), B.append(b)
    a, b = base(n), base(n)                                         # any two boxes that overlap, far from the origin
    b[:, 0:2] = a[:, 0:2] + rng.uniform(-1.5, 1.5, (n, 2))
    A.append(a), B.append(b)
    return np.concatenate(A).astype(np.float32), np.concatenate(B).astype(np.float32)


def test_bev_iou_within_bound_of_fp64():
    """The measured maxima are printed; the bound is the one the selection needs (half the fixtures' band)."""
    import bevformer_tensorrt_amd as bev
    worst = 0.0
    for c in (ROTATE[0], next(c for c in ROTATE if c["name"] == "rot_n1000")):
        q = U.bev_of(c["boxes"][0], c["labels"][0], c["factors"])
        ours = bev.bev_iou(torch.from_numpy(q).to(DEV), torch.from_numpy(q).to(DEV)).cpu().numpy().astype(np.float64)
        want = U.iou_matrix(q)
        err = np.abs(ours - want).max()
        print(f"bev_iou, {c['name']} boxes ({(want > 0).sum()} overlapping entries): max |ours - fp64| = {err:.3e}")
        worst = max(worst, err)
        assert err <= IOU_BOUND
    a, b = _awkward_pairs()
    ours = np.concatenate([torch.diagonal(bev.bev_iou(torch.from_numpy(a[k:k + 400]).to(DEV),
                                                      torch.from_numpy(b[k:k + 400]).to(DEV))).cpu().numpy()
                           for k in range(0, len(a), 400)]).astype(np.float64)
    want = np.array([U.iou_pair(p, q) for p, q in zip(a, b)])
    err = np.abs(ours - want)
    for k in range(0, len(a), 400):
        print(f"bev_iou, awkward class {k // 400}: max |ours - fp64| = {err[k:k + 400].max():.3e}, "
              f"IoU range {want[k:k + 400].min():.3f} .. {want[k:k + 400].max():.3f}")
    print(f"bev_iou, awkward pairs overall: max |ours - fp64| = {err.max():.3e}")
    assert err.max() <= IOU_BOUND
    assert np.isfinite(ours).all() and ours.min() >= 0.0


def test_wrappers_on_gpu_tensors():
    import bevformer_tensorrt_amd as bev
    for c in (ROTATE[0], next(c for c in ROTATE if c["name"] == "rot_premax")):
        n = int(c["count"][0])
        xywhr = torch.from_numpy(U.bev_of(c["boxes"][0, :n], c["labels"][0, :n], c["factors"])).to(DEV)
        scores = torch.from_numpy(c["scores"][0, :n].copy()).to(DEV)
        keep = bev.nms_bev(xywhr, scores, c["threshold"], c["pre"], c["post"], xyxyr2xywhr=False)
        assert keep.is_cuda and keep.dtype == torch.int64 and keep.tolist() == c["items"][0]["keep"].tolist()
    x = torch.tensor([[0.0, 0.0, 2.0, 2.0, 0.0], [0.5, 0.0, 2.5, 2.0, 0.0], [5.0, 5.0, 6.0, 6.0, 0.0]], device=DEV)
    assert bev.nms_bev(x, torch.tensor([0.3, 0.9, 0.5], device=DEV), 0.5).tolist() == [1, 2]
    assert bev.nms_bev(x, torch.tensor([0.3, 0.9, 0.5], device=DEV), 0.7).tolist() == [1, 2, 0]
    for c in CIRCLE:
        dets = torch.from_numpy(np.concatenate([c["boxes"][0][:, :2], c["scores"][0][:, None]], 1)).to(DEV)
        keep = bev.circle_nms(dets, c["threshold"], post_max_size=c["post"])
        assert keep.is_cuda and keep.tolist() == c["items"][0]["keep"].tolist()


# ------------------------------------------------------------------------------------------------ invariants
def test_invariants_on_random_scenes():
    """No band guarantee here: a pair may sit at the threshold, so selection equality with an fp64 scan is not asserted;
    what every correct implementation satisfies is."""
    import bevformer_tensorrt_amd as bev
    kept_total = 0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        n = int(rng.integers(200, 501))
        boxes, scores, labels = U.clustered_scene(rng, n, neighbours=int(rng.integers(3, 12)))
        if seed % 4 == 0:
            scores[rng.integers(0, n, n // 5)] = scores[0]                # ties
        post = n if seed % 3 else n // 8
        pre = None if seed % 5 else n - 40
        factors = U.R50_FACTORS if seed % 2 == 0 else [0.7]
        t = lambda a: torch.from_numpy(a)[None].to(DEV)
        out = _np(bev.bev_nms(t(boxes), t(scores), t(labels), nms_type="rotate", threshold=0.2, pre_max_size=pre,
                              post_max_size=post, rescale_factor=factors, padded=True))
        kept_total += U.check_invariants(boxes, scores, labels, n, out[4][0], out[3][0], 0.2, pre, post, factors,
                                         f"scene {seed}")
    assert kept_total > 20 * 20


# ------------------------------------------------------------------------------------------------ contract
def test_bit_reproducible_and_blind_behind_count():
    import bevformer_tensorrt_amd as bev
    case = next(c for c in ROTATE if c["name"] == "rot_b2")
    boxes, scores, labels, count = _dev(case)
    kw = U.kwargs_of(case)
    first = bev.bev_nms(boxes, scores, labels, count, **kw, padded=True)
    cfirst = bev.bev_nms(boxes, scores, labels, count, **dict(kw, nms_type="circle", threshold=4.0), padded=True)
    for _ in range(20):
        again = bev.bev_nms(boxes, scores, labels, count, **kw, padded=True)
        cagain = bev.bev_nms(boxes, scores, labels, count, **dict(kw, nms_type="circle", threshold=4.0), padded=True)
        for a, b in zip(first + cfirst, again + cagain):
            assert torch.equal(a, b)
    for fill_b, fill_s, fill_l in ((float("nan"), float("nan"), -7), (3.0e38, 3.0e38, 2 ** 31 - 1), (0.0, 1.0, 0)):
        b2, s2, l2 = boxes.clone(), scores.clone(), labels.clone()
        for b, n in enumerate(count.tolist()):
            b2[b, n:], s2[b, n:], l2[b, n:] = fill_b, fill_s, fill_l
        other = bev.bev_nms(b2, s2, l2, count, **kw, padded=True)
        for a, b in zip(first, other):
            assert torch.equal(a, b)


CP_TAIL = [500, [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], [-51.2, -51.2], 8, [0.1, 0.1], 0.1]
NMS_KW = dict(nms_type="rotate", threshold=0.2, pre_max_size=1000, post_max_size=500, rescale_factor=U.R50_FACTORS,
              bottom_center=True, padded=True)


def _head_maps(g, shift):
    mk = lambda c, s=1.0, o=0.0: ((torch.randn(1, c, 128, 128, generator=g) * s + o).half().to(DEV)
                                  .contiguous(memory_format=torch.channels_last))
    return [mk(2), mk(1, 6.0), mk(3, 0.5, 0.5), mk(2), mk(2), mk(10, 1.0, -5.2 + shift)]


def test_graph_capture_with_centerpoint_decode():
    """Decode and NMS in one captured graph (a synchronising call inside would make the capture raise), replayed on
    three different head outputs, equal to the eager results."""
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(21)
    maps = _head_maps(g, 0.0)

    def run():
        cand = bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
        return cand + bev.bev_nms(*cand, **NMS_KW)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    seen = set()
    for r in range(3):
        for m, fresh in zip(maps, _head_maps(g, 0.6 * r)):
            m.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager = run()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
        n_cand, n_kept = int(out[3][0]), int(out[7][0])
        assert 0 < n_kept <= n_cand
        seen.add((n_cand, n_kept))
    assert len(seen) == 3, seen          # the replays did follow the inputs


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def bevdet_frames():
    from bevformer_tensorrt_amd import bevdet as D
    dev = torch.device(DEV)
    model = D.BEVDet(seed=0).to(dev, torch.float16)
    # a trained head's `dim` bias sits at the log of an object's size; the zero bias of random weights makes every
    # box about 1 m, smaller than the 0.8 m cell pitch can make overlap.  A car's log sizes, so that neighbours do.
    model.heads["dim"][1].bias.data.copy_(torch.tensor([0.67, 1.53, 0.5]))
    ranks = [r.to(dev) for r in model.view.get_bev_pool_input(*D.synthetic_rig(model.view))]
    g = torch.Generator().manual_seed(4)
    outs = [model(torch.randn(1, 6, 3, 256, 704, generator=g).to(dev, torch.float16), *ranks) for _ in range(2)]
    torch.cuda.synchronize()
    return model, outs


def test_bevdet_get_bboxes_on_the_models_own_outputs(bevdet_frames):
    """A random-weight head puts many overlapping neighbours among its 500 candidates, so some pair will sit inside the
    band: no selection equality is asserted here (the fixtures carry that); the invariants and the row identity are."""
    from bevformer_tensorrt_amd import bevdet as D
    model, outs = bevdet_frames
    cfg = D.CENTERPOINT_TEST_CFG_R50
    for fi, outputs in enumerate(outs):
        cand = _np(model.get_candidates(outputs, padded=True))
        got_t = model.get_bboxes(outputs, padded=True)
        got = _np(got_t)
        boxes, scores, labels, count, index = got
        assert boxes.shape == (1, 500, 9) and labels.dtype == np.int32 and index.dtype == np.int32
        n_cand, n = int(cand[3][0]), int(count[0])
        assert 0 < n < n_cand, "nothing was suppressed: the frame does not exercise the NMS"
        print(f"BEVDet frame {fi}: {n_cand} candidates -> {n} detections")
        U.check_invariants(cand[0][0], cand[1][0], cand[2][0], n_cand, index[0], n, cfg["nms_thr"], cfg["pre_max_size"],
                           cfg["post_max_size"], cfg["nms_rescale_factor"], f"get_bboxes frame {fi}")
        rows = index[0, :n]
        src = cand[0][0][rows]
        for col in (0, 1, 6, 7, 8):
            assert U.bits_equal(boxes[0, :n, col], src[:, col])
        assert U.bits_equal(scores[0, :n], cand[1][0][rows]) and np.array_equal(labels[0, :n], cand[2][0][rows])
        f = U.factors_of(cand[2][0][rows], cfg["nms_rescale_factor"])[:, None]
        sizes = (src[:, 3:6] * f) / f                                    # fp32, IEEE division
        assert U.bits_equal(boxes[0, :n, 3:6], sizes)
        assert U.bits_equal(boxes[0, :n, 2], src[:, 2] - sizes[:, 2] * np.float32(0.5))
        assert not boxes[0, n:].any() and not scores[0, n:].any() and not labels[0, n:].any() and not index[0, n:].any()
        trimmed = model.get_bboxes(outputs)
        assert len(trimmed) == 1 and len(trimmed[0]) == 3
        tb, ts, tl = trimmed[0]
        assert tb.shape == (n, 9) and tl.dtype == torch.int32
        assert torch.equal(tb, got_t[0][0, :n]) and torch.equal(ts, got_t[1][0, :n]) and torch.equal(tl, got_t[2][0, :n])


def test_bevdet_get_bboxes_inside_a_captured_graph(bevdet_frames):
    model, outs = bevdet_frames
    outputs = tuple(o.clone() for o in outs[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        model.get_bboxes(outputs, padded=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.get_bboxes(outputs, padded=True)
    for frame in outs:
        for dst, src in zip(outputs, frame):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, model.get_bboxes(frame, padded=True)):
            assert torch.equal(a, b)
