#!/usr/bin/env python3
"""Golden vectors for the 2-D heads: CenterNet decode, YOLOX decode and the axis-aligned batched NMS.

mmdet and mmcv are not part of this project's environment and the reference's Python only subclasses them, so these
fixtures are NOT made by the reference's own code.  They are made by tests/util_decode2d.py: an independent numpy /
float32 statement of the published algorithms (mmdet 2.x CenterNetHead.decode_heatmap / get_bboxes, YOLOXHead
_bbox_decode / get_bboxes / _bboxes_nms, mmcv batched_nms) in the operation order include/bevops.h fixes, which imports
nothing from the package.  Parity with the libraries themselves stays unpinned (design/postprocess.md).

    python tests/golden/make_decode2d_golden.py          ->  tests/golden/decode2d.npz

The generator ASSERTS (and tests/test_decode2d_cpu.py re-asserts on the stored arrays) what keeps a comparison from
hiding a failure:
  * YOLOX: no score within 1e-5 (relative) of score_thr; no two candidate scores of an image closer than 1e-5
    (relative); the top two class logits of every prior at least 1e-3 apart and |logit| <= 12 (argmax before and after
    the sigmoid then agree); no candidate pair -- of any labels, which covers the class-blind run too -- with a float64
    IoU within 1e-3 of the threshold.  A draw that misses a condition is drawn again with the next seed.
  * CenterNet: all values of a map distinct except where a tie is the point of the case (constant, plateau, the zeros
    of the sparse maps).
  * every case does what its name says (fewer peaks than k, count 0, cut by max_out, kept only under class_aware, ...).
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import util_decode2d as U  # noqa: E402

F32 = np.float32


def distinct(rng, shape, denom=None):
    """Distinct values in (0, 1): a permutation of 1 .. n over n + 1 (or over `denom`, for fp16-exact values)."""
    n = int(np.prod(shape))
    return ((rng.permutation(n) + 1).astype(np.float64) / (denom or (n + 1))).astype(F32).reshape(shape)


def n_peaks(heat, kernel):
    B, C, H, W = heat.shape
    r = (kernel - 1) // 2
    pad = np.full((B, C, H + 2 * r, W + 2 * r), -np.inf, F32)
    pad[..., r:r + H, r:r + W] = heat
    hmax = np.max([pad[..., dy:dy + H, dx:dx + W] for dy in range(kernel) for dx in range(kernel)], 0)
    return ((hmax == heat) & (heat != 0)).reshape(B, -1).sum(1)


def make_centernet(res):
    names = []

    def add(name, heat, k, kernel, inp, seed, border=None, scale=None, f16=False, heads=None):
        rng = np.random.default_rng(seed)
        B, C, H, W = heat.shape
        wh = rng.uniform(1.0, 9.0, (B, 2, H, W)).astype(F32) if heads is None else heads[0]
        off = rng.uniform(0.0, 1.0, (B, 2, H, W)).astype(F32) if heads is None else heads[1]
        if f16:
            heat, wh, off = (a.astype(np.float16) for a in (heat, wh, off))
            assert np.unique(heat).size == heat.size, f"{name}: fp16 rounding made values equal"
        out = U.np_centernet(heat, wh, off, k, kernel, inp, border, scale)
        res[f"{name}_heat"], res[f"{name}_wh"], res[f"{name}_off"] = heat, wh, off
        res[f"{name}_params"] = np.array([k, kernel, inp[0], inp[1], int(f16)], np.int64)
        if border is not None:
            res[f"{name}_border"] = np.asarray(border, F32)
        if scale is not None:
            res[f"{name}_scale"] = np.asarray(scale, F32)
        for key, a in zip(("boxes", "scores", "labels", "count", "index"), out):
            res[f"{name}_{key}"] = a
        names.append(name)
        peaks = n_peaks(np.asarray(heat, F32), kernel)
        print(f"  {name}: {B} x {C} x {H} x {W}, k {k}, kernel {kernel}, peaks {peaks.tolist()}, "
              f"zeros selected {[int((out[1][b] == 0).sum()) for b in range(B)]}")
        return out, peaks

    rng = np.random.default_rng(100)
    out, peaks = add("cn_3x8x12", distinct(rng, (1, 3, 8, 12)), 10, 3, (32, 48), 1)
    assert peaks[0] > 10 and (out[1] > 0).all(), "more peaks than k"
    add("cn_1x1x1", distinct(rng, (1, 1, 1, 1)), 1, 3, (4, 4), 2)
    # two bumps on a 6 x 6 map: fewer peaks than k, the rest of the top k are zeros in flat-index order
    yy, xx = np.mgrid[0:6, 0:6]
    bump = lambda cy, cx, a: a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 1.7)
    few = np.maximum(bump(1, 4, 0.9), bump(4, 1, 0.6)).astype(F32)[None, None]
    out, peaks = add("cn_few_peaks", few, 8, 3, (24, 24), 3)
    assert peaks[0] == 2 and int((out[1][0] == 0).sum()) == 6
    zeros = out[4][0][2:]
    assert (np.diff(zeros) > 0).all(), "zeros not in flat-index order"
    out, _ = add("cn_constant", np.full((1, 2, 5, 7), 0.5, F32), 12, 3, (20, 28), 4)
    assert np.array_equal(out[4][0], np.arange(12)), "a constant map must return the first k flat indices"
    # peaks in the four corners and on the four borders of a 9 x 11 map
    edge = np.zeros((1, 1, 9, 11), F32)
    spots = [(0, 0), (0, 10), (8, 0), (8, 10), (0, 5), (8, 5), (4, 0), (4, 10), (4, 5)]
    for i, (y, x) in enumerate(spots):
        edge[0, 0, y, x] = 0.95 - 0.07 * i
    out, peaks = add("cn_borders", edge, 9, 3, (36, 44), 5)
    assert peaks[0] == 9 and sorted(out[4][0].tolist()) == sorted(y * 11 + x for y, x in spots)
    # a plateau of two equal neighbours: both are maxima of their windows, both kept, lower flat index first
    plat = (distinct(rng, (1, 1, 5, 5)) * F32(0.5)).astype(F32)
    plat[0, 0, 2, 2] = plat[0, 0, 2, 3] = 0.9
    out, _ = add("cn_plateau", plat, 4, 3, (20, 20), 6)
    assert out[4][0][:2].tolist() == [12, 13] and (out[1][0][:2] == F32(0.9)).all()
    out, _ = add("cn_kernel1", distinct(rng, (1, 3, 8, 12)), 10, 1, (32, 48), 7)
    assert (np.diff(out[1][0]) < 0).all()
    # border, a non-unit scale factor, a non-integral input / map ratio; 16 384 cells = two selection chunks
    big = distinct(rng, (1, 1, 128, 128))
    h16 = lambda lo, hi: rng.uniform(lo, hi, (1, 2, 128, 128)).astype(np.float16).astype(F32)     # (stored as fp16)
    out, _ = add("cn_meta", big, 100, 3, (511, 509), 8, border=[[3.0, 5.0]], scale=[[0.8, 0.75, 0.8, 0.75]],
                 heads=(h16(1.0, 9.0), h16(0.0, 1.0)))
    res["cn_meta_wh"], res["cn_meta_off"] = res["cn_meta_wh"].astype(np.float16), res["cn_meta_off"].astype(np.float16)
    assert F32(511 / 128) != F32(4) and F32(509 / 128) != F32(4)
    add("cn_b2", distinct(rng, (2, 3, 8, 12)), 10, 3, (33, 47), 9, border=[[0.0, 2.0], [6.0, 1.0]],
        scale=[[1.5, 1.25, 1.5, 1.25], [0.6, 0.7, 0.6, 0.7]])
    # 9 000 cells: one full chunk and a ragged one with fewer cells than k
    out, _ = add("cn_ragged", distinct(rng, (1, 3, 60, 50)), 1500, 3, (240, 200), 10)
    assert (out[1][0] == 0).any(), "k beyond the peaks"
    add("cn_f16", distinct(rng, (1, 3, 8, 12), denom=512), 10, 3, (32, 48), 11, f16=True)
    add("cn_kernel5", distinct(rng, (1, 2, 9, 9)), 6, 5, (36, 36), 12)
    res["cn_names"] = np.array(names)


def draw_yolox(rng, B, C, shapes, strides, obj_range, off_range=(-1.0, 1.0)):
    cls, box, obj = [], [], []
    for (H, W), s in zip(shapes, strides):
        cls.append(rng.uniform(-6.0, 6.0, (B, C, H, W)).astype(F32))
        b = np.concatenate([rng.uniform(*off_range, (B, 2, H, W)), rng.uniform(1.2, 2.1, (B, 2, H, W))], 1).astype(F32)
        exact = rng.random((B, H, W)) < 0.25          # log sizes exactly 0: w = h = stride, no transcendental
        b[:, 2][exact] = 0
        b[:, 3][exact] = 0
        box.append(b)
        obj.append(rng.uniform(*obj_range, (B, 1, H, W)).astype(F32))
    return cls, box, obj


def make_yolox(res, nm):
    names = []

    def add(name, B, C, shapes, strides, thr, iou_thr, scale, seed, obj_range=(-3.0, 4.0), max_out=None, edit=None,
            off_range=(-1.0, 1.0), expect=None):
        for attempt in range(200):
            rng = np.random.default_rng(seed * 1000 + attempt)
            cls, box, obj = draw_yolox(rng, B, C, shapes, strides, obj_range, off_range)
            if edit:
                edit(cls, box, obj)
            dec = U.np_yolox(cls, box, obj, strides, scale)
            try:
                U.check_logits(cls, dec["top2"], name)
                for b in range(B):
                    U.check_scores(dec["scores64"][b], thr, f"{name}[{b}]")
                    cand = U.candidates(dec["scores"][b], dec["scores"].shape[1], thr)
                    assert np.array_equal(np.sort(cand), np.nonzero(dec["scores64"][b] >= thr)[0])
                    U.check_iou_band(dec["boxes64"][b], cand, iou_thr, f"{name}[{b}]")
                P = dec["scores"].shape[1]
                post = P if max_out is None else max_out
                nms = {a: U.np_box_nms(dec["boxes"], dec["scores"], dec["labels"], None, thr, iou_thr, a, post)
                       for a in (0, 1)}
                ncand = [int((dec["scores"][b] >= F32(thr)).sum()) for b in range(B)]
                if expect:
                    expect(dec, nms, ncand)
            except AssertionError as e:
                last = e
                continue
            break
        else:
            raise AssertionError(f"{name}: no draw meets the conditions (last: {last})")
        res[f"{name}_levels"] = np.array([[H, W, s] for (H, W), s in zip(shapes, strides)], np.int32)
        for l in range(len(shapes)):
            res[f"{name}_cls{l}"], res[f"{name}_box{l}"], res[f"{name}_obj{l}"] = cls[l], box[l], obj[l]
        if scale is not None:
            res[f"{name}_scale"] = np.asarray(scale, F32)
        res[f"{name}_params"] = np.array([thr, iou_thr, post], np.float64)
        for key in ("boxes", "scores", "labels", "boxes64", "scores64", "exact", "top2"):
            res[f"{name}_{key}"] = dec[key]
        for a in (0, 1):
            for key, arr in zip(("boxes", "scores", "labels", "count", "index"), nms[a]):
                res[f"{name}_nms{a}_{key}"] = arr
        names.append(name)
        print(f"  {name}: {P} priors, attempt {attempt}, candidates {ncand}, kept class-aware {nms[1][3].tolist()}, "
              f"class-blind {nms[0][3].tolist()}, exact rows {int(dec['exact'].sum())}")
        return dec, nms

    S3, R3 = [(8, 8), (4, 4), (2, 2)], [(5, 7), (3, 4), (2, 2)]
    some = lambda dec, nms, nc: _assert(all(0 < nms[1][3][b] < nc[b] < dec["scores"].shape[1] for b in range(len(nc))),
                                        "keeps all or none, or nothing is below the threshold")
    add("yx_base", 1, 3, S3, [8, 16, 32], 0.3, 0.65, [[1.6, 1.6, 1.6, 1.6]], 1, expect=some)
    add("yx_ragged", 1, 3, R3, [8, 16, 32], 0.3, 0.65, [[1.25, 1.5, 1.25, 1.5]], 2, expect=some)
    add("yx_l1", 1, 3, [(8, 8)], [8], 0.3, 0.65, [[2.0, 2.0, 2.0, 2.0]], 3, expect=some)
    add("yx_b2", 2, 3, S3, [8, 16, 32], 0.3, 0.65, [[1.6, 1.6, 1.6, 1.6], [0.75, 0.7, 0.75, 0.7]], 4, expect=some)
    add("yx_norescale", 1, 3, S3, [8, 16, 32], 0.3, 0.65, None, 5, expect=some)
    add("yx_none", 1, 3, S3, [8, 16, 32], 0.01, 0.65, [[1.6, 1.6, 1.6, 1.6]], 6, obj_range=(-12.0, -8.0),
        expect=lambda dec, nms, nc: _assert(nc == [0] and nms[1][3][0] == 0, "rows above the threshold"))
    add("yx_all", 1, 3, S3, [8, 16, 32], 0.01, 0.65, [[1.6, 1.6, 1.6, 1.6]], 7, obj_range=(0.0, 4.0),
        expect=lambda dec, nms, nc: _assert(nc == [84] and 0 < nms[1][3][0] < 84, "not every row is a candidate"))

    def twins(cls, box, obj):
        # priors 0 and 1 of level 0 decode to the SAME box (cx = 1 * 8 + 0 = 0 * 8 + 8) with different classes
        box[0][0, :, 0, 0] = [1.0, 0.5, 0.75, 0.75]
        box[0][0, :, 0, 1] = [0.0, 0.5, 0.75, 0.75]
        cls[0][0, :, 0, 0], cls[0][0, :, 0, 1] = [5.0, -2.0, -3.0], [-2.0, 4.5, -3.0]
        obj[0][0, 0, 0, 0], obj[0][0, 0, 0, 1] = 5.0, 4.0

    def twins_expect(dec, nms, nc):
        assert U.bits_equal(dec["boxes"][0, 0], dec["boxes"][0, 1]) and dec["labels"][0, :2].tolist() == [0, 1]
        aware, blind = set(nms[1][4][0, :nms[1][3][0]].tolist()), set(nms[0][4][0, :nms[0][3][0]].tolist())
        assert {0, 1} <= aware and 0 in blind and 1 not in blind, "the twin is kept only under class_aware"
    add("yx_twoclass", 1, 3, S3, [8, 16, 32], 0.3, 0.65, None, 8, edit=twins, expect=twins_expect)
    add("yx_negative", 1, 3, S3, [8, 16, 32], 0.3, 0.65, [[1.6, 1.6, 1.6, 1.6]], 9, off_range=(-6.0, -1.0),
        expect=lambda dec, nms, nc: _assert((nms[1][0][0, :nms[1][3][0]] < 0).any() and nms[1][3][0] > 1,
                                            "no kept box with a negative coordinate"))

    def cut(dec, nms, nc):
        free = U.np_box_nms(dec["boxes"], dec["scores"], dec["labels"], None, 0.3, 0.65, 1, 84)
        assert nms[1][3][0] == 5 < free[3][0] and np.array_equal(nms[1][4][0], free[4][0, :5])
    add("yx_maxout", 1, 3, S3, [8, 16, 32], 0.3, 0.65, [[1.6, 1.6, 1.6, 1.6]], 10, max_out=5, expect=cut)
    res["yx_names"] = np.array(names)


def _assert(cond, what):
    assert cond, what


def scene(rng, n, labels=3):
    """n boxes in clusters, so that the NMS both keeps and suppresses."""
    centres = rng.uniform(-20.0, 120.0, (max(n // 4, 1), 2))
    c = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 3.0, (n, 2))
    wh = rng.uniform(8.0, 30.0, (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(F32)
    return boxes, rng.permutation(n).astype(F32) / F32(n + 1) + F32(0.001), rng.integers(0, labels, n).astype(np.int32)


def make_nms(res):
    names = []

    def add(name, boxes, scores, labels, count, thr, iou_thr, aware, max_out, expect=None):
        want = U.np_box_nms(boxes, scores, labels, count, thr, iou_thr, aware, max_out)
        for b in range(scores.shape[0]):
            n = scores.shape[1] if count is None else int(np.clip(count[b], 0, scores.shape[1]))
            cand = U.candidates(scores[b], n, thr)
            U.check_iou_band(boxes[b].astype(np.float64), cand, iou_thr, f"{name}[{b}]")
        if expect:
            expect(want)
        res[f"{name}_in_boxes"], res[f"{name}_in_scores"], res[f"{name}_in_labels"] = boxes, scores, labels
        if count is not None:
            res[f"{name}_in_count"] = np.asarray(count, np.int32)
        res[f"{name}_params"] = np.array([thr, iou_thr, aware, max_out], np.float64)
        for key, arr in zip(("boxes", "scores", "labels", "count", "index"), want):
            res[f"{name}_{key}"] = arr
        names.append(name)
        print(f"  {name}: {scores.shape}, kept {want[3].tolist()}")

    def repaired(seed, n, iou_thr):
        for attempt in range(500):
            rng = np.random.default_rng(seed * 1000 + attempt)
            bx, sc, lb = scene(rng, n)
            try:
                U.check_iou_band(bx.astype(np.float64), np.arange(n), iou_thr, "draw")
            except AssertionError:
                continue
            return rng, bx, sc, lb
        raise AssertionError("no draw meets the IoU band")

    for n in (1, 64, 65, 130):
        rng, bx, sc, lb = repaired(20 + n, n, 0.5)
        add(f"nm_n{n}", bx[None], sc[None], lb[None], None, -np.inf, 0.5, 1, n,
            expect=(lambda w, n=n: _assert(n == 1 or 0 < w[3][0] < n, "keeps all or none")))
    # equal scores: lower input row first (rows 2k and 2k + 1 share a score)
    rng, bx, sc, lb = repaired(31, 40, 0.5)
    sc = (np.arange(40) // 2).astype(F32) / F32(32) + F32(0.1)
    sc[7] = -sc[7] * 0          # a -0 beside ...
    sc[6] = 0.0                 # ... a +0: equal, row 6 first
    add("nm_ties", bx[None], sc[None], lb[None], None, -np.inf, 0.5, 0, 40)
    # two items, counts below N, garbage (NaN and huge values) behind the counts, a threshold that cuts
    rng, bx0, sc0, lb0 = repaired(32, 50, 0.45)
    _, bx1, sc1, lb1 = repaired(33, 17, 0.45)
    boxes = rng.normal(0, 1e6, (2, 60, 4)).astype(F32)
    boxes.reshape(-1)[::3] = np.nan
    scores = np.full((2, 60), 0.99, F32)
    labels = rng.integers(0, 3, (2, 60)).astype(np.int32)
    boxes[0, :50], scores[0, :50], labels[0, :50] = bx0, sc0, lb0
    boxes[1, :17], scores[1, :17], labels[1, :17] = bx1, sc1, lb1
    add("nm_count_b2", boxes, scores, labels, [50, 17], 0.2, 0.45, 1, 30,
        expect=lambda w: _assert(np.isfinite(w[0]).all() and (w[3] > 0).all(), "garbage behind the count was read"))
    # a row with a non-finite coordinate suppresses nothing and is not suppressed
    rng, bx, sc, lb = repaired(34, 30, 0.5)
    top = int(np.argmax(sc))
    bx[top, 2] = np.inf
    add("nm_nonfinite", bx[None], sc[None], lb[None], None, -np.inf, 0.5, 0, 30,
        expect=lambda w: _assert(w[4][0, 0] == top, "the non-finite row is not kept first"))
    res["nm_names"] = np.array(names)


def main():
    res = {}
    print("CenterNet")
    make_centernet(res)
    print("YOLOX")
    make_yolox(res, None)
    print("box NMS")
    make_nms(res)
    path = os.path.join(OUT, "decode2d.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "fixture above the repository's 1 MiB limit"


if __name__ == "__main__":
    main()
