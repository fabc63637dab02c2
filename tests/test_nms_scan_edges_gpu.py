"""GPU: the edges of the one scan kernel both NMS entries share (csrc/nms.hip), each against the CPU statement of
postprocess.py on the same input bits, bit for bit (index, count, copied rows: both sides evaluate one fp32 operation
sequence for the circle and the axis-aligned pair tests, so no margin is needed).

bev_nms, circle mode, no pre_max_size: N = 63, 64, 65 (the last word partly filled, full, one row into the next) and
N = 4 096 (64 words: every lane of the scan wave owns one).
box_nms with M = 12 353 candidates out of N = 12 400 rows (193 words: the four-words-per-lane scan with all four word
classes in use, 32 mask rows staged per round): 193 clusters of 64 near-duplicates and one row on its own.  Three
quarters of a cluster rank side by side, so every word of the scan keeps one row; the last quarter ranks anywhere
behind, so those rows are suppressed from words far ahead.  The statement keeps 194 rows.  Then the same scene with
max_out = 150, which the scan reaches in a late round."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = g.cpu().numpy(), w.numpy()
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: output {i} differs"


@functools.lru_cache(maxsize=None)
def _circle_scene(n):
    rng = np.random.default_rng(1000 + n)
    boxes = np.zeros((1, n, 9), np.float32)
    side = 2.0 * np.sqrt(n)                                  # about four rows per threshold disc
    boxes[0, :, :2] = rng.uniform(-side / 2, side / 2, (n, 2))
    boxes[0, :, 2:6] = rng.uniform(0.5, 3.0, (n, 4))
    boxes[0, :, 6] = rng.uniform(-3.1, 3.1, n)
    scores = rng.permutation(n).astype(np.float32)[None] / n
    labels = rng.integers(0, 10, (1, n)).astype(np.int32)
    return tuple(torch.from_numpy(a) for a in (boxes, scores, labels))


@functools.lru_cache(maxsize=None)
def _circle_reference(n):
    from bevformer_tensorrt_amd.postprocess import bev_nms_torch
    return bev_nms_torch(*_circle_scene(n), nms_type="circle", threshold=4.0, post_max_size=n)


@pytest.mark.parametrize("n", [63, 64, 65, 4096])
def test_circle_nms_at_the_word_edges(n):
    import bevformer_tensorrt_amd as bev
    want = _circle_reference(n)
    kept = int(want[3][0])
    print(f"circle, N = {n}: {kept} kept")
    assert 0 < kept < n
    got = bev.bev_nms(*[t.to(DEV) for t in _circle_scene(n)], nms_type="circle", threshold=4.0, post_max_size=n, padded=True)
    _same(got, want, f"circle N = {n}")


BOX_N, BOX_CLUSTERS, BOX_CANDIDATES = 12400, 193, 12353


@functools.lru_cache(maxsize=None)
def _cluster_scene():
    rng = np.random.default_rng(12353)
    n, per = BOX_N, 64
    boxes, scores = np.zeros((n, 4), np.float32), np.full(n, 0.001, np.float32)       # 47 rows stay below the threshold
    labels = np.zeros(n, np.int32)
    rows = rng.permutation(n)
    for c in range(BOX_CLUSTERS + 1):                                                  # the last one is a single row
        mine = rows[c * per:(c + 1) * per] if c < BOX_CLUSTERS else rows[BOX_CLUSTERS * per:BOX_CLUSTERS * per + 1]
        cx, cy = 40.0 * (c % 16), 40.0 * (c // 16)
        jit = rng.uniform(-0.3, 0.3, (len(mine), 4)).astype(np.float32)
        boxes[mine] = np.array([cx, cy, cx + 10.0, cy + 10.0], np.float32) + jit
        labels[mine] = c % 5
        band = 0.99 - 0.005 * c                                                        # cluster c's band of scores
        s = band - 0.00005 * np.arange(len(mine))
        s[48:] = rng.uniform(0.011, band - 0.0045, max(len(mine) - 48, 0))             # ... and its stragglers, anywhere behind
        scores[mine] = s.astype(np.float32)
    assert int((scores >= 0.01).sum()) == BOX_CANDIDATES
    return tuple(torch.from_numpy(a[None]) for a in (boxes, scores, labels))


@functools.lru_cache(maxsize=None)
def _cluster_reference(max_out):
    from bevformer_tensorrt_amd.postprocess import box_nms_torch
    return box_nms_torch(*_cluster_scene(), score_threshold=0.01, iou_threshold=0.65, class_aware=True, max_out=max_out)


@pytest.mark.parametrize("max_out", [None, 150], ids=["all", "max_out_150"])
def test_box_nms_193_words_of_clusters(max_out):
    import bevformer_tensorrt_amd as bev
    want = _cluster_reference(max_out)
    kept, full = int(want[3][0]), int(_cluster_reference(None)[3][0])
    last = int(np.flatnonzero(np.sort(-_cluster_scene()[1][0].numpy(), kind="stable") == -float(want[1][0, kept - 1]))[0])
    print(f"box, M = {BOX_CANDIDATES}: {kept} kept of {full}, the last one at rank {last} (word {last // 64})")
    assert full == BOX_CLUSTERS + 1 and kept == (full if max_out is None else max_out)
    assert last // 64 >= 128                                  # the scan is still keeping rows in the third word class
    got = bev.box_nms(*[t.to(DEV) for t in _cluster_scene()], score_threshold=0.01, iou_threshold=0.65, class_aware=True,
                      max_out=max_out, padded=True)
    _same(got, want, f"box clusters, max_out={max_out}")
