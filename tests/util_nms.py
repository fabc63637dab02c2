"""Shared by test_nms_cpu.py / test_nms_gpu.py and by tests/golden/make_nms_golden.py: an fp64 IoU of rotated
rectangles written independently of the package (general convex clipping in ABSOLUTE coordinates with cross products,
one pair at a time -- neither the frame nor the code of bevformer_tensorrt_amd/postprocess.py), the golden cases of
tests/golden/nms_*.npz as python objects, scene builders and the invariant checker of the NMS."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# configs/bevdet/bevdet-r50-cbgs.py:173-182
R50_FACTORS = [1.0, 0.7, 0.7, 0.4, 0.55, 1.1, 1.0, 1.0, 1.5, 3.5]
R50_MIN_RADIUS = [4, 12, 10, 1, 0.85, 0.175]
# typical (w, l, h) per nuScenes class, in the order of the config's class list
CLASS_SIZES = [(1.95, 4.6, 1.7), (2.5, 6.9, 2.8), (2.8, 6.4, 3.2), (2.9, 11.0, 3.5), (2.9, 12.3, 3.9),
               (2.5, 0.5, 1.0), (0.8, 2.1, 1.5), (0.6, 1.7, 1.3), (0.7, 0.7, 1.8), (0.4, 0.4, 1.1)]
COPIED, SIZES = (0, 1, 6, 7, 8), (3, 4, 5)


# ------------------------------------------------------------------------------------------------ fp64 IoU
def corners(box, T=float):
    """Corners (counter-clockwise) of (x, y, w, l, yaw), w along (cos yaw, sin yaw), as 4 (x, y) pairs of scalars of
    type T (float = fp64; numpy.float32 rounds every operation to fp32)."""
    x, y, w, l, r = (T(v) for v in box)
    c, s, h = T(math.cos(r)), T(math.sin(r)), T(0.5)
    ux, uy, vx, vy = h * w * c, h * w * s, -(h * l * s), h * l * c
    return [(x + ux + vx, y + uy + vy), (x - ux + vx, y - uy + vy), (x - ux - vx, y - uy - vy),
            (x + ux - vx, y + uy - vy)]


def _clip_convex(subject, clip):
    """Sutherland-Hodgman: polygon `subject` (list of points) against the convex counter-clockwise polygon `clip`."""
    out = list(subject)
    n = len(clip)
    for e in range(n):
        ax, ay = clip[e]
        bx, by = clip[(e + 1) % n]
        side = lambda p: (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)      # >= 0: left of a -> b = inside
        src, out = out, []
        for k in range(len(src)):
            p, q = src[k], src[(k + 1) % len(src)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return []
    return out


def _area(poly, T=float):
    if len(poly) < 3:
        return T(0)
    acc = T(0)
    for k in range(len(poly)):
        p, q = poly[k], poly[(k + 1) % len(poly)]
        acc = acc + (p[0] * q[1] - q[0] * p[1])
    return T(0.5) * abs(acc)


def iou_pair(a, b, T=float):
    """IoU of two (x, y, w, l, yaw) boxes in ABSOLUTE coordinates, arithmetic in T (float = fp64, the oracle;
    numpy.float32 = the crudest fp32 evaluation); 0 when the union is not positive."""
    inter = _area(_clip_convex(corners(a, T), corners(b, T)), T)
    union = T(a[2]) * T(a[3]) + T(b[2]) * T(b[3]) - inter
    return float(inter / union) if union > 0 else 0.0


def iou_matrix(a, b=None, rows=None):
    """fp64 IoU [M, N] of boxes a [M, 5] and b [N, 5] (b = None: a against itself, evaluated once per pair).  Pairs
    whose circumcircles are apart are 0 without clipping.  rows: only these rows of the matrix are evaluated."""
    a = np.asarray(a, np.float64)
    same = b is None
    b = a if same else np.asarray(b, np.float64)
    out = np.zeros((a.shape[0], b.shape[0]), np.float64)
    ra, rb = 0.5 * np.hypot(a[:, 2], a[:, 3]), 0.5 * np.hypot(b[:, 2], b[:, 3])
    d2 = (a[:, None, 0] - b[None, :, 0]) ** 2 + (a[:, None, 1] - b[None, :, 1]) ** 2
    near = d2 <= ((ra[:, None] + rb[None, :]) * (1 + 1e-9)) ** 2
    if rows is not None:
        pick = np.zeros(a.shape[0], bool)
        pick[np.asarray(rows)] = True
        near &= pick[:, None]
    for i, j in zip(*np.nonzero(near)):
        if same and rows is None and j < i:
            continue
        out[i, j] = iou_pair(a[i], b[j])
        if same and rows is None:
            out[j, i] = out[i, j]
    return out


def closed_form_checks(iou=iou_pair, tol=1e-12):
    """The IoU function against cases whose answer is known in closed form."""
    A = [3.0, -2.0, 4.0, 2.0, 0.7]
    assert abs(iou(A, A) - 1.0) <= tol
    assert iou(A, [30.0, 5.0, 4.0, 2.0, 0.1]) == 0.0
    for dx, dy in ((1.0, 0.0), (0.5, 0.25), (3.9, 1.9), (4.5, 0.0)):          # axis-aligned: interval formula
        P, Q = [0.0, 0.0, 4.0, 2.0, 0.0], [dx, dy, 4.0, 2.0, 0.0]
        inter = max(0.0, 4.0 - abs(dx)) * max(0.0, 2.0 - abs(dy))
        assert abs(iou(P, Q) - inter / (16.0 - inter)) <= tol, (dx, dy)
    big, small = [1.0, 1.0, 6.0, 4.0, 0.4], [1.2, 0.9, 1.0, 0.5, 1.1]         # inside: area ratio
    assert abs(iou(big, small) - 0.5 / 24.0) <= tol
    B = [3.5, -1.5, 3.0, 1.5, -0.4]
    ref = iou(A, B)
    assert 0.05 < ref < 0.95
    assert abs(iou(A, [B[0], B[1], B[2], B[3], B[4] + math.pi]) - ref) <= 1e-12              # yaw + pi
    assert abs(iou(A, [B[0], B[1], B[3], B[2], B[4] + math.pi / 2]) - ref) <= 1e-12          # w <-> l, yaw + pi / 2
    assert abs(iou(B, A) - ref) <= 1e-12                                                     # symmetry
    sh = lambda q: [q[0] + 41.5, q[1] - 17.25] + list(q[2:])
    assert abs(iou(sh(A), sh(B)) - ref) <= 1e-12                                             # translation


def point_count_iou(a, b, n=2000):
    """IoU by counting the points of an n x n grid over the bounding box of both; returns (iou, resolution)."""
    allc = np.array(corners(a) + corners(b), np.float64)
    lo, hi = allc.min(0), allc.max(0)
    xs = lo[0] + (np.arange(n) + 0.5) * (hi[0] - lo[0]) / n
    ys = lo[1] + (np.arange(n) + 0.5) * (hi[1] - lo[1]) / n
    X, Y = np.meshgrid(xs, ys)

    def inside(box):
        x, y, w, l, r = (float(v) for v in box)
        c, s = math.cos(r), math.sin(r)
        u, v = (X - x) * c + (Y - y) * s, (Y - y) * c - (X - x) * s
        return (np.abs(u) <= 0.5 * w) & (np.abs(v) <= 0.5 * l)

    ia, ib = inside(a), inside(b)
    inter, union = (ia & ib).sum(), (ia | ib).sum()
    # a boundary cell is mis-counted at most: perimeter / cell size cells out of `union` cells
    cell = max(hi[0] - lo[0], hi[1] - lo[1]) / n
    per = 2 * (a[2] + a[3] + b[2] + b[3])
    res = 2.0 * per / cell / max(union, 1)
    return inter / union, res


# ------------------------------------------------------------------------------------------------ scenes
def clustered_scene(rng, n, spread=50.0, neighbours=8, cell=0.8, yaw_jitter=0.1):
    """n candidate boxes [n, 9] fp32, scores [n] fp32 (pairwise distinct), labels [n] int32: objects of the nuScenes
    class sizes over +-spread m, each with ~`neighbours` near-duplicates up to one heat-map cell away -- what the top
    cells of a CenterPoint heat map look like."""
    objects = max(1, n // (neighbours + 1))
    boxes, labels = np.zeros((n, 9), np.float64), np.zeros(n, np.int32)
    centre = rng.uniform(-spread, spread, (objects, 2))
    cls = rng.integers(0, 10, objects)
    yaw = rng.uniform(-math.pi, math.pi, objects)
    z = rng.uniform(-2.0, 1.0, objects)
    for i in range(n):
        o = i % objects
        w, l, h = CLASS_SIZES[cls[o]]
        jitter = (rng.uniform(-cell, cell, 2) if i >= objects else np.zeros(2))
        boxes[i, 0:2] = centre[o] + jitter
        boxes[i, 2] = z[o] + rng.normal(0, 0.1)
        boxes[i, 3:6] = np.array([w, l, h]) * np.exp(rng.normal(0, 0.08, 3))
        boxes[i, 6] = yaw[o] + rng.normal(0, yaw_jitter)
        boxes[i, 7:9] = rng.normal(0, 2.0, 2)
        labels[i] = cls[o]
    scores = distinct_scores(rng, n)
    perm = rng.permutation(n)
    return boxes[perm].astype(np.float32), scores, labels[perm]


def distinct_scores(rng, n, lo=0.1, hi=0.95):
    s = np.unique(rng.uniform(lo, hi, 2 * n + 8).astype(np.float32))
    assert s.size >= n
    return rng.permutation(s)[:n].astype(np.float32)


def sparse_scene(rng, n, spread=50.0):
    """n small boxes on a jittered grid: no two overlap."""
    side = int(math.ceil(math.sqrt(n)))
    step = 2 * spread / side
    assert step > 1.6
    boxes, labels = np.zeros((n, 9), np.float32), rng.integers(0, 10, n).astype(np.int32)
    for i in range(n):
        boxes[i, 0] = -spread + (i % side + 0.5) * step + rng.uniform(-0.1, 0.1)
        boxes[i, 1] = -spread + (i // side + 0.5) * step + rng.uniform(-0.1, 0.1)
        boxes[i, 3:6] = (0.6, 0.9, 1.5)
        boxes[i, 6] = rng.uniform(-math.pi, math.pi)
    return boxes, distinct_scores(rng, n), labels


def factors_of(labels, factors):
    """fp32 factor per row under the rule of bevops_bev_nms."""
    f = np.ones(len(labels), np.float32)
    fac = np.asarray(factors, np.float32)
    if fac.size == 1:
        f[:] = fac[0]
    elif fac.size:
        ok = (labels >= 0) & (labels < fac.size)
        f[ok] = fac[labels[ok]]
    return f


def bev_of(boxes, labels, factors):
    """The (x, y, w f, l f, yaw) the pair test sees, fp32 [n, 5]."""
    f = factors_of(labels, factors)
    b = np.asarray(boxes, np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 3] * f, b[:, 4] * f, b[:, 6]], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ fixtures
def cases(kind):
    """The cases of tests/golden/nms_<kind>.npz: dicts with boxes [B, N, 9], scores, labels, count, the settings and,
    per item, what the reference returned (keep = kept input rows in rank order, bboxes, scores, labels)."""
    g = dict(np.load(os.path.join(GOLDEN, f"nms_{kind}.npz")))
    out = []
    for name in g["names"].tolist():
        thr, pre, post, bottom = g[f"{name}_params"].tolist()
        B = g[f"{name}_boxes"].shape[0]
        out.append(dict(name=name, kind=kind, boxes=g[f"{name}_boxes"], scores=g[f"{name}_scores"],
                        labels=g[f"{name}_labels"], count=g[f"{name}_count"], factors=g[f"{name}_factors"].tolist(),
                        threshold=thr, pre=int(pre) if pre > 0 else None, post=int(post), bottom=bool(bottom),
                        items=[{k: g[f"{name}_{k}{b}"] for k in ("keep", "bboxes", "scores", "labels")}
                               for b in range(B)]))
    return out


def kwargs_of(c):
    return dict(nms_type=c["kind"], threshold=c["threshold"], pre_max_size=c["pre"], post_max_size=c["post"],
                rescale_factor=c["factors"] if c["factors"] else None, bottom_center=c["bottom"])


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_against_fixture(c, out, what):
    """out = (boxes, scores, labels, count, index) as numpy, padded: equal to the fixture's bits, zero tail."""
    boxes, scores, labels, count, index = out
    for b, it in enumerate(c["items"]):
        n = it["keep"].shape[0]
        assert int(count[b]) == n, f"{what} {c['name']}[{b}]: count {int(count[b])}, reference {n}"
        assert np.array_equal(index[b, :n], it["keep"].astype(np.int32)), f"{what} {c['name']}[{b}]: kept rows differ"
        assert np.array_equal(labels[b, :n], it["labels"].astype(np.int32)), f"{what} {c['name']}[{b}]: labels"
        assert bits_equal(scores[b, :n], it["scores"]), f"{what} {c['name']}[{b}]: scores"
        for col in range(9):
            assert bits_equal(boxes[b, :n, col], it["bboxes"][:, col]), f"{what} {c['name']}[{b}]: box column {col}"
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any() \
            and not index[b, n:].any(), f"{what} {c['name']}[{b}]: rows behind count are not zero"


# ------------------------------------------------------------------------------------------------ invariants
def check_invariants(boxes, scores, labels, n_valid, index, count, threshold, pre, post, factors, what, slack=5e-4):
    """What any correct rotated NMS satisfies on any input (one item; numpy).  With I the fp64 IoU of the scaled
    boxes: (a) every two kept rows have I <= thr + slack, (b) every valid, in-pre_max row that is neither kept nor
    ranked after the post-th kept row has an earlier kept row with I >= thr - slack, (c) kept scores descend, ties by
    row, (d) count <= post."""
    count = int(count)
    assert 0 <= count <= post, f"{what}: count {count} above post_max_size {post}"
    kept = index[:count].astype(np.int64)
    assert len(set(kept.tolist())) == count and (kept >= 0).all() and (kept < n_valid).all(), f"{what}: kept rows invalid"
    sc = scores[:n_valid].astype(np.float32) + np.float32(0)
    order = np.argsort(-sc.astype(np.float64), kind="stable")
    if pre:
        order = order[:pre]
    rank = {int(r): k for k, r in enumerate(order)}
    assert all(int(k) in rank for k in kept), f"{what}: a kept row is outside pre_max_size"
    ranks = [rank[int(k)] for k in kept]
    assert ranks == sorted(ranks), f"{what}: kept rows are not in rank order"
    bev = bev_of(boxes[:n_valid], labels[:n_valid], factors)
    I = iou_matrix(bev[kept]) if count else np.zeros((0, 0))
    off = I - np.eye(count) * I
    assert count == 0 or off.max() <= threshold + slack, f"{what}: two kept rows overlap by {off.max()}"
    full = count == post
    last = ranks[-1] if count else -1
    kept_set = set(kept.tolist())
    lost = [int(r) for k, r in enumerate(order) if int(r) not in kept_set and not (full and k > last)]
    if lost:
        J = iou_matrix(bev[lost], bev[kept]) if count else np.zeros((len(lost), 0))
        for a, r in enumerate(lost):
            earlier = [k for k in range(count) if ranks[k] < rank[r]]
            best = max((J[a, k] for k in earlier), default=-1.0)
            assert best >= threshold - slack, f"{what}: row {r} dropped, best earlier kept IoU {best}"
    return count
