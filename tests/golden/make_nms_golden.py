#!/usr/bin/env python3
"""Golden vectors for the BEV NMS, made by the REFERENCE's own Python on the CPU:
  * CenterHead.get_task_detections   third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py:808-905
    (scale, nms_bev, divide back, gather), the method lifted by AST and called with three-line stand-ins for
    `self.test_cfg`, `self.task_heads`, `self.bbox_coder.code_size` and `img_metas[i]["box_type_3d"]` (whose `.bev`
    is the reference's own column list, core/bbox/structures/lidar_box3d.py:94);
  * nms_bev                          third_party/bev_mmdet3d/core/post_processing/box3d_nms.py:227-273;
  * circle_nms                       box3d_nms.py:182-221, its numba.jit decorator dropped (plain Python), called as
    CenterHead.get_bboxes calls it (centerpoint_head.py:750-773);
  * the z shift of get_bboxes (centerpoint_head.py:793), one expression, restated here on the returned boxes.
The one thing the reference cannot supply is mmcv.ops.nms_rotated (a CUDA extension).  In its place nms_bev is handed
a greedy scan over an fp64 IoU matrix ("the exact overlapping area of the two boxes", box3d_nms.py:230-231) from
tests/util_nms.py, cross-checked below against closed forms.  mmcv's kernel itself was never run; the assertions
below are what makes its answer the only possible one whatever fp32 IoU it evaluates.

Run in the build container only (needs the reference tree, see make_golden.py); the .npz files are committed:
    python tests/golden/make_nms_golden.py

The generator ASSERTS, per case and item:
  * the scores of the rows that enter the scan are pairwise distinct as fp32;
  * rotate: NO pair of candidates has an fp64 IoU within 1e-3 of the threshold (all pairs, so the suppression matrix
    itself is unique).  A raw draw of 500 rows or more usually has a few such pairs, so the draw is REPAIRED: the
    lower-ranked box of such a pair is moved by a fresh jitter of a few centimetres (and its w, l by a per cent: a box
    inside another has the area ratio as IoU wherever it sits) and its row of the matrix recomputed, until none is left; the band is then asserted over all pairs of the final scene, which is stored
    already rounded to fp32;
  * rotate: an fp32 evaluation of the same clip in ABSOLUTE coordinates (the crudest plausible kernel) takes the same
    decision on every pair;
  * circle: no squared distance equals the threshold as fp32;
  * every case keeps some rows and suppresses some (the one-row case excepted: it has nothing to suppress);
    `*_postmax` is cut by post_max_size, `*_premax` by pre_max_size (rows beyond it would otherwise have survived);
  * with factors, at least one returned size differs in bits from its input ((d f) / f != d).
"""
import ast
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import REF  # noqa: E402
import util_nms as U  # noqa: E402

BAND = 1e-3
HEAD = "third_party/bev_mmdet3d/models/dense_heads/centerpoint_head.py"
NMS = "third_party/bev_mmdet3d/core/post_processing/box3d_nms.py"


def lift(path, name, ns, cls=None):
    """The function `name` (a method of class `cls` when given) of the reference file, decorators dropped."""
    body = ast.parse(open(os.path.join(REF, path)).read()).body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == name)
    node.decorator_list = []
    ns = dict(ns)
    exec(compile(ast.unparse(node), path, "exec"), ns)
    print(f"  lifted {name} at {path}:{node.lineno}-{node.end_lineno}")
    return ns[name]


def nms_rotated_fp64(boxes, scores, thresh):
    """Stand-in for mmcv.ops.nms_rotated(boxes [n, 5] xywhr, scores, iou_threshold) -> (dets, keep): greedy scan in
    descending score order, row j suppressed by an earlier kept row i when the fp64 IoU(i, j) > thresh."""
    order = torch.sort(scores, descending=True, stable=True).indices
    I = U.iou_matrix(boxes[order].numpy())
    removed, keep = np.zeros(len(order), bool), []
    for i in range(len(order)):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= I[i, i + 1:] > thresh
    keep = order[torch.tensor(keep, dtype=torch.long)]
    return torch.cat([boxes[keep], scores[keep, None]], 1), keep


class Box3D:                    # stand-in for LiDARInstance3DBoxes: the tensor and the reference's `.bev` columns
    def __init__(self, tensor, box_dim):
        self.tensor = tensor
    bev = property(lambda self: self.tensor[:, [0, 1, 3, 4, 6]])          # lidar_box3d.py:94


class Head:                     # stand-in for the `self` of CenterHead.get_task_detections
    task_heads = [None]
    bbox_coder = type("Coder", (), {"code_size": 9})

    def __init__(self, test_cfg):
        self.test_cfg = test_cfg


def repair(rng, boxes, scores, labels, factors, thr, pre):
    """Move boxes until no candidate pair has an fp64 IoU within BAND of thr.  Returns the number of moves."""
    order = np.argsort(-scores.astype(np.float64), kind="stable")[:pre]
    rank = np.full(len(scores), len(scores), np.int64)
    rank[order] = np.arange(len(order))
    I = U.iou_matrix(U.bev_of(boxes[order], labels[order], factors))
    moves = 0
    while True:
        bad = np.argwhere(np.triu(np.abs(I - thr) < BAND, 1))
        if len(bad) == 0:
            return moves
        for i, j in bad:
            if abs(I[i, j] - thr) >= BAND:
                continue            # already cured by an earlier move of this round
            lo = max(i, j)          # the lower-ranked of the two
            boxes[order[lo], 0:2] += rng.uniform(-0.04, 0.04, 2).astype(np.float32)
            # (a box inside another has IoU = the area ratio wherever it sits: move the sizes by a per cent too)
            boxes[order[lo], 3:5] *= np.exp(rng.normal(0, 0.01, 2)).astype(np.float32)
            row = U.iou_matrix(U.bev_of(boxes[order], labels[order], factors), rows=[lo])[lo]
            I[lo, :], I[:, lo] = row, row
            moves += 1
        assert moves < 2000, "repair does not converge"


def check_rotate(boxes, scores, labels, factors, thr, pre, what):
    order = np.argsort(-scores.astype(np.float64), kind="stable")[:pre]
    s = scores[order]
    assert np.unique(s).size == s.size, f"{what}: equal scores"
    bev = U.bev_of(boxes[order], labels[order], factors)
    I = U.iou_matrix(bev)
    iu = np.triu_indices(len(order), 1)
    gap = np.abs(I[iu] - thr).min() if len(iu[0]) else np.inf
    assert gap >= BAND, f"{what}: a pair {gap} from the threshold"
    n_over, flips = 0, 0
    for i, j in zip(*np.nonzero(np.triu(I > 0, 1))):
        n_over += 1
        flips += (U.iou_pair(bev[i], bev[j], np.float32) > thr) != (I[i, j] > thr)
    assert flips == 0, f"{what}: the fp32 absolute-coordinate clip decides {flips} pairs differently"
    return gap, n_over, int((I[iu] > thr).sum())


# name: (batch, N, counts, factors, thr, pre, post, scene seed)
ROTATE = {
    "rot_r50": (1, 500, [500], U.R50_FACTORS, 0.2, 1000, 500, 1),          # bevdet-r50-cbgs.py:172-182
    "rot_b2": (2, 500, [420, 137], U.R50_FACTORS, 0.2, 1000, 500, 2),      # garbage behind the counts
    "rot_n1": (1, 1, [1], U.R50_FACTORS, 0.2, 1000, 1, 3),
    "rot_n63": (1, 63, [63], U.R50_FACTORS, 0.2, 1000, 63, 4),
    "rot_n64": (1, 64, [64], U.R50_FACTORS, 0.2, 1000, 64, 5),
    "rot_n65": (1, 65, [65], U.R50_FACTORS, 0.2, 1000, 65, 6),
    "rot_n1000": (1, 1000, [1000], U.R50_FACTORS, 0.2, 1000, 500, 7),
    "rot_scalar": (1, 300, [300], [0.7], 0.2, 1000, 300, 8),
    "rot_nofactor": (1, 300, [300], [], 0.2, 1000, 300, 9),
    "rot_thr": (1, 300, [300], U.R50_FACTORS, 0.45, 1000, 300, 10),
    "rot_postmax": (1, 500, [500], U.R50_FACTORS, 0.2, 1000, 60, 11),
    "rot_premax": (1, 1300, [1300], U.R50_FACTORS, 0.2, 1000, 500, 12),
}


def garbage(rng, shape):
    g = rng.normal(0, 1e6, shape).astype(np.float32)
    g.reshape(-1)[::3] = np.nan
    return g


def make_rotate():
    ns = {"torch": torch, "nms_rotated": nms_rotated_fp64}
    nms_bev = lift(NMS, "nms_bev", ns)
    task = lift(HEAD, "get_task_detections", dict(ns, nms_bev=nms_bev), cls="CenterHead")
    res = {"names": np.array(list(ROTATE))}
    for name, (B, N, counts, factors, thr, pre, post, seed) in ROTATE.items():
        rng = np.random.default_rng(seed)
        boxes, scores = garbage(rng, (B, N, 9)), garbage(rng, (B, N))
        labels = rng.integers(-5, 50, (B, N)).astype(np.int32)
        cfg = dict(nms_thr=thr, pre_max_size=pre, post_max_size=post)
        if factors:
            cfg["nms_rescale_factor"] = [list(factors) if len(factors) > 1 else factors[0]]
        for b, n in enumerate(counts):
            bx, sc, lb = U.clustered_scene(rng, n)
            moves = repair(rng, bx, sc, lb, factors, thr, pre)
            gap, n_over, n_above = check_rotate(bx, sc, lb, factors, thr, pre, f"{name}[{b}]")
            boxes[b, :n], scores[b, :n], labels[b, :n] = bx, sc, lb
            t = lambda a: torch.from_numpy(a.copy())
            det = task(Head(cfg), [t(sc)], [t(bx)], [t(lb).float()], [{"box_type_3d": Box3D}], 0)[0]
            out = det["bboxes"].clone()
            out[:, 2] = out[:, 2] - out[:, 5] * 0.5                                     # centerpoint_head.py:793
            keep = nms_bev(t(U.bev_of(bx, lb, factors)), t(sc), thresh=thr, pre_max_size=pre, post_max_size=post,
                           xyxyr2xywhr=False)
            k = keep.numel()
            assert k == det["scores"].numel() and torch.equal(det["scores"], t(sc)[keep]), f"{name}: keep mismatch"
            assert torch.equal(det["labels"], t(lb).long()[keep])
            if n > 1:
                assert 0 < k < min(n, pre), f"{name}[{b}]: keeps all or none ({k} of {n})"
            for col in U.COPIED:
                assert U.bits_equal(out[:, col].numpy(), bx[keep.numpy(), col])
            if factors:
                differs = int((out[:, 3:6].numpy().view(np.uint32) != bx[keep.numpy(), 3:6].view(np.uint32)).sum())
                assert differs > 0 or n == 1, f"{name}[{b}]: the divide-back returns every size unchanged"
            else:
                differs = 0
                assert U.bits_equal(out[:, 3:6].numpy(), bx[keep.numpy(), 3:6])
            if name.endswith("postmax") or name.endswith("premax"):
                free = nms_bev(t(U.bev_of(bx, lb, factors)), t(sc), thresh=thr, pre_max_size=None, post_max_size=None,
                               xyxyr2xywhr=False)
                order = np.argsort(-sc.astype(np.float64), kind="stable")
                if name.endswith("postmax"):
                    assert k == post < free.numel(), f"{name}: not cut by post_max_size"
                else:
                    beyond = set(order[pre:].tolist())
                    assert any(int(r) in beyond for r in free.tolist()), f"{name}: no survivor beyond pre_max_size"
                    assert k < post
            res[f"{name}_keep{b}"], res[f"{name}_bboxes{b}"] = keep.numpy(), out.numpy()
            res[f"{name}_scores{b}"], res[f"{name}_labels{b}"] = det["scores"].numpy(), det["labels"].numpy()
            print(f"  {name}[{b}]: {n} rows, {n_over} overlapping pairs, {n_above} above {thr}, {moves} repair moves, "
                  f"nearest pair {gap:.2e} from the threshold, kept {k}, sizes changed by the divide-back {differs}")
        res[f"{name}_boxes"], res[f"{name}_scores"], res[f"{name}_labels"] = boxes, scores, labels
        res[f"{name}_count"] = np.array(counts, np.int32)
        res[f"{name}_factors"] = np.array(factors, np.float64)
        res[f"{name}_params"] = np.array([thr, pre, post, 1], np.float64)
    save("nms_rotate.npz", res)


def make_circle():
    circle = lift(NMS, "circle_nms", {"np": np})
    res, names = {}, []
    rng = np.random.default_rng(40)
    for ri, radius in enumerate(U.R50_MIN_RADIUS):
        for post in (83, 500):
            name = f"cir_r{ri}_p{post}"
            names.append(name)
            n = 500
            while True:
                bx, sc, lb = U.clustered_scene(rng, n, spread=50.0 if post == 83 else 120.0, neighbours=4, cell=1.5)
                x, y = bx[:, 0], bx[:, 1]
                d = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
                assert d.dtype == np.float32
                if not (d == np.float32(radius)).any():
                    break
            assert np.unique(sc).size == n
            # CenterHead.get_bboxes, centerpoint_head.py:756-766
            dets = np.concatenate([bx[:, [0, 1]], sc.reshape(-1, 1)], 1)
            keep = np.array(circle(dets, radius, post_max_size=post), np.int64)
            k = len(keep)
            assert 0 < k < n, f"{name}: keeps all or none"
            out = torch.from_numpy(bx[keep].copy())
            out[:, 2] = out[:, 2] - out[:, 5] * 0.5                                     # centerpoint_head.py:793
            res[f"{name}_boxes"], res[f"{name}_scores"], res[f"{name}_labels"] = bx[None], sc[None], lb[None]
            res[f"{name}_count"], res[f"{name}_factors"] = np.array([n], np.int32), np.zeros(0, np.float64)
            res[f"{name}_params"] = np.array([radius, -1, post, 1], np.float64)
            res[f"{name}_keep0"], res[f"{name}_bboxes0"] = keep, out.numpy()
            res[f"{name}_scores0"], res[f"{name}_labels0"] = sc[keep], lb[keep].astype(np.int64)
            print(f"  {name}: {n} rows, min_radius {radius}, kept {k} (post_max_size {post})")
    res["names"] = np.array(names)
    save("nms_circle.npz", res)


def save(fname, res):
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "fixture above the repository's 1 MiB limit"


if __name__ == "__main__":
    torch.set_num_threads(1)
    U.closed_form_checks()
    for a, b in (([3.0, -2.0, 4.0, 2.0, 0.7], [3.5, -1.5, 3.0, 1.5, -0.4]),):
        pc, res_ = U.point_count_iou(a, b)
        assert abs(pc - U.iou_pair(a, b)) <= res_
    make_rotate()
    make_circle()
