#!/usr/bin/env python3
"""Golden vectors for the detection decode, made by the REFERENCE's own coder code on the CPU in fp32:
  * NMSFreeCoder.decode_single         third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py:42-98
    (+ denormalize_bbox                third_party/bev_mmdet3d/core/bbox/util.py:26-53)
  * CenterPointBBoxCoder.decode/_topk  third_party/bev_mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py:61-230,
    fed as CenterHead.get_bboxes feeds it (models/dense_heads/centerpoint_head.py:716-746: heatmap.sigmoid(),
    exp(dim) under norm_bbox, rot split into its two channels).
mmdet is not installed, so the two classes are lifted out of their files by AST -- base class and registry decorator
dropped, nothing else touched -- as make_wrapper_golden.py lifts `forward_trt`.

Run in the build container only (needs the reference tree, see make_golden.py); the .npz files are committed:
    python tests/golden/make_decode_golden.py

The generator ASSERTS, for every case and batch item, what makes the reference alone define the answer:
  * the first max_num + 1 sorted scores are pairwise distinct as fp32 (torch.topk's order among equals is unspecified);
  * no selected candidate has a score within 1e-4 of a score threshold in force, nor a centre coordinate within 1e-3
    of a post_center_range bound;
  * some candidates are kept and some dropped: at least one selected candidate fails the range mask and, where a
    threshold is in force, at least one fails it (the "keep all" case excepted: its relaxed threshold drops nothing
    by definition);
  * `nf_relax` runs the relaxation loop at least twice, `nf_keepall` ends in "keep all".
"""
import ast
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import REF  # noqa: E402

RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]          # configs/bevformer/bevformer_base.py:168
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def lift_function(path, name):
    for node in ast.parse(open(os.path.join(REF, path)).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            ns = {"torch": torch}
            exec(compile(ast.unparse(node), path, "exec"), ns)
            print(f"  lifted {name} at {path}:{node.lineno}-{node.end_lineno}")
            return ns[name]
    raise KeyError((path, name))


def lift_class(path, name, ns):
    for node in ast.parse(open(os.path.join(REF, path)).read()).body:
        if isinstance(node, ast.ClassDef) and node.name == name:
            node.bases, node.decorator_list = [], []
            ns = dict(ns, torch=torch, np=np)
            exec(compile(ast.unparse(node), path, "exec"), ns)
            print(f"  lifted class {name} at {path}:{node.lineno}-{node.end_lineno}")
            return ns[name]
    raise KeyError((path, name))


def check_distinct(scores_flat, max_num, what):
    s = torch.sort(scores_flat, descending=True).values[:max_num + 1]
    gap = (s[:-1] - s[1:]).min().item() if s.numel() > 1 else float("inf")
    assert gap > 0, f"{what}: equal scores among the first {max_num + 1}"
    return gap


def check_margins(centres, bounds, what):
    r = torch.tensor(bounds, dtype=torch.float32)
    d = torch.minimum((centres - r[:3]).abs(), (centres - r[3:]).abs()).min().item()
    assert d > 1e-3, f"{what}: a centre {d} from a post_center_range bound"


# name: (batch, num_query, num_classes, max_num, score_threshold, logit shift, logit scale)
NF_CASES = {
    "nf_base": (1, 900, 10, 300, None, 0.0, 1.0),        # bevformer_base.py:166-173
    "nf_thr_b2": (2, 300, 10, 100, 0.93, 0.0, 1.0),      # plain threshold: some of the top 100 fail it
    "nf_all": (1, 50, 3, 150, None, 0.0, 1.0),           # max_num = every candidate
    "nf_relax": (1, 300, 10, 100, 0.8, -3.5, 1.0),       # top score ~0.45: 0.72, 0.648, 0.583, 0.525, 0.472, 0.425
    "nf_keepall": (1, 50, 3, 150, 0.3, -9.0, 0.5),       # every score < 0.01: ends in "keep all"
}


def relaxation(scores, thr):
    """(threshold in force, operator, rounds) as nms_free_coder.py:67-75 walks them."""
    if (scores > thr).sum() > 0:
        return thr, ">", 0
    tmp, rounds = thr, 0
    while True:
        tmp *= 0.9
        rounds += 1
        if tmp < 0.01:
            return None, "all", rounds
        if (scores >= tmp).sum() > 0:
            return tmp, ">=", rounds


def make_nms_free():
    denorm = lift_function("third_party/bev_mmdet3d/core/bbox/util.py", "denormalize_bbox")
    Coder = lift_class("third_party/bev_mmdet3d/core/bbox/coders/nms_free_coder.py", "NMSFreeCoder",
                       {"denormalize_bbox": denorm})
    res = {"names": np.array(list(NF_CASES))}
    for ci, (name, (B, nq, nc, K, thr, shift, scale)) in enumerate(NF_CASES.items()):
        seed = 100 + ci
        while True:     # re-seed until the conditions hold
            g = torch.Generator().manual_seed(seed)
            cls = torch.randn(B, nq, nc, generator=g) * scale + shift
            box = torch.randn(B, nq, 10, generator=g)
            box[..., 0:2] = (torch.rand(B, nq, 2, generator=g) * 2 - 1) * 70.0      # cx, cy: some outside +-61.2
            box[..., 4] = (torch.rand(B, nq, generator=g) * 2 - 1) * 12.0          # cz: some outside +-10
            box[..., [2, 3, 5]] *= 0.5                                              # log sizes
            try:
                outs = []
                for b in range(B):
                    coder = Coder(PC_RANGE, voxel_size=[0.512, 0.512, 8], post_center_range=list(RANGE), max_num=K,
                                  score_threshold=thr, num_classes=nc)
                    scores_all = cls[b].sigmoid().view(-1)
                    gap = check_distinct(scores_all, min(K, nq * nc - 1), name)
                    top, index = scores_all.topk(K)        # the call decode_single makes
                    centres = box[b][torch.div(index, nc, rounding_mode="trunc")][:, [0, 1, 4]]
                    check_margins(centres, RANGE, name)
                    r = torch.tensor(RANGE)
                    in_range = ((centres >= r[:3]).all(1) & (centres <= r[3:]).all(1))
                    assert 0 < in_range.sum() < K, f"{name}: the range mask keeps all or none"
                    rounds = 0
                    if thr is not None:
                        eff, op, rounds = relaxation(top, thr)
                        if eff is not None:
                            assert (top - eff).abs().min() > 1e-4, f"{name}: a score within 1e-4 of {eff}"
                            assert (top < eff).sum() > 0, f"{name}: nothing fails the threshold"
                        if name == "nf_relax":
                            assert op == ">=" and rounds >= 2, (op, rounds)
                        if name == "nf_keepall":
                            assert op == "all", op
                        if name == "nf_thr_b2":
                            assert op == ">", op
                    d = coder.decode_single(cls[b].clone(), box[b].clone())
                    assert 0 < d["scores"].numel() < K
                    outs.append((d, index, gap, rounds))
                break
            except AssertionError as e:
                print(f"  {name}: seed {seed} rejected ({e})")
                seed += 1000
        res[f"{name}_cls"], res[f"{name}_box"] = cls.numpy(), box.numpy()
        res[f"{name}_params"] = np.array([K, -1.0 if thr is None else thr], np.float64)
        for b, (d, index, gap, rounds) in enumerate(outs):
            res[f"{name}_bboxes{b}"], res[f"{name}_scores{b}"] = d["bboxes"].numpy(), d["scores"].numpy()
            res[f"{name}_labels{b}"], res[f"{name}_index{b}"] = d["labels"].numpy(), index.numpy()
            print(f"  {name}[{b}]: seed {seed}, kept {d['scores'].numel()} of {K}, smallest score gap {gap:.3g}, "
                  f"relaxation rounds {rounds}")
    path = os.path.join(OUT, "decode_nms_free.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


# name: (batch, classes, H, W, max_num, threshold, with vel, with reg, out_size_factor, voxel, pc)
CP_CASES = {
    "cp_r50": (1, 10, 128, 128, 500, 0.1, True, True, 8, [0.1, 0.1], [-51.2, -51.2]),     # bevdet-r50-cbgs.py:138-147
    "cp_small_b2": (2, 3, 20, 24, 40, 0.25, True, True, 4, [0.2, 0.25], [-10.0, -12.0]),
    "cp_novel": (1, 3, 20, 24, 40, None, False, True, 4, [0.2, 0.25], [-10.0, -12.0]),
    "cp_noreg": (1, 3, 20, 24, 40, 0.25, True, False, 4, [0.2, 0.25], [-10.0, -12.0]),
}


def half_values(t):
    """Values an fp16 holds exactly: these maps are committed as fp16 (half the bytes) and widened by the tests."""
    return t.half().float()


def make_centerpoint():
    Coder = lift_class("third_party/bev_mmdet3d/core/bbox/coders/centerpoint_bbox_coders.py", "CenterPointBBoxCoder", {})
    res = {"names": np.array(list(CP_CASES))}
    for ci, (name, (B, nc, H, W, K, thr, with_vel, with_reg, osf, voxel, pc)) in enumerate(CP_CASES.items()):
        seed = 200 + ci
        rng = [pc[0] - 2.0, pc[1] - 2.0, -10.0, -pc[0] + 2.0, -pc[1] + 2.0, 10.0] if name != "cp_r50" else list(RANGE)
        while True:
            g = torch.Generator().manual_seed(seed)
            # heat map: fp32 logits around CenterHead's init bias region so that the threshold splits the top max_num
            heat = torch.randn(B, nc, H, W, generator=g) + (-5.2 if name == "cp_r50" else -3.2)
            reg = half_values(torch.rand(B, 2, H, W, generator=g) * 6 - 2.5) if with_reg else None
            hei = half_values(torch.randn(B, 1, H, W, generator=g) * 6.0)        # some outside +-10
            dim = half_values(torch.randn(B, 3, H, W, generator=g) * 0.5)
            rot = half_values(torch.randn(B, 2, H, W, generator=g))
            vel = half_values(torch.randn(B, 2, H, W, generator=g)) if with_vel else None
            try:
                coder = Coder(pc, osf, voxel, post_center_range=list(rng), max_num=K, score_threshold=thr)
                # CenterHead.get_bboxes, centerpoint_head.py:716-746 (norm_bbox = True)
                batch_heatmap = heat.sigmoid()
                batch_dim = torch.exp(dim)
                batch_rots, batch_rotc = rot[:, 0].unsqueeze(1), rot[:, 1].unsqueeze(1)
                score, inds, clses, ys, xs = coder._topk(batch_heatmap, K=K)
                index = clses.long() * (H * W) + inds
                out = coder.decode(batch_heatmap, batch_rots, batch_rotc, hei, batch_dim, vel, reg=reg, task_id=0)
                gaps = []
                for b in range(B):
                    gaps.append(check_distinct(batch_heatmap[b].reshape(-1), K, name))
                    # the two-stage top-k equals the global one
                    assert torch.equal(score[b], batch_heatmap[b].reshape(-1).topk(K).values)
                    if thr is not None:
                        assert (score[b] - thr).abs().min() > 1e-4, f"{name}: a score within 1e-4 of {thr}"
                        assert 0 < (score[b] > thr).sum() < K, f"{name}: the threshold keeps all or none"
                    cell = inds[b]
                    rx = reg[b, 0].reshape(-1)[cell] if with_reg else 0.5
                    ry = reg[b, 1].reshape(-1)[cell] if with_reg else 0.5
                    cx = (xs[b] + rx) * osf * voxel[0] + pc[0]
                    cy = (ys[b] + ry) * osf * voxel[1] + pc[1]
                    centres = torch.stack([cx, cy, hei[b, 0].reshape(-1)[cell]], 1)
                    check_margins(centres, rng, name)
                    r = torch.tensor(rng)
                    in_range = ((centres >= r[:3]).all(1) & (centres <= r[3:]).all(1))
                    assert 0 < in_range.sum() < K, f"{name}: the range mask keeps all or none"
                    assert 0 < out[b]["scores"].numel() < K
                break
            except AssertionError as e:
                print(f"  {name}: seed {seed} rejected ({e})")
                seed += 1000
        res[f"{name}_heat"] = heat.numpy()
        for key, t in (("reg", reg), ("height", hei), ("dim", dim), ("rot", rot), ("vel", vel)):
            if t is not None:
                assert torch.equal(t.half().float(), t)
                res[f"{name}_{key}"] = t.half().numpy()
        res[f"{name}_params"] = np.array([K, -1.0 if thr is None else thr, osf] + voxel + pc + rng, np.float64)
        for b in range(B):
            d = out[b]
            res[f"{name}_bboxes{b}"], res[f"{name}_scores{b}"] = d["bboxes"].numpy(), d["scores"].numpy()
            res[f"{name}_labels{b}"], res[f"{name}_index{b}"] = d["labels"].numpy(), index[b].numpy()
            print(f"  {name}[{b}]: seed {seed}, kept {d['scores'].numel()} of {K}, smallest score gap {gaps[b]:.3g}")
    path = os.path.join(OUT, "decode_centerpoint.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "fixture above the repository's 1 MiB limit"


if __name__ == "__main__":
    torch.set_num_threads(1)
    make_nms_free()
    make_centerpoint()
