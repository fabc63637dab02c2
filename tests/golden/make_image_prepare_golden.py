#!/usr/bin/env python3
"""Golden vectors for BEVDet's camera front end, made by the REFERENCE's own Python and PIL on the CPU:
  * PrepareImageInputs.sample_augmentation (is_train=False), img_transform_core, img_transform and get_rot
    (third_party/bev_mmdet3d/datasets/pipelines/loading.py:722-792), lifted by AST and called with a three-line
    stand-in for `self` (data_config, is_train);
  * the 3 x 3 embedding of get_inputs (loading.py:856-859), four assignments, restated here.
Stored per case (tests/util_image_prepare.py: CASES) and image kind (noise; 5-pixel 0 / 255 block checkerboard with
differing channels): the raw images, the parameters sample_augmentation returned, the canvases PIL produced, post_rot
and post_tran.

Run in the build container only (needs the reference tree and PIL); the .npz is committed:
    python tests/golden/make_image_prepare_golden.py

The generator ASSERTS, per case:
  * the geometry is the one the case table expects;
  * the numpy restatement (tests/util_image_prepare.py) equals PIL's canvas bit for bit;
  * every checkerboard canvas holds both 0 and 255 pixels, so the clip decides;
  * a vertical-first evaluation differs from PIL's result, so the pass order and the uint8 intermediate are observable.
"""
import ast
import os
import sys

import numpy as np
import torch
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
from make_golden import REF  # noqa: E402
import util_image_prepare as U  # noqa: E402

LOADING = "third_party/bev_mmdet3d/datasets/pipelines/loading.py"
CAMERAS = {"default": 2, "resize_test_flip": 1, "crop_h_scale": 2, "upscale": 3, "odd_flip": 2}


def lift_methods(names):
    body = ast.parse(open(os.path.join(REF, LOADING)).read()).body
    cls = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == "PrepareImageInputs")
    ns = {"np": np, "torch": torch, "Image": Image}
    for node in cls.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.unparse(node), LOADING, "exec"), ns)
            print(f"  lifted {node.name} at {LOADING}:{node.lineno}-{node.end_lineno}")
    return ns


def main():
    ns = lift_methods(("sample_augmentation", "img_transform_core", "img_transform", "get_rot"))

    class Self:
        is_train = False
        get_rot, img_transform_core = ns["get_rot"], ns["img_transform_core"]

        def __init__(self, data_config):
            self.data_config = data_config

    res = {"names": np.array(list(U.CASES))}
    for ci, (name, ((H, W), cfg, flip, scale, expect)) in enumerate(U.CASES.items()):
        s = Self(cfg)
        resize, dims, crop, fl, rot = ns["sample_augmentation"](s, H, W, flip, scale)
        for got, want in zip((resize, tuple(dims), tuple(crop)), expect):
            assert want is None or got == want, f"{name}: geometry {resize, dims, crop}, expected {expect}"
        assert rot == 0
        assert U.ref_augmentation(H, W, cfg, flip, scale) == (resize, tuple(dims), tuple(crop), bool(fl), 0)
        n = CAMERAS[name]
        for kind in ("noise", "checker"):
            raw = U.noise(100 + ci, n, H, W) if kind == "noise" else U.checkerboard(n, H, W)
            canvas, nvf = [], 0
            for i in range(n):
                img, post_rot2, post_tran2 = ns["img_transform"](s, Image.fromarray(raw[i]), torch.eye(2), torch.zeros(2),
                                                                 resize=resize, resize_dims=dims, crop=crop, flip=fl,
                                                                 rotate=rot)
                want = np.array(img)
                assert want.dtype == np.uint8 and want.shape == (crop[3] - crop[1], crop[2] - crop[0], 3)
                assert np.array_equal(U.prepare(raw[i], dims, crop, fl), want), f"{name}/{kind}: restatement != PIL"
                vf = U.resize_vertical_first(raw[i], *dims)[crop[1]:crop[3], crop[0]:crop[2]]
                d = int(((vf[:, ::-1] if fl else vf) != want).sum())
                assert d > 0, f"{name}/{kind}: the pass order is not observable"
                nvf += d
                if kind == "checker":
                    assert (want == 0).any() and (want == 255).any(), f"{name}: no clipped pixel"
                canvas.append(want)
            canvas = np.stack(canvas)
            post_rot, post_tran = torch.eye(3), torch.zeros(3)          # loading.py:856-859
            post_tran[:2] = post_tran2
            post_rot[:2, :2] = post_rot2
            res[f"{name}_{kind}_raw"], res[f"{name}_{kind}_canvas"] = raw, canvas
            print(f"  {name}/{kind}: {n} x {H} x {W} -> resize {resize:.6f} dims {tuple(dims)} crop {tuple(crop)} flip {fl}: "
                  f"0s {int((canvas == 0).sum())}, 255s {int((canvas == 255).sum())}, vertical-first differs in {nvf}")
        res[f"{name}_resize"] = np.array(resize, np.float64)
        res[f"{name}_geometry"] = np.array(list(dims) + list(crop) + [int(bool(fl)), rot], np.int64)
        res[f"{name}_post_rot"], res[f"{name}_post_tran"] = post_rot.numpy(), post_tran.numpy()
    # the R50 geometry (configs/bevdet/bevdet-r50-cbgs.py:44-62): parameters and matrices only, plain and flipped
    s = Self(U.DATA_CONFIG_R50)
    for tag, flip in (("r50", None), ("r50_flip", True)):
        resize, dims, crop, fl, rot = ns["sample_augmentation"](s, 900, 1600, flip, None)
        assert (resize, tuple(dims), tuple(crop)) == (0.44, (704, 396), (0, 140, 704, 396))
        tiny = Image.fromarray(np.zeros((4, 4, 3), np.uint8))
        _, r2, t2 = ns["img_transform"](s, tiny, torch.eye(2), torch.zeros(2), resize=resize, resize_dims=(2, 2),
                                        crop=crop, flip=fl, rotate=rot)
        post_rot, post_tran = torch.eye(3), torch.zeros(3)
        post_tran[:2] = t2
        post_rot[:2, :2] = r2
        res[f"{tag}_resize"] = np.array(resize, np.float64)
        res[f"{tag}_geometry"] = np.array(list(dims) + list(crop) + [int(bool(fl)), rot], np.int64)
        res[f"{tag}_post_rot"], res[f"{tag}_post_tran"] = post_rot.numpy(), post_tran.numpy()
        print(f"  {tag}: post_rot {post_rot.tolist()} post_tran {post_tran.tolist()}")
    path = os.path.join(OUT, "image_prepare.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "fixture above the repository's 1 MiB limit"


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
