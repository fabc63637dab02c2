#!/usr/bin/env python3
"""Golden vectors for the BEVFormer tiny / small camera front end, made by the REFERENCE's own Python on the CPU:
RandomScaleImageMultiViewImage.__call__ (third_party/bev_mmdet3d/datasets/pipelines/transform_3d.py:404-438), lifted by
AST and called with a stand-in for `self` (scales) and an `mmcv` stand-in whose `imresize` only RECORDS the size it was
asked for and returns the image unchanged.

Stored: six realistic float64 lidar2img matrices; for the scales 0.5 (tiny) and 0.8 (small) the float64 products
`scale_factor @ l2i` the reference computed and their float32 casts (tools/bevformer/evaluate_trt.py:99,131-132); for
900 x 1600, 45 x 70 and 37 x 53 images the (x_size, y_size) the reference requested from mmcv.imresize.

NO PIXEL FIXTURE can come from the reference: the resize itself is mmcv.imresize = cv2.resize, and neither mmcv nor cv2
is installed.  The pixel contract is the restatement in tests/util_image_scale.py (parity against cv2 unpinned,
design/image_scale.md).

Run in the build container only (needs the reference tree); the .npz is committed:
    python tests/golden/make_image_scale_golden.py

The generator ASSERTS that tests/util_image_scale.py's scale_lidar2img and scaled_size equal what the reference computed
bit for bit, and that a float32-by-float32 product would NOT at 0.8 (the float64 rule is observable).
"""
import ast
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import REF  # noqa: E402
import util_image_scale as U  # noqa: E402

TRANSFORM = "third_party/bev_mmdet3d/datasets/pipelines/transform_3d.py"
SIZES = ((900, 1600), (45, 70), (37, 53))
SCALES = (0.5, 0.8)


def lift_call(requests):
    body = ast.parse(open(os.path.join(REF, TRANSFORM)).read()).body
    cls = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == "RandomScaleImageMultiViewImage")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__call__")

    def imresize(img, size, return_scale=False):
        requests.append(tuple(size))
        return img

    ns = {"np": np, "mmcv": types.SimpleNamespace(imresize=imresize)}
    exec(compile(ast.unparse(fn), TRANSFORM, "exec"), ns)
    print(f"  lifted RandomScaleImageMultiViewImage.__call__ at {TRANSFORM}:{fn.lineno}-{fn.end_lineno}")
    return ns["__call__"]


def main():
    requests = []
    call = lift_call(requests)
    l2i = U.realistic_lidar2img(0)
    res = {"lidar2img": l2i, "scales": np.array(SCALES), "sizes": np.array(SIZES, np.int64)}
    for s in SCALES:
        tag = f"s{int(s * 10):02d}"
        self = types.SimpleNamespace(scales=[s])
        imgs = [np.zeros(hw + (3,), np.float32) for hw in SIZES]
        del requests[:]
        results = call(self, {"img": imgs[:1] * 6, "lidar2img": [m for m in l2i]})
        prod64 = np.stack(results["lidar2img"])
        assert prod64.dtype == np.float64 and prod64.shape == (6, 4, 4)
        prod32 = prod64.astype(np.float32)
        assert np.array_equal(U.scale_lidar2img(l2i, s).view(np.uint32), prod32.view(np.uint32))
        naive = (l2i.astype(np.float32)[:, :2] * np.float32(s)).astype(np.float32)
        differ = int((naive != prod32[:, :2]).sum())
        assert (differ > 0) == (s == 0.8), (s, differ)
        del requests[:]
        call(self, {"img": imgs, "lidar2img": [l2i[0]] * len(imgs)})
        req = np.array(requests, np.int64)                      # (x_size, y_size) per image
        for (h, w), (xs, ys) in zip(SIZES, req):
            assert U.scaled_size(h, w, s) == (ys, xs)
        res[f"{tag}_prod64"], res[f"{tag}_prod32"], res[f"{tag}_requested"] = prod64, prod32, req
        print(f"  scale {s}: requested {req.tolist()}; a float32 product differs in {differ} of 48 scaled entries")
    path = os.path.join(OUT, "image_scale.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < (1 << 20), "fixture above the repository's 1 MiB limit"


if __name__ == "__main__":
    main()
