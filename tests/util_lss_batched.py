"""Shared by the tests of the batched BEVDet index build (tests/golden/lss_prepare_batched.npz, recorded by
tests/golden/make_lss_prepare_batched_golden.py from the reference's own view-transformer methods at B > 1)."""
import ctypes

import numpy as np
import torch

from conftest import golden
from util_lss import check_arrays, digest, view_for   # noqa: F401  (the same checks, the same fixture keys)


def fixture():
    g = golden("lss_prepare_batched")
    return g, [str(c) for c in g["cases"]]


def inputs(g, case):
    t = lambda k: torch.from_numpy(g[f"{case}.{k}"])
    return t("sensor2ego"), None, t("cam2imgs"), t("post_rots"), t("post_trans"), t("bda")


def tiny_view(d, h, w, cells_xyz, span=40.0, depth_step=9.0, z=(-5.0, 3.0)):
    """An LSSViewTransformer with a (d, h, w) frustum (a 16 h x 16 w image, depths 1, 1 + depth_step, ...) and an
    (nx, ny, nz) grid reaching `span` metres to each side of the rig: the smallest shapes of the GPU tests."""
    from bevformer_tensorrt_amd.bevdet import LSSViewTransformer
    nx, ny, nz = cells_xyz
    grid = dict(x=[-span, span, 2 * span / nx], y=[-span, span, 2 * span / ny], z=[z[0], z[1], (z[1] - z[0]) / nz],
                depth=[1.0, 1.0 + d * depth_step - 0.5 * depth_step, depth_step])
    vt = LSSViewTransformer(grid_config=grid, input_size=(16 * h, 16 * w), downsample=16, in_channels=8, out_channels=8,
                            ops=object())
    assert tuple(vt.frustum.shape) == (d, h, w, 3)
    # the sizes as exact integers (a quotient such as 80 / (80 / 127) need not round to one)
    vt.grid_size = torch.tensor([float(nx), float(ny), float(nz)])
    return vt


def grid9(vt):
    return (ctypes.c_float * 9)(*[float(v) for t in (vt.grid_lower_bound, vt.grid_interval, vt.grid_size) for v in t])


def cells_of(vt):
    return int(vt.grid_size[0]) * int(vt.grid_size[1]) * int(vt.grid_size[2])


def compose(per_sample, cells, n_cams, dhw, hw):
    """The batched arrays from per-sample trimmed arrays [(rb, rd, rf, st, ln) or None (nothing kept)], numpy int32:
    ranks_bev + b cells, ranks_depth + b n dhw, ranks_feat + b n hw, interval_starts + the running point count."""
    out, at = [[] for _ in range(5)], 0
    for b, r in enumerate(per_sample):
        if r is None:
            continue
        rb, rd, rf, st, ln = r
        for dst, a in zip(out, (rb + b * cells, rd + b * n_cams * dhw, rf + b * n_cams * hw, st + at, ln)):
            dst.append(a.astype(np.int32))
        at += rb.size
    return [np.concatenate(p) if p else np.zeros(0, np.int32) for p in out]
