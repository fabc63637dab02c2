#!/usr/bin/env python3
"""Fixture of the BATCHED device index build of BEVDet's view transformer (bevops_lss_voxel_prepare_batched,
csrc/lss_prepare.hip): tests/golden/lss_prepare_batched.npz.  Build container only (needs the reference tree):

    python tests/golden/make_lss_prepare_batched_golden.py

Same method as make_lss_prepare_golden.py: create_grid_infos, create_frustum, get_lidar_coor and
voxel_pooling_prepare_v2 are lifted from the reference's third_party/bev_mmdet3d/models/necks/view_transformer.py by
AST and EXECUTED on the CPU at B > 1, in a child interpreter under tests/conftest.py's PINNED_CPU_ENV.  The reference's
methods carry B through (a batch column in coor, ranks_bev = b (Z Y X) + cell, ranks_feat over B N H W); only its
engine fixes B = 1.  Per case the fixture holds the calibration inputs [B, N, ...], the packed calibration [B, N 24 + 9],
the grid, the counts, small samples and SHA-256 digests of coor, ranks_bev, interval_starts, interval_lengths and the
CANONICAL ranks_depth / ranks_feat (ascending inside each interval).  Data only.

The coordinates: the lifted get_lidar_coor is called once with the whole batch and once per sample.  Where the batched
call differs from the per-sample calls in the last bit, that is the CPU library's choice of a batched matmul kernel, not
the semantics (a sample's coordinates cannot depend on its neighbours in the batch): the PER-SAMPLE calls are what is
recorded, and `<case>.batched_matmul_equal` says what was seen.

Asserted while recording: the plain-order statement (lidar_coor_plain on calibration_matrices_batched) equals the
recorded lifted coordinates bit for bit; ranks_feat is (ranks_depth // (D H W)) (H W) + ranks_depth % (H W); the batched
arrays of the lifted voxel_pooling_prepare_v2 equal the composition of its per-sample arrays (ranks_bev + b cells,
ranks_depth + b N D H W, ranks_feat + b N H W, interval_starts + the running point count); the middle sample of
`empty_middle` keeps nothing.
"""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]

from make_lss_prepare_golden import R50_GRID, canonical, digest   # noqa: E402


def cases(view):
    """(name, grid, [per-sample rigs (s2e, K, post_rots, post_trans, bda)])"""
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    pick = lambda rig: [rig[0], rig[2], rig[3], rig[4], rig[5]]

    def rig(seed, n_cams=6, bda=None, far=False):
        r = pick(jittered_rig(view, seed, n_cams=n_cams))
        if bda is not None:
            r[4] = bda.view(1, 3, 3)
        if far:
            r[0] = r[0].clone()
            r[0][0, :, :3, 3] += torch.tensor([5000.0, -7000.0, 0.0])    # kilometres away: nothing lands in the grid
        return r
    eye = torch.eye(3)
    out = [("two_rigs", R50_GRID, [rig(11, bda=eye), rig(12)]),                   # identity bda | flipped, rotated bda
           ("empty_middle", R50_GRID, [rig(13), rig(14, far=True), rig(15)]),
           ("one_camera", R50_GRID, [rig(16, n_cams=1), rig(17, n_cams=1)]),
           ("two_z_cells", dict(R50_GRID, z=[-5, 3, 4]), [rig(18), rig(19)]),
           ("four_r50", R50_GRID, [rig(20), rig(21), rig(22), rig(23)])]          # B cells = 65 536: a third digit
    assert not torch.equal(out[0][2][1][4].view(3, 3), eye)
    return out


def record():
    import make_wrapper_golden as W
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, LSSViewTransformer
    path = "third_party/bev_mmdet3d/models/necks/view_transformer.py"
    fns = {n: W.lift(path, "LSSViewTransformer", n)
           for n in ("create_grid_infos", "create_frustum", "get_lidar_coor", "voxel_pooling_prepare_v2")}
    ours = LSSViewTransformer(**BEVDET_R50, ops=object())
    res, names = {}, []
    for name, grid, rigs in cases(ours):
        me = W.Stub(sid=False)
        fns["create_grid_infos"](me, **grid)
        me.frustum = fns["create_frustum"](me, grid["depth"], (256, 704), 16)
        assert torch.equal(me.frustum, ours.frustum)
        s2e, K, post_rots, post_trans, bda = (torch.cat([r[i] for r in rigs], 0) for i in range(5))
        B = s2e.shape[0]
        batched = fns["get_lidar_coor"](me, s2e, None, K, post_rots, post_trans, bda)
        singles = [fns["get_lidar_coor"](me, s2e[b:b + 1], None, K[b:b + 1], post_rots[b:b + 1], post_trans[b:b + 1],
                                         bda[b:b + 1]) for b in range(B)]
        coor = torch.cat(singles, 0).contiguous()
        same = np.array_equal(batched.numpy().view(np.int32), coor.numpy().view(np.int32))
        calib = ours.calibration_matrices_batched(s2e, None, K, post_rots, post_trans, bda)
        assert calib.shape == (B, s2e.shape[1] * 24 + 9)
        plain = ours.lidar_coor_plain(calib)
        assert plain.shape == coor.shape and np.array_equal(plain.numpy().view(np.int32), coor.numpy().view(np.int32)), name
        _, N, D, H, Wd, _ = coor.shape
        dhw, hw = D * H * Wd, H * Wd
        cells = int(me.grid_size[0]) * int(me.grid_size[1]) * int(me.grid_size[2])
        ranks = fns["voxel_pooling_prepare_v2"](me, coor)
        assert ranks[0] is not None, name
        rb, rd, rf, st, ln = (t.numpy().astype(np.int32) for t in ranks)
        assert np.array_equal(rf, (rd // dhw) * hw + rd % hw), name
        rdc = canonical(rd, st, ln)
        rfc = (rdc // dhw) * hw + rdc % hw
        # the composition of the per-sample arrays
        comp, per_sample, at = [[] for _ in range(5)], [], 0
        for b in range(B):
            r1 = fns["voxel_pooling_prepare_v2"](me, singles[b])
            if r1[0] is None:
                per_sample.append((0, 0))
                continue
            b1, d1, f1, s1, l1 = (t.numpy().astype(np.int32) for t in r1)
            d1 = canonical(d1, s1, l1)
            f1 = (d1 // dhw) * hw + d1 % hw
            for dst, a in zip(comp, (b1 + b * cells, d1 + b * N * dhw, f1 + b * N * hw, s1 + at, l1)):
                dst.append(a)
            per_sample.append((b1.size, s1.size))
            at += b1.size
        for got, parts in zip((rb, rdc, rfc, st, ln), comp):
            assert np.array_equal(got, np.concatenate(parts)), name
        if name == "empty_middle":
            assert per_sample[1] == (0, 0) and per_sample[0][0] > 0 and per_sample[2][0] > 0
        pre = name + "."
        res.update({pre + "sensor2ego": s2e.numpy(), pre + "cam2imgs": K.numpy(), pre + "post_rots": post_rots.numpy(),
                    pre + "post_trans": post_trans.numpy(), pre + "bda": bda.numpy(), pre + "calib": calib.numpy(),
                    pre + "grid": np.stack([me.grid_lower_bound.numpy(), me.grid_interval.numpy(), me.grid_size.numpy()]),
                    pre + "batched_matmul_equal": np.array(same),
                    pre + "coor_sha256": np.array(digest(coor.numpy())),
                    pre + "coor_sample": coor[:, :, ::7, ::3, ::5].contiguous().numpy(),
                    pre + "counts": np.array([rb.size, st.size], np.int32),
                    pre + "counts_per_sample": np.array(per_sample, np.int32)})
        for k, a in (("ranks_bev", rb), ("ranks_depth_canonical", rdc), ("ranks_feat_canonical", rfc),
                     ("interval_starts", st), ("interval_lengths", ln)):
            res[pre + k + "_sha256"] = np.array(digest(a))
            res[pre + k + "_sample"] = a[::max(1, a.size // 64)][:64].copy()
        print(f"{name}: B {B}, points {rb.size} of {B * N * dhw}, intervals {st.size}, per sample {per_sample}, "
              f"batched matmul == per-sample calls: {same}")
        names.append(name)
    res["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "lss_prepare_batched.npz"), **res)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pinned":
        record()
        raise SystemExit(0)
    from conftest import PINNED_CPU_ENV
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "pinned"], env=dict(os.environ, **PINNED_CPU_ENV))
