#!/usr/bin/env python3
"""Fixture of the device index build of BEVDet's view transformer (csrc/lss_prepare.hip): tests/golden/lss_prepare.npz.
Build container only (needs the reference tree):

    python tests/golden/make_lss_prepare_golden.py

create_grid_infos, create_frustum, get_lidar_coor and voxel_pooling_prepare_v2 are lifted from the reference's
third_party/bev_mmdet3d/models/necks/view_transformer.py by AST (make_wrapper_golden.lift) and EXECUTED on the CPU,
in a child interpreter under tests/conftest.py's PINNED_CPU_ENV (the CPU kernel choice the bit-exact tests run with).
Per case the fixture holds the calibration inputs, the packed calibration buffer, the grid, the counts, small samples
and SHA-256 digests of: coor, ranks_bev, interval_starts, interval_lengths and the CANONICAL ranks_depth / ranks_feat
(sorted ascending inside each interval -- the reference's argsort leaves that order unspecified).  Whole arrays are
megabytes and are not stored.

Asserted while recording: the plain-order statement of the coordinates equals the lifted get_lidar_coor bit for bit;
ranks_feat is (ranks_depth // (D H W)) (H W) + ranks_depth % (H W); every R50-grid case keeps some points and drops some.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]

R50_GRID = dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 60.0, 1.0])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def canonical(ranks_depth, starts, lengths):
    """ranks_depth sorted ascending inside each interval"""
    out = ranks_depth.copy()
    for s, n in zip(starts.tolist(), lengths.tolist()):
        out[s:s + n] = np.sort(out[s:s + n])
    return out


def cases(view):
    import make_wrapper_golden as W
    from bevformer_tensorrt_amd.bevdet import jittered_rig, synthetic_rig
    s2e, K, post_rots, post_trans, bda = W.reference_test_calibration()
    post_rots = post_rots.clone()
    post_rots[..., :2, :2] *= 0.5          # the test's rig is calibrated for 512x1408; R50 runs at 256x704
    out = [("ref_r50", R50_GRID, (s2e, K, post_rots, post_trans.clone() * 0.5, bda))]
    pick = lambda rig: (rig[0], rig[2], rig[3], rig[4], rig[5])
    out.append(("rig", R50_GRID, pick(synthetic_rig(view))))
    for k in (1, 2, 3):
        out.append((f"jitter{k}", R50_GRID, pick(jittered_rig(view, k))))
    out.append(("one_camera", R50_GRID, pick(jittered_rig(view, 4, n_cams=1))))
    out.append(("z_cells", dict(R50_GRID, z=[-5, 3, 2]), pick(jittered_rig(view, 5))))
    out.append(("small_grid", dict(R50_GRID, x=[-22.0, 22.0, 4.0], y=[-14.0, 14.0, 4.0]), pick(jittered_rig(view, 6))))
    out.append(("one_cell", dict(R50_GRID, x=[-1000.0, 1000.0, 2000.0], y=[-1000.0, 1000.0, 2000.0]),
                pick(jittered_rig(view, 7))))
    out.append(("nothing_kept", dict(R50_GRID, x=[5000.0, 5102.4, 0.8]), pick(synthetic_rig(view))))
    return out


def record():
    import make_wrapper_golden as W
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, LSSViewTransformer
    path = "third_party/bev_mmdet3d/models/necks/view_transformer.py"
    fns = {n: W.lift(path, "LSSViewTransformer", n)
           for n in ("create_grid_infos", "create_frustum", "get_lidar_coor", "voxel_pooling_prepare_v2")}
    ours = LSSViewTransformer(**BEVDET_R50, ops=object())
    res = {}
    names = []
    for name, grid, (s2e, K, post_rots, post_trans, bda) in cases(ours):
        me = W.Stub(sid=False)
        fns["create_grid_infos"](me, **grid)
        me.frustum = fns["create_frustum"](me, grid["depth"], (256, 704), 16)
        assert torch.equal(me.frustum, ours.frustum)
        coor = fns["get_lidar_coor"](me, s2e, None, K, post_rots, post_trans, bda)
        calib = ours.calibration_matrices(s2e, None, K, post_rots, post_trans, bda)
        plain = ours.lidar_coor_plain(calib)
        assert plain.shape == coor.shape and np.array_equal(plain.numpy().view(np.int32), coor.numpy().view(np.int32)), name
        ranks = fns["voxel_pooling_prepare_v2"](me, coor)
        B, N, D, H, Wd, _ = coor.shape
        num_points = N * D * H * Wd
        pre = name + "."
        res.update({pre + "sensor2ego": s2e.numpy(), pre + "cam2imgs": K.numpy(), pre + "post_rots": post_rots.numpy(),
                    pre + "post_trans": post_trans.numpy(), pre + "bda": bda.numpy(), pre + "calib": calib.numpy(),
                    pre + "grid": np.stack([me.grid_lower_bound.numpy(), me.grid_interval.numpy(), me.grid_size.numpy()]),
                    pre + "coor_sha256": np.array(digest(coor.contiguous().numpy())),
                    pre + "coor_sample": coor[0, :, ::7, ::3, ::5].contiguous().numpy()})
        if ranks[0] is None:
            res[pre + "counts"] = np.array([0, 0], np.int32)
            assert name == "nothing_kept"
        else:
            rb, rd, rf, st, ln = (t.numpy().astype(np.int32) for t in ranks)
            assert np.array_equal(rf, (rd // (D * H * Wd)) * (H * Wd) + rd % (H * Wd)), name
            if grid is R50_GRID:
                assert 0 < rb.size < num_points, name
            rdc = canonical(rd, st, ln)
            rfc = (rdc // (D * H * Wd)) * (H * Wd) + rdc % (H * Wd)
            res[pre + "counts"] = np.array([rb.size, st.size], np.int32)
            for k, a in (("ranks_bev", rb), ("ranks_depth_canonical", rdc), ("ranks_feat_canonical", rfc),
                         ("interval_starts", st), ("interval_lengths", ln)):
                res[pre + k + "_sha256"] = np.array(digest(a))
                res[pre + k + "_sample"] = a[::max(1, a.size // 64)][:64].copy()
            print(f"{name}: points {rb.size} of {num_points}, intervals {st.size}, longest {int(ln.max())}")
        names.append(name)
    assert "nothing_kept" in names and int(res["nothing_kept.counts"].sum()) == 0
    res["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "lss_prepare.npz"), **res)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pinned":
        record()
        raise SystemExit(0)
    from conftest import PINNED_CPU_ENV
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "pinned"], env=dict(os.environ, **PINNED_CPU_ENV))
