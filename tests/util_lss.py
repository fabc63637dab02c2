"""Shared by the tests of the BEVDet index build (tests/golden/lss_prepare.npz, recorded by
tests/golden/make_lss_prepare_golden.py from the reference's own view-transformer methods)."""
import hashlib

import numpy as np
import torch

from conftest import golden

ORDER_FREE = ("ranks_bev", "interval_starts", "interval_lengths")
CANONICAL = ("ranks_depth_canonical", "ranks_feat_canonical")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture():
    g = golden("lss_prepare")
    return g, [str(c) for c in g["cases"]]


def view_for(g, case):
    """LSSViewTransformer at the R50 frustum with the grid of `case`."""
    from bevformer_tensorrt_amd.bevdet import BEVDET_R50, LSSViewTransformer
    vt = LSSViewTransformer(**BEVDET_R50, ops=object())
    lower, interval, size = (torch.from_numpy(a.copy()) for a in g[case + ".grid"])
    vt.grid_lower_bound, vt.grid_interval, vt.grid_size = lower, interval, size
    return vt


def inputs(g, case):
    t = lambda k: torch.from_numpy(g[f"{case}.{k}"])
    return t("sensor2ego"), None, t("cam2imgs"), t("post_rots"), t("post_trans"), t("bda")


def sample(a):
    return a[::max(1, a.size // 64)][:64]


def check_arrays(g, case, rb, rd, rf, st, ln):
    """the five trimmed int32 numpy arrays, in the stable order, against the fixture's digests and samples"""
    n_pts, n_int = (int(v) for v in g[case + ".counts"])
    assert rb.size == rd.size == rf.size == n_pts and st.size == ln.size == n_int, case
    for name, a in zip(ORDER_FREE + CANONICAL, (rb, st, ln, rd, rf)):
        assert a.dtype == np.int32
        assert np.array_equal(sample(a), g[f"{case}.{name}_sample"]), (case, name)
        assert digest(a) == str(g[f"{case}.{name}_sha256"]), (case, name)
