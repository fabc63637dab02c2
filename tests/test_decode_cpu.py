"""CPU-only: the detection decode -- the torch statement of both coders (bevformer_tensorrt_amd/postprocess.py)
against what the reference's own coder code returned (tests/golden/make_decode_golden.py), the tie rule, and the C ABI's
argument checks, query table and exports."""
import ctypes

import numpy as np
import pytest
import torch

import util_decode as U

F32, F16, I8 = 0, 1, 2
RTOL = 1e-6     # same library, same fp32 ops as the reference's run: scores, sizes, angle, computed x / y


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
    print(f"{what}: max relative difference {err.max() if err.size else 0.0:.3g}")
    assert err.size == 0 or err.max() <= RTOL, (what, err.max())


def _check_padded(case, got, copied, computed):
    boxes, scores, labels, count = (t.numpy() for t in got[:4])
    wb, ws, wl, wc = U.golden_padded(case["items"], case["max_num"])
    name = case["name"]
    assert np.array_equal(count, wc), (name, count, wc)
    assert np.array_equal(labels, wl), name
    assert U.bits_equal(boxes[..., list(copied)], wb[..., list(copied)]), name
    _close(boxes[..., list(computed)], wb[..., list(computed)], f"{name} computed box columns")
    _close(scores, ws, f"{name} scores")
    for b, n in enumerate(count):      # rows behind count are zero
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any(), name


@pytest.mark.parametrize("case", U.nf_cases(), ids=lambda c: c["name"])
def test_nms_free_torch_path_matches_reference(case):
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch, NMSFreeCoder
    got = nms_free_decode_torch(case["cls"], case["box"], case["max_num"], U.NF_RANGE, case["thr"], return_index=True)
    for b, it in enumerate(case["items"]):
        assert np.array_equal(got[4][b].numpy(), it["index"]), case["name"]
    _check_padded(case, got, U.NF_COPIED, U.NF_COMPUTED)
    # the coder class, reference call: per-item dicts with int64 labels
    coder = NMSFreeCoder([-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], post_center_range=U.NF_RANGE, max_num=case["max_num"],
                         score_threshold=case["thr"], num_classes=case["cls"].shape[-1])
    dicts = coder.decode({"all_cls_scores": case["cls"][None], "all_bbox_preds": case["box"][None]})
    assert len(dicts) == len(case["items"])
    for d, it in zip(dicts, case["items"]):
        assert d["labels"].dtype == torch.int64 and np.array_equal(d["labels"].numpy(), it["labels"])
        assert d["bboxes"].shape == it["bboxes"].shape and d["scores"].shape == it["scores"].shape
    # bottom_center: only z moves, by half the height
    plain = got[0]
    shifted = nms_free_decode_torch(case["cls"], case["box"], case["max_num"], U.NF_RANGE, case["thr"], True)[0]
    assert torch.equal(shifted[..., 2], plain[..., 2] - plain[..., 5] * 0.5)
    keep = [c for c in range(9) if c != 2]
    assert torch.equal(shifted[..., keep], plain[..., keep])


@pytest.mark.parametrize("case", U.cp_cases(), ids=lambda c: c["name"])
def test_centerpoint_torch_path_matches_reference(case):
    from bevformer_tensorrt_amd.postprocess import centerpoint_decode_torch, CenterPointBBoxCoder
    got = centerpoint_decode_torch(*U.cp_args(case), return_index=True)
    for b, it in enumerate(case["items"]):
        assert np.array_equal(got[4][b].numpy(), it["index"]), case["name"]
    _check_padded(case, got, U.CP_COPIED, U.CP_COMPUTED)
    # the coder class with the reference's call: scores, exp'd sizes and the rotation's two channels
    coder = CenterPointBBoxCoder(case["pc"], case["osf"], case["voxel"], post_center_range=case["range"],
                                 max_num=case["max_num"], score_threshold=case["thr"])
    dicts = coder.decode(case["heat"].sigmoid(), case["rot"][:, 0:1], case["rot"][:, 1:2], case["height"],
                         case["dim"].exp(), case["vel"], reg=case["reg"])
    for d, it in zip(dicts, case["items"]):
        assert d["labels"].dtype == torch.float32 and np.array_equal(d["labels"].numpy(), it["labels"])
        assert d["bboxes"].shape == it["bboxes"].shape      # 7 columns without vel
        _close(d["bboxes"].numpy(), it["bboxes"], f"{case['name']} coder.decode boxes")
        _close(d["scores"].numpy(), it["scores"], f"{case['name']} coder.decode scores")
    # decode_heads = the raw maps
    heads = coder.decode_heads(case["reg"], case["height"], case["dim"], case["rot"], case["vel"], case["heat"])
    for a, b in zip(heads, got[:4]):
        assert torch.equal(a, b)


def test_tie_rule_is_a_stable_descending_sort():
    """fp16-rounded logits repeat inside the top max_num; the selection must be the lexicographic order
    (logit descending, flat index ascending), stated here independently with numpy."""
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch, centerpoint_decode_torch
    g = torch.Generator().manual_seed(5)
    cls = torch.randn(2, 900, 10, generator=g).half().float()
    cls[0, 17, 3] = -0.0
    cls[0, 5, 1] = 0.0           # -0 and +0 are equal logits
    box = torch.randn(2, 900, 10, generator=g)
    K = 300
    index = nms_free_decode_torch(cls, box, K, [-1e9] * 3 + [1e9] * 3, return_index=True)[4]
    ties = 0
    for b in range(2):
        flat = cls[b].reshape(-1).numpy()
        want = np.lexsort((np.arange(flat.size), -flat))[:K]
        assert np.array_equal(index[b].numpy(), want)
        ties += int((np.diff(flat[want]) == 0).sum())
    assert ties > 0, "the draw has no equal neighbours: the test shows nothing"
    heat = (torch.randn(1, 4, 12, 10, generator=g) - 2).half().float()
    z = lambda c: torch.zeros(1, c, 12, 10)
    index = centerpoint_decode_torch(z(2), z(1), z(3), z(2), z(2), heat, 200, [-1e9] * 3 + [1e9] * 3, [0.0, 0.0], 1,
                                     [1.0, 1.0], return_index=True)[4]
    flat = heat.reshape(-1).numpy()
    assert np.array_equal(index[0].numpy(), np.lexsort((np.arange(flat.size), -flat))[:200])
    assert (np.diff(flat[index[0].numpy()]) == 0).any()


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_status_codes_without_gpu(lib):
    buf = (ctypes.c_char * 512)()
    p = (ctypes.addressof(buf) + 15) & ~15          # a host address that is never dereferenced
    rng = (ctypes.c_float * 6)(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)
    strides = (ctypes.c_int32 * 12)(*([16384, 1] * 6))

    def nf(dt=F32, cls=p, box=p, boxes=p, scores=p, labels=p, count=p, B=1, nq=900, nc=10, K=300, r=rng, thr=-1.0):
        return lib.bevops_nms_free_decode(dt, cls, box, boxes, scores, labels, count, B, nq, nc, K, r, thr, 0, None)

    assert nf(cls=None) == 2 and nf(box=None) == 2 and nf(boxes=None) == 2 and nf(scores=None) == 2
    assert nf(labels=None) == 2 and nf(count=None) == 2 and nf(r=None) == 2
    assert nf(K=0) == 2 and nf(K=-3) == 2 and nf(K=9001) == 2 and nf(B=0) == 2 and nf(nq=0) == 2 and nf(nc=0) == 2
    assert nf(thr=float("inf")) == 2 and nf(thr=float("nan")) == 2
    assert nf(dt=I8) == 3
    assert nf(nq=1639, nc=10, K=300) == 3            # 16 390 candidates: beyond one workgroup's selection
    assert nf(F16, nq=2048, nc=8, K=0) == 2          # argument errors come first

    def cp(dt=F32, reg=p, hei=p, dim=p, rot=p, vel=p, heat=p, s=strides, boxes=p, scores=p, labels=p, count=p, B=1,
           nc=10, H=128, W=128, K=500, r=rng, thr=0.1, ws=None, nws=0):
        return lib.bevops_centerpoint_decode(dt, reg, hei, dim, rot, vel, heat, s, boxes, scores, labels, count, B, nc,
                                             H, W, K, 8.0, 0.1, 0.1, -51.2, -51.2, r, thr, 1, 0, ws, nws, None)

    assert cp(hei=None) == 2 and cp(dim=None) == 2 and cp(rot=None) == 2 and cp(heat=None) == 2 and cp(s=None) == 2
    assert cp(boxes=None) == 2 and cp(scores=None) == 2 and cp(labels=None) == 2 and cp(count=None) == 2
    assert cp(r=None) == 2
    assert cp(K=0) == 2 and cp(nc=3, H=20, W=24, K=1441) == 2 and cp(B=0) == 2 and cp(H=0) == 2
    assert cp(dt=I8) == 3 and cp(K=4097) == 3
    need = lib.bevops_centerpoint_decode_workspace_size(1, 10, 128, 128, 500)
    assert need == 40 * 500 * 8                      # 40 chunks of 4 096 cells, 500 keys each
    assert cp() == 2 and cp(ws=p, nws=need - 1) == 2  # needs the workspace it asks for
    assert lib.bevops_centerpoint_decode_workspace_size(2, 3, 20, 24, 40) == 0      # fits one workgroup: one launch
    assert lib.bevops_centerpoint_decode_workspace_size(0, 10, 128, 128, 500) == 0


def test_query_table_exports_and_registry(lib):
    import bevformer_tensorrt_amd as bev
    import bevformer_tensorrt_amd.functions as fn
    from test_qkv_inverse_cpu import REFERENCE_REGISTRY

    def addr(sym):
        return ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value
    for sym in ("bevops_nms_free_decode", "bevops_centerpoint_decode", "bevops_centerpoint_decode_workspace_size"):
        assert lib.bevops_query(sym.encode()) == addr(sym), sym
    # ... and the old name still means the head's de-normalisation
    assert lib.bevops_query(b"bevops_decode_boxes") == addr("bevops_decode_boxes")
    assert addr("bevops_decode_boxes") != addr("bevops_nms_free_decode")
    for name in ("nms_free_decode", "centerpoint_decode"):
        assert name in fn.__all__ and getattr(bev, name) is getattr(fn, name)
        assert name not in bev.TRT_FUNCTIONS
    # the registry mirrors the reference's 13 names (plus this package's int8 / SCA variants), decode not among them
    extra = {"multi_scale_deformable_attn_int8", "rotate_int8", "grid_sampler_int8", "bev_pool_v2_int8",
             "modulated_deformable_conv2d_int8", "spatial_cross_attention_sample"}
    assert set(bev.TRT_FUNCTIONS.module_dict) - extra == set(REFERENCE_REGISTRY)
