"""GPU: the detection decode kernels (csrc/decode.hip) through the C ABI and the Python layer -- the golden cases of the
reference's own coder code, fp16 inputs, shapes off the fixtures against the CPU torch statement
(bevformer_tensorrt_amd/postprocess.py), determinism, graph capture, and the two models' decode entry points.

Numeric rule for the columns that go through a transcendental or an fp32 multiply-add (score, e^w / e^l / e^h or
exp(dim), angle, x / y): the error against an fp64 evaluation of the same inputs must not exceed twice the larger of
(a) the error of torch's own fp32 device ops (sigmoid, exp, atan2, the multiply-add of x / y) on the same values and
(b) one fp32 ulp of the value -- element by element.  The factor 2 admits a different but equally good expf / atan2f.
Everything else (count, labels, which candidates, copied columns, zero tail) is exact."""
import ctypes

import numpy as np
import pytest
import torch

import util_decode as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDE = [-1e9] * 3 + [1e9] * 3


def _bounded(ours, theirs, truth, what):
    ours, theirs, truth = (np.asarray(t, np.float64) for t in (ours, theirs, truth))
    eo, et = np.abs(ours - truth), np.abs(theirs - truth)
    bound = 2 * np.maximum(et, U.ulp32(truth))
    u = U.ulp32(truth)
    print(f"{what}: ours max {np.max(eo / u) if eo.size else 0:.3f} ulp, torch device ops max "
          f"{np.max(et / u) if et.size else 0:.3f} ulp ({eo.size} values)")
    assert (eo <= bound).all(), (what, float((eo / u).max()), float((et / u).max()))


def _exact_part(got, want, copied, what):
    """count, labels, copied columns and the zero tail of a padded result against another (numpy, cpu)."""
    gb, gs, gl, gc = (t.cpu().numpy() if torch.is_tensor(t) else t for t in got[:4])
    wb, ws, wl, wc = (t.cpu().numpy() if torch.is_tensor(t) else t for t in want[:4])
    assert np.array_equal(gc, wc), (what, gc, wc)
    assert np.array_equal(gl, wl), what
    assert U.bits_equal(gb[..., list(copied)], wb[..., list(copied)]), what
    for b, n in enumerate(gc):
        assert not gb[b, n:].any() and not gs[b, n:].any() and not gl[b, n:].any(), what
    return gb, gs, gc


def _nf_numeric(case_name, cls, box, got_boxes, got_scores, index, keep):
    """cls / box: CPU fp32 tensors (the values the kernel saw, widened); index / keep from the torch path."""
    nc = cls.shape[-1]
    for b in range(cls.shape[0]):
        sel = index[b][keep[b]]
        n = sel.numel()
        t = U.nf_fp64(cls[b], box[b], sel, nc)
        dc, db = cls[b].reshape(-1)[sel].to(DEV), box[b][torch.div(sel, nc, rounding_mode="trunc")].to(DEV)
        dev = dict(score=dc.sigmoid(), w=db[:, 2].exp(), l=db[:, 3].exp(), h=db[:, 5].exp(),
                   rot=torch.atan2(db[:, 6], db[:, 7]))
        ours = dict(score=got_scores[b, :n], w=got_boxes[b, :n, 3], l=got_boxes[b, :n, 4], h=got_boxes[b, :n, 5],
                    rot=got_boxes[b, :n, 6])
        for k in ours:
            _bounded(ours[k], dev[k].cpu().numpy(), t[k].numpy(), f"{case_name}[{b}] {k}")


def _cp_numeric(case, maps, got_boxes, got_scores, index, keep):
    H, W = maps["heat"].shape[-2:]
    for b in range(maps["heat"].shape[0]):
        sel = index[b][keep[b]]
        n = sel.numel()
        t = U.cp_fp64(case, b, sel, maps)
        cell = (sel % (H * W)).to(DEV)
        at = lambda m, ch: m[b, ch].reshape(-1).to(DEV)[cell]
        rx = at(maps["reg"], 0) if maps["reg"] is not None else 0.5
        ry = at(maps["reg"], 1) if maps["reg"] is not None else 0.5
        dev = dict(score=maps["heat"][b].reshape(-1).to(DEV)[sel.to(DEV)].sigmoid(),
                   x=((cell % W).float() + rx) * case["osf"] * case["voxel"][0] + case["pc"][0],
                   y=(torch.div(cell, W, rounding_mode="trunc").float() + ry) * case["osf"] * case["voxel"][1] + case["pc"][1],
                   d0=at(maps["dim"], 0).exp(), d1=at(maps["dim"], 1).exp(), d2=at(maps["dim"], 2).exp(),
                   rot=torch.atan2(at(maps["rot"], 0), at(maps["rot"], 1)))
        ours = dict(score=got_scores[b, :n], x=got_boxes[b, :n, 0], y=got_boxes[b, :n, 1], d0=got_boxes[b, :n, 3],
                    d1=got_boxes[b, :n, 4], d2=got_boxes[b, :n, 5], rot=got_boxes[b, :n, 6])
        for k in ours:
            _bounded(ours[k], dev[k].cpu().numpy(), t[k].numpy(), f"{case['name']}[{b}] {k}")


# ---------------------------------------------------------------------------------------------- golden cases, fp32
@pytest.mark.parametrize("case", U.nf_cases(), ids=lambda c: c["name"])
def test_nms_free_golden_fp32(case):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch
    got = bev.nms_free_decode(case["cls"].to(DEV), case["box"].to(DEV), case["max_num"], U.NF_RANGE, case["thr"],
                              padded=True)
    want = U.golden_padded(case["items"], case["max_num"])
    gb, gs, gc = _exact_part(got, want, U.NF_COPIED, case["name"])
    ref = nms_free_decode_torch(case["cls"], case["box"], case["max_num"], U.NF_RANGE, case["thr"], return_index=True)
    for b, it in enumerate(case["items"]):      # the torch path selected what the reference selected
        assert np.array_equal(ref[4][b].numpy(), it["index"])
    _nf_numeric(case["name"], case["cls"], case["box"], gb, gs, ref[4], ref[5])
    # the trimmed form and the z shift
    dicts = bev.nms_free_decode(case["cls"].to(DEV), case["box"].to(DEV), case["max_num"], U.NF_RANGE, case["thr"])
    for b, d in enumerate(dicts):
        assert d["bboxes"].shape == (gc[b], 9) and torch.equal(d["bboxes"].cpu(), got[0][b, :gc[b]].cpu())
    low = bev.nms_free_decode(case["cls"].to(DEV), case["box"].to(DEV), case["max_num"], U.NF_RANGE, case["thr"],
                              bottom_center=True, padded=True)
    assert torch.equal(low[0][..., 2], got[0][..., 2] - got[0][..., 5] * 0.5)
    others = [c for c in range(9) if c != 2]
    assert torch.equal(low[0][..., others], got[0][..., others]) and torch.equal(low[3], got[3])


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("case", U.cp_cases(), ids=lambda c: c["name"])
def test_centerpoint_golden_fp32(case, layout):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centerpoint_decode_torch
    got = bev.centerpoint_decode(*U.cp_args(case, DEV, torch.float32, layout == "channels_last"), padded=True)
    want = U.golden_padded(case["items"], case["max_num"])
    gb, gs, gc = _exact_part(got, want, U.CP_COPIED, case["name"])
    ref = centerpoint_decode_torch(*U.cp_args(case), return_index=True)
    for b, it in enumerate(case["items"]):
        assert np.array_equal(ref[4][b].numpy(), it["index"])
    _cp_numeric(case, case, gb, gs, ref[4], ref[5])
    dicts = bev.centerpoint_decode(*U.cp_args(case, DEV, torch.float32, layout == "channels_last"))
    for b, d in enumerate(dicts):
        assert d["bboxes"].shape == (gc[b], 9 if case["vel"] is not None else 7)


# ---------------------------------------------------------------------------------------------- fp16 inputs
@pytest.mark.parametrize("case", U.nf_cases(), ids=lambda c: c["name"])
def test_nms_free_fp16_inputs(case):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch
    cls16, box16 = case["cls"].half(), case["box"].half()
    got = bev.nms_free_decode(cls16.to(DEV), box16.to(DEV), case["max_num"], U.NF_RANGE, case["thr"], padded=True)
    ref = nms_free_decode_torch(cls16.float(), box16.float(), case["max_num"], U.NF_RANGE, case["thr"],
                                return_index=True)
    gb, gs, _ = _exact_part(got, ref, U.NF_COPIED, case["name"] + " fp16")
    _nf_numeric(case["name"] + " fp16", cls16.float(), box16.float(), gb, gs, ref[4], ref[5])


@pytest.mark.parametrize("case", U.cp_cases(), ids=lambda c: c["name"])
def test_centerpoint_fp16_inputs(case):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centerpoint_decode_torch
    args16 = U.cp_args(case, DEV, torch.float16, True)
    got = bev.centerpoint_decode(*args16, padded=True)
    wide = [None if t is None else t.float().cpu().contiguous() for t in args16[:6]]
    ref = centerpoint_decode_torch(*wide, *args16[6:], return_index=True)
    gb, gs, _ = _exact_part(got, ref, U.CP_COPIED, case["name"] + " fp16")
    maps = dict(zip(("reg", "height", "dim", "rot", "vel", "heat"), wide))
    _cp_numeric(case, maps, gb, gs, ref[4], ref[5])


# ---------------------------------------------------------------------------------------------- off the fixtures
def _same_as_torch_path(got, ref, copied, computed, what):
    gb, gs, _ = _exact_part(got, ref, copied, what)
    rb, rs = ref[0].numpy(), ref[1].numpy()
    # both sides are fp32 evaluations with library functions good to a few ulp: 1e-6 relative covers their sum; x / y
    # are the same rounded steps on both sides and the angle keeps its relative error at any size
    assert np.allclose(gb[..., list(computed)], rb[..., list(computed)], rtol=1e-6, atol=1e-6), what
    assert np.allclose(gs, rs, rtol=1e-6, atol=0), what


@pytest.mark.parametrize("B,nq,nc,K,thr,dtype", [
    (3, 901, 7, 333, None, torch.float32), (3, 777, 1, 777, 0.6, torch.float16), (1, 1, 1, 1, None, torch.float32),
    (2, 1638, 10, 1025, 0.999, torch.float16), (1, 2048, 8, 16384, None, torch.float32), (3, 63, 7, 64, 0.3, torch.float32)])
def test_nms_free_random_shapes_equal_torch_path(B, nq, nc, K, thr, dtype):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch
    g = torch.Generator().manual_seed(B * 1000 + nq + nc)
    cls = torch.randn(B, nq, nc, generator=g).to(dtype)
    box = (torch.randn(B, nq, 10, generator=g) * torch.tensor([40.0, 40, 0.5, 0.5, 6, 0.5, 1, 1, 1, 1])).to(dtype)
    for bottom in (False, True):
        got = bev.nms_free_decode(cls.to(DEV), box.to(DEV), K, U.NF_RANGE, thr, bottom_center=bottom, padded=True)
        ref = nms_free_decode_torch(cls, box, K, U.NF_RANGE, thr, bottom_center=bottom)
        _same_as_torch_path(got, ref, (0, 1, 7, 8), (2, 3, 4, 5, 6), f"nms_free {B}x{nq}x{nc} top {K} {dtype}")


@pytest.mark.parametrize("B,nc,H,W,K,thr,dtype,cl,vel,reg", [
    (3, 7, 33, 21, 100, 0.05, torch.float16, True, True, True),      # 4 851 cells: two chunks, the second ragged
    (3, 1, 64, 64, 4096, None, torch.float32, False, True, True),    # one class, one chunk, max_num = every cell
    (1, 10, 128, 128, 500, 0.1, torch.float16, True, True, True),    # BEVDet-R50, channels-last fp16 as the model emits
    (2, 3, 9, 11, 297, 0.2, torch.float32, True, False, False),      # one launch, max_num = every cell, no vel, no reg
    (1, 5, 100, 100, 4096, None, torch.float32, False, True, False)])
def test_centerpoint_random_shapes_equal_torch_path(B, nc, H, W, K, thr, dtype, cl, vel, reg):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centerpoint_decode_torch
    g = torch.Generator().manual_seed(nc * 100 + H + W)
    mk = lambda c, s=1.0: (torch.randn(B, c, H, W, generator=g) * s).to(dtype)
    maps = [mk(2) if reg else None, mk(1, 6.0), mk(3, 0.5), mk(2), mk(2) if vel else None, mk(nc) - 2]
    post = [-40.0, -40.0, -10.0, 40.0, 40.0, 10.0]
    tail = [K, post, [-51.2, -50.0], 8, [0.1, 0.125], thr]
    dev = [None if t is None else (t.to(DEV).contiguous(memory_format=torch.channels_last) if cl else t.to(DEV))
           for t in maps]
    for norm in (True, False):
        got = bev.centerpoint_decode(*dev, *tail, norm_bbox=norm, padded=True)
        ref = centerpoint_decode_torch(*maps, *tail, norm_bbox=norm)
        copied = (2, 7, 8) if norm else (2, 3, 4, 5, 7, 8)
        _same_as_torch_path(got, ref, copied, (0, 1, 3, 4, 5, 6), f"centerpoint {B}x{nc}x{H}x{W} top {K} {dtype}")
    # the coder's own call: scores in, ranked as they are
    scores = maps[5].float().sigmoid().to(dtype)
    got = bev.centerpoint_decode(*dev[:5], scores.to(DEV), *tail, norm_bbox=False, heatmap_is_score=True, padded=True)
    ref = centerpoint_decode_torch(*maps[:5], scores, *tail, norm_bbox=False, heatmap_is_score=True)
    _same_as_torch_path(got, ref, (2, 3, 4, 5, 7, 8), (0, 1, 6), "centerpoint, scores in")
    assert U.bits_equal(got[1].cpu().numpy(), ref[1].numpy())


# ---------------------------------------------------------------------------------------------- contract
def _tie_inputs():
    g = torch.Generator().manual_seed(11)
    cls = torch.randn(2, 900, 10, generator=g).half()          # fp16 logits: ties inside the top 300
    box = torch.randn(2, 900, 10, generator=g).half()
    heat = (torch.randn(1, 10, 128, 128, generator=g) - 3).half()
    mk = lambda c: torch.randn(1, c, 128, 128, generator=g).half().to(DEV).contiguous(memory_format=torch.channels_last)
    maps = [mk(2), mk(1), mk(3), mk(2), mk(2), heat.to(DEV).contiguous(memory_format=torch.channels_last)]
    return cls.to(DEV), box.to(DEV), maps


CP_TAIL = [500, U.NF_RANGE, [-51.2, -51.2], 8, [0.1, 0.1], 0.1]


def test_ties_follow_the_rule_and_results_are_bit_reproducible():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch, centerpoint_decode_torch
    cls, box, maps = _tie_inputs()
    first = bev.nms_free_decode(cls, box, 300, WIDE, padded=True)
    ref = nms_free_decode_torch(cls.cpu(), box.cpu(), 300, WIDE, return_index=True)
    flat = cls[0].float().cpu().reshape(-1).numpy()
    assert (np.diff(flat[ref[4][0].numpy()]) == 0).sum() > 0, "no equal neighbours in the top 300"
    _exact_part(first, ref, (0, 1, 2, 7, 8), "ties, nms_free")
    cp_first = bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
    cp_ref = centerpoint_decode_torch(*[m.cpu() for m in maps], *CP_TAIL, return_index=True)
    flat = maps[5].float().cpu().reshape(-1).numpy()
    assert (np.diff(flat[cp_ref[4][0].numpy()]) == 0).sum() > 0, "no equal neighbours in the top 500"
    _exact_part(cp_first, cp_ref, U.CP_COPIED, "ties, centerpoint")
    for _ in range(20):
        again = bev.nms_free_decode(cls, box, 300, WIDE, padded=True)
        cp_again = bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
        for a, b in zip(first + cp_first, again + cp_again):
            assert torch.equal(a, b)


def test_graph_capture_follows_inputs_changed_in_place():
    import bevformer_tensorrt_amd as bev
    cls, box, maps = _tie_inputs()
    cls, box = cls[:1].clone(), box[:1].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bev.nms_free_decode(cls, box, 300, U.NF_RANGE, 0.5, bottom_center=True, padded=True)
        bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_nf = bev.nms_free_decode(cls, box, 300, U.NF_RANGE, 0.5, bottom_center=True, padded=True)
        out_cp = bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
    g = torch.Generator().manual_seed(3)
    seen = set()
    for r in range(3):
        cls.copy_(torch.randn(1, 900, 10, generator=g).half() + (r - 1) * 2.0)
        box.copy_((torch.randn(1, 900, 10, generator=g) * torch.tensor([40.0, 40, 0.5, 0.5, 6, 0.5, 1, 1, 1, 1])).half())
        maps[5].copy_((torch.randn(1, 10, 128, 128, generator=g) - 4 + r).half())
        maps[1].copy_((torch.randn(1, 1, 128, 128, generator=g) * (3 + 3 * r)).half())
        graph.replay()
        torch.cuda.synchronize()
        eager_nf = bev.nms_free_decode(cls, box, 300, U.NF_RANGE, 0.5, bottom_center=True, padded=True)
        eager_cp = bev.centerpoint_decode(*maps, *CP_TAIL, padded=True)
        for a, b in zip(out_nf + out_cp, eager_nf + eager_cp):
            assert torch.equal(a, b)
        seen.add((int(out_nf[3][0]), int(out_cp[3][0])))
    assert len(seen) == 3, seen          # the replays did follow the inputs


def test_c_abi_direct_and_domain():
    """The C entry with raw pointers (no Python wrapper in between) and the unsupported domains through the wrapper."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    from bevformer_tensorrt_amd.postprocess import nms_free_decode_torch
    lib = L.load_library()
    case = U.nf_cases()[0]
    cls, box = case["cls"].to(DEV), case["box"].to(DEV)
    K = case["max_num"]
    boxes = torch.full((1, K, 9), 7.0, device=DEV)
    scores = torch.full((1, K), 7.0, device=DEV)
    labels = torch.full((1, K), 7, device=DEV, dtype=torch.int32)
    count = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    rng = (ctypes.c_float * 6)(*U.NF_RANGE)
    st = lib.bevops_nms_free_decode(0, cls.data_ptr(), box.data_ptr(), boxes.data_ptr(), scores.data_ptr(),
                                    labels.data_ptr(), count.data_ptr(), 1, 900, 10, K, rng, -1.0, 0,
                                    L.current_stream_ptr(cls.device))
    assert st == 0
    torch.cuda.synchronize()
    _exact_part((boxes, scores, labels, count), U.golden_padded(case["items"], K), U.NF_COPIED, "C ABI")
    z = torch.zeros(1, 1700, 10, device=DEV)
    with pytest.raises(L.BevopsError) as e:
        bev.nms_free_decode(z, z, 300, WIDE)
    assert e.value.status == L.NOT_SUPPORTED
    with pytest.raises(L.BevopsError) as e:
        bev.nms_free_decode(z[:, :900], z[:, :900], 9001, WIDE)
    assert e.value.status == L.BAD_PARAM
    zi = torch.zeros(1, 900, 10, device=DEV, dtype=torch.int8)
    with pytest.raises(L.BevopsError) as e:
        bev.nms_free_decode(zi, zi, 300, WIDE)
    assert e.value.status == L.NOT_SUPPORTED
    # an unaligned view is read in place
    pad = torch.zeros(9001, device=DEV)
    pad[1:] = cls.reshape(-1)
    got = bev.nms_free_decode(pad[1:].view(1, 900, 10), box, K, U.NF_RANGE, padded=True)
    ref = nms_free_decode_torch(case["cls"], case["box"], K, U.NF_RANGE)
    _exact_part(got, ref, U.NF_COPIED, "unaligned input")


# ---------------------------------------------------------------------------------------------- models
def _frames(image, n, dtype):
    from test_model_gpu import frames
    return frames(image, n, torch.device(DEV), dtype)


def test_frame_runner_decode_inside_the_graph():
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev, dtype = torch.device(DEV), torch.float16
    make = lambda: B.BEVFormer("tiny", seed=0).to(dev, dtype)      # the same weights for every runner
    model = make()
    l2i = G.synthetic_lidar2img(B.CONFIGS["tiny"]["image"]).to(dev)
    plain = B.FrameRunner(make(), dev, dtype, graph=True)
    off = B.FrameRunner(make(), dev, dtype, graph=True, decode=False)
    on = B.FrameRunner(model, dev, dtype, graph=True, decode=True)
    eager = B.FrameRunner(make(), dev, dtype, graph=False, decode=True)
    for img, can, scene in _frames(B.CONFIGS["tiny"]["image"], 2, dtype):
        a, b = plain.step(img, can, l2i, scene), off.step(img, can, l2i, scene)
        c, e = on.step(img, can, l2i, scene), eager.step(img, can, l2i, scene)
        assert len(a) == len(b) == 2 and len(c) == len(e) == 6
        for x, y in zip(a, b):
            assert torch.equal(x, y)            # decode=False is today's step
        for x, y in zip(a, c[:2]):
            assert torch.equal(x, y)            # ... and decoding does not disturb the frame
        cls, crd, boxes, scores, labels, count = c
        assert boxes.shape == (1, 300, 9) and scores.shape == (1, 300) and labels.dtype == torch.int32
        ref = model.bbox_coder.decode_padded(cls[-1].float().cpu(), crd[-1].float().cpu(), bottom_center=True)
        _same_as_torch_path((boxes, scores, labels, count), ref, (0, 1, 7, 8), (2, 3, 4, 5, 6), "FrameRunner(decode=True)")
        assert int(count[0]) > 0
        # the eager runner decodes its own frame the same way
        ref_e = model.bbox_coder.decode_padded(e[0][-1].float().cpu(), e[1][-1].float().cpu(), bottom_center=True)
        _same_as_torch_path(e[2:], ref_e, (0, 1, 7, 8), (2, 3, 4, 5, 6), "FrameRunner(decode=True), eager")
        # trimmed dicts from the model's own entry point
        d = model.get_bboxes(cls, crd)[0]
        assert d["bboxes"].shape == (int(count[0]), 9) and d["labels"].dtype == torch.int64
        assert torch.equal(d["scores"], scores[0, :int(count[0])])


def test_bevdet_get_candidates():
    from bevformer_tensorrt_amd import bevdet as D
    model = D.BEVDet(seed=0)
    g = torch.Generator().manual_seed(2)
    mk = lambda c, s=1.0, o=0.0: ((torch.randn(1, c, 128, 128, generator=g) * s + o).half().to(DEV)
                                  .contiguous(memory_format=torch.channels_last))
    outputs = (mk(2), mk(1, 6.0), mk(3, 0.5), mk(2), mk(2), mk(10, 1.0, -5.2))     # one synthetic frame of head maps
    got = model.get_candidates(outputs, padded=True)
    ref = model.bbox_coder.decode_heads(*[t.float().cpu().contiguous() for t in outputs])
    _same_as_torch_path(got, ref, U.CP_COPIED, U.CP_COMPUTED, "BEVDet.get_candidates")
    n = int(got[3][0])
    assert 0 < n < 500 and got[0].shape == (1, 500, 9)
    d = model.get_candidates(outputs)[0]
    assert d["bboxes"].shape == (n, 9) and d["labels"].dtype == torch.float32
    assert float(d["scores"].min()) > 0.1
