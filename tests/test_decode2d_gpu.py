"""GPU: the 2-D heads' kernels (csrc/decode2d.hip) through the Python layer and the C ABI.

Exactness.  bevops_centernet_decode contains only +, -, x, / and comparisons: every output equals the fixtures of
tests/golden/make_decode2d_golden.py (an independent numpy / float32 statement) bit for bit.  bevops_box_nms equals
`box_nms_torch` run on the SAME input bits exactly (index, count, copied rows): both sides evaluate one fp32 operation
sequence, so no margin is needed.  bevops_yolox_decode: labels and prior order exact; the rows whose log sizes are 0
(w = h = stride exactly, so the corners are cx, cy plus or minus an exact half stride) exact, which pins cx and cy.

Transcendental columns (w and h, seen through the corners, and the score) against float64.  No bar was fixed in advance:
measured on the fixtures, torch's own fp32 CPU ops are off by at most 1.4782 ulp (corners) and 2.3075 ulp (score), the
kernel by 1.4782 and 2.2906; the bar is twice the larger, rounded up to a whole ulp: 3 and 5 (util_decode2d.BAR_ULP;
the units are defined at util_decode2d.yolox_errors).

Call contract: each entry captured into a graph and replayed (a host synchronisation inside would break the capture),
two calls and two replays give equal bits, outputs behind `count` are zero.  Buffer contract: the entries in the
guarded arena of tests/util_arena.py at the fixtures' tail shapes, workspace exactly the size query's bytes at the
documented 8-byte alignment, both poisons."""
import numpy as np
import pytest
import torch

import util_decode2d as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
CL = lambda t: t.contiguous(memory_format=torch.channels_last)


def _same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        w = w.cpu().numpy() if torch.is_tensor(w) else w
        assert U.bits_equal(g, w), f"{what}: output {i} differs"


def _zero_behind_count(out, what):
    count = out[3].cpu().numpy()
    for t in (out[0], out[1], out[2]) + tuple(out[4:5]):
        a = t.cpu().numpy()
        for b, n in enumerate(count):
            assert not a[b, n:].any(), f"{what}: non-zero behind count"


def _cn_args(case, layout=False, dtype=None):
    dt = dtype or (torch.float16 if case["f16"] else torch.float32)
    maps = [T(case[k]).to(dt) for k in ("heat", "wh", "off")]
    return [CL(m) for m in maps] if layout else maps


# ------------------------------------------------------------------------------------------------------ CenterNet
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("case", U.cn_cases(), ids=lambda c: c["name"])
def test_centernet_equals_fixture_bit_for_bit(case, layout):
    import bevformer_tensorrt_amd as bev
    out = bev.centernet_decode(*_cn_args(case, layout == "channels_last"), case["k"], case["inp"], case["kernel"],
                               case["border"], case["scale"], padded=True)
    _same(out, [case[k] for k in ("boxes", "scores", "labels", "count")], case["name"])
    # the padded form under a score test, and the trimmed dicts
    thr = float(np.median(case["scores"]))
    got = bev.centernet_decode(*_cn_args(case, layout == "channels_last"), case["k"], case["inp"], case["kernel"],
                               case["border"], case["scale"], score_threshold=thr, padded=True)
    want = U.np_centernet(case["heat"], case["wh"], case["off"], case["k"], case["kernel"], case["inp"], case["border"],
                          case["scale"], thr)
    _same(got, want[:4], case["name"] + " with a score threshold")
    _zero_behind_count(got, case["name"])
    dicts = bev.centernet_decode(*_cn_args(case), case["k"], case["inp"], case["kernel"], case["border"], case["scale"])
    assert [tuple(d["bboxes"].shape) for d in dicts] == [(case["k"], 4)] * case["heat"].shape[0]


def test_centernet_fp16_inputs_are_widened():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centernet_decode_torch
    g = torch.Generator().manual_seed(3)
    heat = torch.rand(2, 5, 37, 29, generator=g).half()          # fp16 scores: ties inside the top k
    wh, off = (torch.rand(2, 2, 37, 29, generator=g) * 9).half(), torch.rand(2, 2, 37, 29, generator=g).half()
    for kernel in (1, 3, 5, 7):
        got = bev.centernet_decode(CL(heat.to(DEV)), wh.to(DEV), CL(off.to(DEV)), 200, (148, 117), kernel,
                                   [[1.0, 2.0], [0.0, 3.0]], [[1.5, 1.25, 1.5, 1.25]] * 2, padded=True)
        ref = centernet_decode_torch(heat, wh, off, 200, (148, 117), kernel, [[1.0, 2.0], [0.0, 3.0]],
                                     [[1.5, 1.25, 1.5, 1.25]] * 2)
        _same(got, ref, f"fp16, kernel {kernel}")
    flat = ref[1][0].numpy()
    assert (np.diff(flat[flat > 0]) == 0).any(), "no equal neighbours among the selected scores"


def test_centernet_full_size():
    """80 x 128 x 128 with k = 100 (160 selection chunks), against the torch statement on the CPU: bit for bit."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import centernet_decode_torch
    g = torch.Generator().manual_seed(5)
    heat, off = torch.rand(1, 80, 128, 128, generator=g), torch.rand(1, 2, 128, 128, generator=g)
    wh = torch.rand(1, 2, 128, 128, generator=g) * 20
    args = (100, (512, 512), 3, [[2.0, 6.0]], [[1.6, 1.5, 1.6, 1.5]])
    got = bev.centernet_decode(heat.to(DEV), wh.to(DEV), off.to(DEV), *args, padded=True)
    _same(got, centernet_decode_torch(heat, wh, off, *args), "80 x 128 x 128")
    const = torch.full((1, 80, 128, 128), 0.25)                  # every cell a maximum, every key tied
    got = bev.centernet_decode(const.to(DEV), wh.to(DEV), off.to(DEV), *args, padded=True)
    _same(got, centernet_decode_torch(const, wh, off, *args), "constant 80 x 128 x 128")
    assert got[2].cpu().eq(0).all()                               # the first 100 flat indices: class 0


# ------------------------------------------------------------------------------------------------------ YOLOX
def _check_yolox(boxes, scores, labels, case, what):
    b, s = boxes.cpu().numpy(), scores.cpu().numpy()
    assert U.bits_equal(labels.cpu().numpy(), case["labels"]), f"{what}: labels / prior order"
    ex = case["exact"]
    assert U.bits_equal(b[ex], case["boxes"][ex]), f"{what}: rows without a transcendental (cx, cy) are not exact"
    corner, score = U.yolox_errors(b, s, case)
    print(f"{what}: kernel against float64: corners {corner:.4f} ulp, score {score:.4f} ulp "
          f"(bars {U.BAR_ULP['corner']}, {U.BAR_ULP['score']})")
    assert corner <= U.BAR_ULP["corner"] and score <= U.BAR_ULP["score"], (what, corner, score)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("case", U.yx_cases(), ids=lambda c: c["name"])
def test_yolox_decode_against_fixture(case, layout):
    import bevformer_tensorrt_amd as bev
    cls, box, obj = U.yx_levels(case, device=DEV, channels_last=layout == "channels_last")
    boxes, scores, labels = bev.yolox_decode(cls, box, obj, case["strides"], case["scale"])
    assert boxes.shape == case["boxes"].shape
    _check_yolox(boxes, scores, labels, case, case["name"])


@pytest.mark.parametrize("case", U.yx_cases(), ids=lambda c: c["name"])
def test_yolox_chain_keeps_the_fixture_set(case):
    """decode -> NMS on the device: the fixture conditions make the kept set independent of last-bit differences."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import yolox_get_bboxes
    cls, box, obj = U.yx_levels(case, device=DEV)
    boxes, scores, labels = bev.yolox_decode(cls, box, obj, case["strides"], case["scale"])
    for a in (0, 1):
        got = bev.box_nms(boxes, scores, labels, score_threshold=case["score_thr"], iou_threshold=case["iou_thr"],
                          class_aware=bool(a), max_out=case["max_out"], padded=True)
        want = case["nms"][a]
        _same((got[3], got[4], got[2]), (want[3], want[4], want[2]), f"{case['name']} class_aware={a}: count, index, labels")
        _zero_behind_count(got, case["name"])
        for b, n in enumerate(want[3]):      # kept rows are copies of the decode's rows
            rows = torch.from_numpy(want[4][b, :n].astype(np.int64)).to(DEV)
            assert torch.equal(got[0][b, :n], boxes[b][rows]) and torch.equal(got[1][b, :n], scores[b][rows])
    B = cls[0].shape[0]
    metas = [{"scale_factor": np.asarray(case["scale"][b], np.float32) if case["scale"] is not None else np.ones(4)}
             for b in range(B)]
    res = yolox_get_bboxes(cls, box, obj, metas, rescale=case["scale"] is not None, score_thr=case["score_thr"],
                           iou_threshold=case["iou_thr"], strides=case["strides"], max_out=case["max_out"])
    want = case["nms"][1]
    for b, (det, lab) in enumerate(res):
        n = int(want[3][b])
        assert det.is_cuda and det.shape == (n, 5) and lab.dtype == torch.int64
        assert np.array_equal(lab.cpu().numpy(), want[2][b, :n])
        rows = torch.from_numpy(want[4][b, :n].astype(np.int64)).to(DEV)
        assert torch.equal(det[:, :4], boxes[b][rows]) and torch.equal(det[:, 4], scores[b][rows])


def _full_yolox():
    g = torch.Generator().manual_seed(7)
    shapes = [(80, 80), (40, 40), (20, 20)]                       # 640 x 640: 8 400 priors
    cls = [torch.randn(1, 80, h, w, generator=g) * 2 for h, w in shapes]
    for c in cls:
        c[:, :3] += 4.0                                          # three classes dominate: same-label neighbours overlap
    box = [torch.cat([torch.randn(1, 2, h, w, generator=g), torch.randn(1, 2, h, w, generator=g) * 0.3 + 1.9], 1)
           for h, w in shapes]
    obj = [torch.randn(1, 1, h, w, generator=g) * 2.5 - 2.5 for h, w in shapes]
    return cls, box, obj


def test_yolox_and_nms_full_size():
    """3 levels at 640 x 640 with 80 classes: the decode against float64 at the bars and against the torch statement's
    labels; then bevops_box_nms on the kernel's own 8 400 decoded rows, copied to the host, against `box_nms_torch` on
    those bits: exactly.  8 400 rows are 132 words: the scan stages 32 rows per round."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import box_nms_torch, yolox_decode_torch
    cls, box, obj = _full_yolox()
    scale = [[1.6, 1.5, 1.6, 1.5]]
    dev = lambda ts: [CL(t.to(DEV)) for t in ts]
    boxes, scores, labels = bev.yolox_decode(dev(cls), dev(box), dev(obj), (8, 16, 32), scale)
    assert boxes.shape == (1, 8400, 4)
    rl = yolox_decode_torch(cls, box, obj, (8, 16, 32), scale)[2]
    truth = U.np_yolox([t.numpy() for t in cls], [t.numpy() for t in box], [t.numpy() for t in obj], (8, 16, 32), scale)
    assert (truth["top2"] > 0).all() and np.array_equal(rl.numpy(), truth["labels"])
    truth["exact"][:] = False
    _check_yolox(boxes, scores, labels, truth, "8 400 x 80")
    hb, hs, hl = boxes.cpu(), scores.cpu(), labels.cpu()
    for aware, max_out in ((True, None), (False, 300)):
        got = bev.box_nms(boxes, scores, labels, score_threshold=0.01, iou_threshold=0.65, class_aware=aware,
                          max_out=max_out, padded=True)
        ref = box_nms_torch(hb, hs, hl, score_threshold=0.01, iou_threshold=0.65, class_aware=aware, max_out=max_out)
        _same(got, ref, f"box_nms on 8 400 rows, class_aware={aware}")
        ncand, kept = int((hs >= 0.01).sum()), int(ref[3][0])
        print(f"8 400 rows: {ncand} candidates, {kept} kept (class_aware={aware}, max_out={max_out})")
        assert 0 < kept < ncand < 8400


# ------------------------------------------------------------------------------------------------------ box NMS
@pytest.mark.parametrize("case", U.nm_cases(), ids=lambda c: c["name"])
def test_box_nms_equals_fixture_and_torch_statement(case):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.postprocess import box_nms_torch
    kw = dict(score_threshold=case["score_thr"], iou_threshold=case["iou_thr"], class_aware=bool(case["aware"]),
              max_out=case["max_out"])
    got = bev.box_nms(T(case["boxes"]), T(case["scores"]), T(case["labels"]), T(case["count"]), **kw, padded=True)
    _same(got, case["want"], case["name"])
    ref = box_nms_torch(*[None if case[k] is None else torch.from_numpy(case[k]) for k in ("boxes", "scores", "labels", "count")],
                        **kw)
    _same(got, ref, case["name"] + " against the torch statement")
    _zero_behind_count(got, case["name"])
    dicts = bev.box_nms(T(case["boxes"]), T(case["scores"]), T(case["labels"]), T(case["count"]), **kw)
    assert [d["index"].numel() for d in dicts] == case["want"][3].tolist()


@pytest.mark.parametrize("case", U.yx_cases(), ids=lambda c: c["name"])
def test_box_nms_on_fixture_decodes(case):
    import bevformer_tensorrt_amd as bev
    for a in (0, 1):
        got = bev.box_nms(T(case["boxes"]), T(case["scores"]), T(case["labels"]), score_threshold=case["score_thr"],
                          iou_threshold=case["iou_thr"], class_aware=bool(a), max_out=case["max_out"], padded=True)
        _same(got, case["nms"][a], f"{case['name']} class_aware={a}")


# ------------------------------------------------------------------------------------------------------ call contract
def _contract_inputs():
    cn = next(c for c in U.cn_cases() if c["name"] == "cn_ragged")
    yx = next(c for c in U.yx_cases() if c["name"] == "yx_b2")
    nm = next(c for c in U.nm_cases() if c["name"] == "nm_count_b2")
    return cn, yx, nm


def _run_all(bev, cn_maps, cn, yx_levels, yx, nm_in, nm):
    a = bev.centernet_decode(*cn_maps, cn["k"], cn["inp"], cn["kernel"], cn["border"], cn["scale"], score_threshold=0.5,
                             padded=True)
    b = bev.yolox_decode(*yx_levels, yx["strides"], yx["scale"])
    c = bev.box_nms(*b, score_threshold=yx["score_thr"], iou_threshold=yx["iou_thr"], padded=True)
    d = bev.box_nms(*nm_in, score_threshold=nm["score_thr"], iou_threshold=nm["iou_thr"], class_aware=bool(nm["aware"]),
                    max_out=nm["max_out"], padded=True)
    return tuple(a) + tuple(b) + tuple(c) + tuple(d)


def test_entries_are_capturable_and_bit_reproducible():
    import bevformer_tensorrt_amd as bev
    cn, yx, nm = _contract_inputs()
    cn_maps = _cn_args(cn)
    yx_levels = U.yx_levels(yx, device=DEV)
    nm_in = [T(nm[k]) for k in ("boxes", "scores", "labels", "count")]
    run = lambda: _run_all(bev, cn_maps, cn, yx_levels, yx, nm_in, nm)
    first, second = run(), run()
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.equal(x, y) or U.bits_equal(x.cpu().numpy(), y.cpu().numpy())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    replays = []
    for _ in range(2):
        for t in captured:
            t.fill_(7)                                           # a replay must rewrite every output byte
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in captured])
    for x, y, z in zip(first, replays[0], replays[1]):
        assert U.bits_equal(x.cpu().numpy(), y.cpu().numpy()) and U.bits_equal(y.cpu().numpy(), z.cpu().numpy())
    # the replay follows inputs changed in place
    cn_maps[0].copy_(torch.flip(cn_maps[0], dims=(3,)))
    nm_in[1].copy_(torch.flip(nm_in[1], dims=(1,)))
    graph.replay()
    torch.cuda.synchronize()
    eager = run()
    changed = 0
    for x, y, z in zip(captured, eager, first):
        assert U.bits_equal(x.cpu().numpy(), y.cpu().numpy())
        changed += not U.bits_equal(x.cpu().numpy(), z.cpu().numpy())
    assert changed > 0
    _zero_behind_count(eager[0:4], "centernet")
    _zero_behind_count(eager[7:12], "box_nms after yolox")
    _zero_behind_count(eager[12:17], "box_nms")


def test_c_abi_direct_and_domain():
    """bevops_centernet_decode with raw pointers into pre-filled outputs, and the unsupported domains through the
    wrappers."""
    import ctypes
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    lib = L.load_library()
    c = next(c for c in U.cn_cases() if c["name"] == "cn_b2")
    heat, wh, off = _cn_args(c)
    B, C, H, W = heat.shape
    k = c["k"]
    boxes = torch.full((B, k, 4), 7.0, device=DEV)
    scores = torch.full((B, k), 7.0, device=DEV)
    labels = torch.full((B, k), 7, device=DEV, dtype=torch.int32)
    count = torch.full((B,), 7, device=DEV, dtype=torch.int32)
    need = lib.bevops_centernet_decode_workspace_size(B, C, H, W, k)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = lib.bevops_centernet_decode(0, heat.data_ptr(), wh.data_ptr(), off.data_ptr(),
                                     (ctypes.c_int32 * 6)(H * W, 1, H * W, 1, H * W, 1), boxes.data_ptr(), scores.data_ptr(),
                                     labels.data_ptr(), count.data_ptr(), B, C, H, W, k, c["kernel"], c["inp"][0], c["inp"][1],
                                     (ctypes.c_float * 4)(*c["border"].reshape(-1).tolist()),
                                     (ctypes.c_float * 8)(*c["scale"].reshape(-1).tolist()), -1.0, ws.data_ptr(), need,
                                     L.current_stream_ptr(heat.device))
    assert st == 0
    torch.cuda.synchronize()
    _same((boxes, scores, labels, count), [c[key] for key in ("boxes", "scores", "labels", "count")], "C ABI")
    z = torch.zeros(1, 3, 8, 12, device=DEV)
    z2 = torch.zeros(1, 2, 8, 12, device=DEV)
    for kwargs, status in ((dict(k=289), L.NOT_SUPPORTED), (dict(k=10, kernel=4), L.NOT_SUPPORTED)):
        with pytest.raises(L.BevopsError) as e:
            bev.centernet_decode(z, z2, z2, kwargs["k"], (32, 48), kwargs.get("kernel", 3))
        assert e.value.status == status
    with pytest.raises(L.BevopsError) as e:
        bev.box_nms(torch.zeros(1, 16385, 4, device=DEV), torch.zeros(1, 16385, device=DEV),
                    torch.zeros(1, 16385, device=DEV, dtype=torch.int32), iou_threshold=0.5)
    assert e.value.status == L.NOT_SUPPORTED
    with pytest.raises(L.BevopsError) as e:
        bev.yolox_decode([z.to(torch.int8)], [torch.zeros(1, 4, 8, 12, device=DEV, dtype=torch.int8)],
                         [torch.zeros(1, 1, 8, 12, device=DEV, dtype=torch.int8)], (8,))
    assert e.value.status == L.NOT_SUPPORTED


# ------------------------------------------------------------------------------------------------------ buffer contract
def test_entries_in_the_guarded_arena(monkeypatch):
    """The three entries at the fixtures' tail shapes (9 000 cells: a full and a ragged selection chunk; ragged YOLOX
    levels; 65 rows = a word and one row; counts below N) with inputs, outputs and scratch in the guarded arena: scratch
    exactly the size query's bytes at 8-byte alignment, both poisons, guards intact, equal bits under both poisons and
    equal to the ordinary call."""
    from test_buffer_contract_gpu import fmod, wrapper_contract
    from bevformer_tensorrt_amd.utils import lib as L
    lib = L.load_library()
    mod = fmod("decode2d")
    for name, cl in (("cn_ragged", False), ("cn_b2", True)):
        c = next(c for c in U.cn_cases() if c["name"] == name)
        heat, wh, off = _cn_args(c, cl)
        need = lib.bevops_centernet_decode_workspace_size(*heat.shape, c["k"])
        plain = wrapper_contract(monkeypatch, [mod], lambda heat, wh, off: mod.centernet_decode(
            heat, wh, off, c["k"], c["inp"], c["kernel"], c["border"], c["scale"], padded=True),
            dict(heat=heat, wh=wh, off=off), ws_align=8, scratch_sizes=[need])
        _same(plain, [c[k] for k in ("boxes", "scores", "labels", "count")], name + " in the arena")
    y = next(c for c in U.yx_cases() if c["name"] == "yx_ragged")
    cls, box, obj = U.yx_levels(y, device=DEV)
    L_ = len(cls)
    inputs = {f"{n}{l}": t for n, ts in (("cls", cls), ("box", box), ("obj", obj)) for l, t in enumerate(ts)}
    plain = wrapper_contract(monkeypatch, [mod], lambda **m: mod.yolox_decode(
        [m[f"cls{l}"] for l in range(L_)], [m[f"box{l}"] for l in range(L_)], [m[f"obj{l}"] for l in range(L_)],
        y["strides"], y["scale"]), inputs, scratch_sizes=[])
    _check_yolox(*plain, y, "yx_ragged in the arena")
    for name in ("nm_n65", "nm_count_b2"):
        c = next(c for c in U.nm_cases() if c["name"] == name)
        B, N = c["scores"].shape
        need = lib.bevops_box_nms_workspace_size(B, N)
        inputs = dict(boxes=T(c["boxes"]), scores=T(c["scores"]), labels=T(c["labels"]))
        if c["count"] is not None:
            inputs["count"] = T(c["count"])
        plain = wrapper_contract(monkeypatch, [mod], lambda boxes, scores, labels, count=None: mod.box_nms(
            boxes, scores, labels, count, score_threshold=c["score_thr"], iou_threshold=c["iou_thr"],
            class_aware=bool(c["aware"]), max_out=c["max_out"], padded=True), inputs, ws_align=8, scratch_sizes=[need])
        _same(plain, c["want"], name + " in the arena")
