"""BEVDet for B samples per call: BEVDet.forward_calibrated(image [B, N, 3, H, W], calib [B, N * 24 + 9]) in both
bev_half modes and in INT8, and BEVDetRunner(batch=B).  Synthetic weights, 256 x 704, a different jittered rig per sample.

* sample independence, exact: replacing one sample's image and calibration leaves the other sample's six outputs
  bit-equal (fp16 "hip", "torch", INT8 bev_half="int8");
* against batch 1: per sample and head, the rms error of the batched "hip" run against the fp32 plain path (`forward` in
  fp32 on that sample's own ranks) is at most 1.25 x the batch-1 "hip" run's (the project's margin for "same arithmetic,
  possibly another kernel": the rule dispatch reads the row count, so another GEMM may serve B * 6 images; bit-equality
  with batch 1 is printed, not asserted).  INT8: per sample the 1.25 x gate of tests/test_bevdet_int8_gpu.py against the
  fake-quant statement;
* BEVDetRunner(batch=2, post="bboxes"): step and step_raw replay bit-equal to the eager batched path, a changed
  calibration needs no new capture, per sample count and boxes equal get_bboxes on that sample's head slices, the decode
  reads the packed head output in place, the capture guard, the wrong-B ValueError;
* the default runner keeps the bits of forward_calibrated with a 1-D calib."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("reg", "height", "dim", "rot", "vel", "heatmap")
MARGIN = 1.25


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _by_rule(fn, *args):
    from bevformer_tensorrt_amd.functions import dispatch
    with dispatch.using(rule=True):
        return fn(*args)


@pytest.fixture(scope="module")
def S():
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    hip = BEVDet(seed=0, bev_half="hip").cuda().half()
    view = hip.view
    rigs = [jittered_rig(view, k) for k in (1, 2, 3, 4)]
    stack = lambda idx: tuple(None if i == 1 else torch.cat([rigs[k][i] for k in idx], 0) for i in range(6))
    rows = view.calibration_matrices_batched(*stack(range(4)))
    img = torch.randn(4, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    return dict(hip=hip, view=view, rigs=rigs, stack=stack, rows=rows, calib=rows.cuda(), img=img)


@pytest.fixture(scope="module")
def int8_model(S):
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    view = S["view"]
    ranks = [r.cuda() for r in view.prepare_stable(view.lidar_coor_plain(S["rows"][0]))]
    gen = torch.Generator().manual_seed(2)
    frames = [(torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(), *ranks) for _ in range(2)]
    model, _, _ = build_int8_bevdet(S["hip"], "cuda", frames, "minmax", bev_half="int8")
    return model


def _model(S, request, mode):
    if mode == "hip":
        return S["hip"]
    if mode == "torch":
        from bevformer_tensorrt_amd.bevdet import BEVDet
        return BEVDet(seed=0, bev_half="torch").cuda().half()
    return request.getfixturevalue("int8_model")


@pytest.mark.parametrize("mode", ["hip", "torch", "int8"])
def test_samples_are_independent_bit_for_bit(S, request, mode):
    model = _model(S, request, mode)
    img, calib = S["img"], S["calib"]
    run = lambda idx: [o.clone() for o in _by_rule(model.forward_calibrated, img[idx], calib[idx])]
    ab, cb, ac = run([0, 1]), run([2, 1]), run([0, 2])
    for name, p, q, r in zip(NAMES, ab, cb, ac):
        assert p.shape[0] == 2 and p.shape[2:] == (128, 128)
        assert _bits(p[1], q[1]), f"{mode} {name}: sample 1 changed with sample 0"
        assert _bits(p[0], r[0]), f"{mode} {name}: sample 0 changed with sample 1"
        assert not _bits(p[0], q[0]) and not _bits(p[1], r[1])          # (the replaced sample did change)
        assert float(p.float().abs().max()) > 0 and bool(torch.isfinite(p.float()).all())


@pytest.mark.parametrize("idx", [[0, 1], [3, 1, 2]], ids=["B2", "B3"])
def test_batched_hip_against_batch_one(S, idx):
    from bevformer_tensorrt_amd.bevdet import BEVDet
    hip, view, img, calib = S["hip"], S["view"], S["img"], S["calib"]
    plain = BEVDet(seed=0, bev_half="torch").cuda().float()
    batched = hip.forward_calibrated(img[idx], calib[idx])
    equal = 0
    for b, k in enumerate(idx):
        ranks = [r.cuda() for r in view.prepare_stable(view.lidar_coor_plain(S["rows"][k]))]
        ref = plain(img[k:k + 1].float(), *ranks)
        single = hip.forward_calibrated(img[k:k + 1], calib[k])
        for name, g, s, r in zip(NAMES, batched, single, ref):
            e_b, e_1 = _rms(g[b:b + 1].float(), r), _rms(s.float(), r)
            same = _bits(g[b:b + 1], s)
            equal += same
            print(f"B = {len(idx)}, sample {b} (rig {k}), {name}: rms error batched {e_b:.4e}, batch 1 {e_1:.4e}, "
                  f"ratio {e_b / e_1:.4f}, bit-equal to batch 1: {same}")
            assert e_1 > 0 and e_b <= MARGIN * e_1, (b, name)
    print(f"B = {len(idx)}: {equal} of {6 * len(idx)} maps bit-equal to their batch-1 run")


def test_batched_int8_holds_the_gate_per_sample(S, int8_model):
    model, view = int8_model, S["view"]
    idx = [0, 1]
    x = model._features(S["img"][idx]).clone()
    got = model.bev_half_calibrated(x, S["calib"][idx])
    for b, k in enumerate(idx):
        ranks = [r.cuda() for r in view.prepare_stable(view.lidar_coor_plain(S["rows"][k]))]
        xb = x[b * 6:(b + 1) * 6]
        fq = model.fake_quant_reference(xb, ranks)
        ref = model.fake_quant_reference(xb, ranks, quantize=False)
        for name, g, f, r in zip(NAMES, got, fq, ref):
            e_k, e_f = _rms(g[b:b + 1].float(), r), _rms(f, r)
            print(f"INT8, sample {b}, {name}: rms error kernels {e_k:.4e}, fake-quant statement {e_f:.4e}, "
                  f"ratio {e_k / e_f:.4f}")
            assert e_f > 0 and e_k <= MARGIN * e_f, (b, name)


@pytest.fixture
def decode_probe(monkeypatch):
    """records (entry name, the six map pointers) of every CenterPoint decode call"""
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    calls = []
    for name in ("bevops_centerpoint_decode", "bevops_centerpoint_decode_ex"):
        real = getattr(handle, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append((_name, tuple(args[1:7])))
            return _real(*args)
        monkeypatch.setattr(handle, name, wrapped)
    return calls


def test_runner_batch_two_with_bboxes(S, decode_probe):
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDetRunner
    model, img, calib, stack = S["hip"], S["img"], S["calib"], S["stack"]
    sets = {"A": [0, 1], "B": [2, 0]}

    def eager(idx):
        out = model.forward_calibrated(img[:2], calib[idx])
        n = len(decode_probe)
        post = tuple(model.get_bboxes(out, padded=True))
        assert len(decode_probe) == n + 1
        name, ptrs = decode_probe[-1]
        assert name == "bevops_centerpoint_decode_ex"
        assert list(ptrs) == [o.data_ptr() for o in out], "a head map was copied in front of the decode"
        return [t.clone() for t in out + post]
    want = {k: eager(idx) for k, idx in sets.items()}
    runner = BEVDetRunner(model, torch.device("cuda"), graph=True, post="bboxes", batch=2)
    order = "ABBA"
    frames = [runner.step(img[:2], *stack(sets[k])) for k in order]
    graph = runner._graph
    torch.cuda.synchronize()
    assert graph is not None and runner._graph is graph and runner._graph_raw is None
    assert tuple(runner.image_buffer.shape) == (2, 6, 3, 256, 704) and tuple(runner._in["calib"].shape) == (2, 6 * 24 + 9)
    for k, got in zip(order, frames):
        assert len(got) == len(want[k]) == 11
        for a, b in zip(got, want[k]):
            assert _bits(a, b), k
    assert not _bits(frames[0][0], frames[1][0])                       # the calibration changed the frame
    out = want["A"]
    boxes, scores, labels, count, index = out[6:]
    assert tuple(boxes.shape) == (2, 500, 9) and tuple(count.shape) == (2,)
    for b in range(2):
        one = model.get_bboxes([o[b:b + 1] for o in out[:6]], padded=True)
        assert decode_probe[-1][0] == "bevops_centerpoint_decode"      # (one sample: the plain entry, as before)
        n = int(count[b])
        assert n == int(one[3][0]) and n > 0
        for a, c in zip((boxes, scores, labels, index), (one[0], one[1], one[2], one[4])):
            assert _bits(a[b:b + 1], c)
    # wrong B
    with pytest.raises(ValueError):
        runner.step(img[:1], *stack([0]))
    with pytest.raises(ValueError):
        runner.step(img[:3], *stack([0, 1, 2]))
    with pytest.raises(ValueError):
        runner.step(img[:3], *stack([0, 1]))
    # the capture guard: missing merged operands raise under capture before anything is launched
    fresh = BEVDet(seed=3, bev_half="hip").cuda().half()
    scratch = torch.zeros(8, device="cuda")
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            fresh.forward_calibrated(img[:2], calib[:2])
    del g2


def test_runner_batch_two_from_raw_frames(S):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, stack = S["hip"], S["stack"]
    raw = torch.randint(0, 256, (2, 6, 900, 1600, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    pick = lambda idx: (lambda r: (r[0], None, r[2], r[5]))(stack(idx))
    want = {}
    for k, idx in (("A", [0, 1]), ("B", [1, 3])):
        e = BEVDetRunner(model, "cuda", graph=False, post="bboxes", raw_size=(900, 1600), batch=2)
        want[k] = [t.clone() for t in e.step_raw(raw, *pick(idx))]
    runner = BEVDetRunner(model, "cuda", graph=True, post="bboxes", raw_size=(900, 1600), batch=2)
    frames = [(k, runner.step_raw(raw, *pick(idx))) for k, idx in (("A", [0, 1]), ("B", [1, 3]), ("A", [0, 1]))]
    graph = runner._graph_raw
    torch.cuda.synchronize()
    assert graph is not None and runner._graph is None
    assert tuple(runner.raw_buffer.shape) == (12, 900, 1600, 3)
    for k, got in frames:
        for a, b in zip(got, want[k]):
            assert _bits(a, b), k
    # each sample's image is what the one-sample runner prepares from that sample's frames
    one = BEVDetRunner(model, "cuda", graph=False, raw_size=(900, 1600))
    r0 = stack([0])
    one.step_raw(raw[1], r0[0], None, r0[2], r0[5])
    assert _bits(one.image_buffer[0], runner.image_buffer[1])
    with pytest.raises(ValueError):
        runner.step_raw(raw[0], *pick([0, 1]))
    with pytest.raises(ValueError):
        runner.step_raw(raw, *pick([0]))


def test_default_runner_is_unchanged(S):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    model, img, view = S["hip"], S["img"], S["view"]
    rig = S["rigs"][1]
    calib = view.calibration_matrices(*rig).cuda()
    assert calib.dim() == 1 and torch.equal(calib, S["calib"][1])
    want = [o.clone() for o in model.forward_calibrated(img[1:2], calib)]
    for kw in ({}, {"batch": 1}):
        runner = BEVDetRunner(model, torch.device("cuda"), graph=True, **kw)
        assert runner.batch == 1
        for _ in range(2):
            got = runner.step(img[1:2], *rig)
        torch.cuda.synchronize()
        assert runner._in["calib"].dim() == 1 and tuple(runner.image_buffer.shape) == (1, 6, 3, 256, 704)
        for name, a, b in zip(NAMES, got, want):
            assert _bits(a, b) and a.shape == (1, a.shape[1], 128, 128), name
