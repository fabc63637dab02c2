"""The INT8 build of YOLOX (quantization.build_int8_yolox, yolox_int8.py) on the GPU, YOLOX_S at [1, 3, 64, 64] and
[2, 3, 96, 128]:

* per-call replay: a recording operator set captures the arguments and the result of every conv_slice_q_taps, Focus,
  pool and up-sampling call of one forward; each call is checked against its own float64 statement from the int8 inputs
  the kernel actually received (tests/util_conv_slice_s8.py: equality for act none, the derived near-tie interval for
  SiLU; the data movers exactly) -- every layer got the right scales, slices and identity;
* buffer and scale consistency from the recorded calls: every channel is written before it is read, and read with the
  scale its writer used;
* model level: against the fp32 plain path, the int8 path's error is at most 1.25 x the error of the torch fp32
  fake-quant statement of the same plan (Int8YOLOX.fake_quant_reference: independent of the kernels).  The error is
  the root mean square over an output (single-step tie flips at well under 1 % of the elements, the only legitimate
  difference, do not move it by a quarter; the maximum of one output can hang on one flip, so it is printed, not
  gated).  The position against the 3e-2 model bar is printed, not gated: a random-weight network is no checkpoint;
* two eager runs and the YOLOXRunner replay give equal bits; capture guard; weight reload; get_bboxes;
* no library convolution, no torch.cat and no dtype conversion on the int8 path;
* the fp16 YOLOX built beside the int8 model gives the bits it gave before, and the plan run on the fp16 operators gives
  YOLOX.forward's bits."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_conv_slice_s8 as S

pytestmark = pytest.mark.gpu

CASES = ((1, 3, 64, 64), (2, 3, 96, 128))
NAMES = tuple(f"{n}_{l}" for n in ("cls_score", "bbox_pred", "objectness") for l in (1, 2, 3))
BAR = 3e-2
ACT_CODE = {None: 0, "none": 0, "relu": 1, "silu": 2}


def _bits(t):
    return t.contiguous().view(torch.int16)


class Recorder:
    """The operator set of an Int8YOLOX that records every call: (name, arguments, result), tensors kept alive (so that
    no buffer's address is reused within a forward) and copied to the host on demand."""

    def __init__(self):
        import bevformer_tensorrt_amd.functions as fn
        self.fn, self.calls = fn, []

    def conv_slice_q_taps(self, x_q, scale_x, w_q_taps, w_scales, bias, act, residual_q=None, scale_res=1.0, stride=1,
                          out=None, scale_out=None, out_dtype=torch.int8):
        res_before = None if residual_q is None else residual_q.clone()      # (out may BE the identity)
        r = self.fn.conv_slice_q_taps(x_q, scale_x, w_q_taps, w_scales, bias, act, residual_q, scale_res, stride, out,
                                      scale_out, out_dtype)
        self.calls.append(("conv", dict(x=x_q, sx=scale_x, w=w_q_taps, ws=w_scales, b=bias, act=act, res=residual_q,
                                        res_before=res_before, sr=scale_res, stride=stride, so=scale_out, out=r)))
        return r

    def focus_nhwc_q(self, image, scale, out=None):
        r = self.fn.focus_nhwc_q(image, scale, out)
        self.calls.append(("focus", dict(image=image, scale=scale, out=r)))
        return r

    def spp_maxpool_nhwc(self, x, out=None, kernel_sizes=(5, 9, 13)):
        r = self.fn.spp_maxpool_nhwc(x, out, kernel_sizes)
        self.calls.append(("pool", dict(x=x, out=r, ks=tuple(kernel_sizes))))
        return r

    def upsample_nearest2x_nhwc(self, x, out=None):
        r = self.fn.upsample_nearest2x_nhwc(x, out)
        self.calls.append(("up", dict(x=x, out=r)))
        return r


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


@pytest.fixture(scope="module")
def built():
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    dev = torch.device("cuda")
    base = YOLOX(YOLOX_S, seed=0, ops=types.SimpleNamespace())
    ref32 = copy.deepcopy(base).cuda()
    fp = base.cuda().half()
    fp.ops = fn
    ref32.load_state_dict({k: v.float() for k, v in fp.state_dict().items()})
    g = torch.Generator().manual_seed(11)
    images = {c: torch.randn(c, generator=g).cuda().half() for c in CASES}
    before = {c: tuple(o.clone() for o in fp(images[c])) for c in CASES}       # the fp16 model's bits BEFORE the build
    frames = [torch.randn(c, generator=g).cuda().half() for c in CASES] + list(images.values())
    model, note = Q.build_int8_yolox(fp, dev, frames, calibrator="minmax")
    ref = {c: tuple(o.clone() for o in ref32(images[c].float())) for c in CASES}
    return dict(fp=fp, model=model, note=note, images=images, before=before, ref=ref, frames=frames)


def test_note_and_scales(built):
    assert built["note"] == {"int8_layers": 74, "scale_groups": 57, "calibration_frames": 4}
    s = built["model"].group_scales
    assert len(s) == 57 and all(0 < v < 1e3 for v in s)


@pytest.fixture(scope="module")
def recorded(built):
    """One recorded forward per case."""
    model, out = built["model"], {}
    for c in CASES:
        rec = Recorder()
        model.ops = rec
        try:
            outs = model(built["images"][c])
            torch.cuda.synchronize()
        finally:
            model.ops = rec.fn
        out[c] = (rec.calls, tuple(o.clone() for o in outs))
    return out


@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_call_against_its_own_statement(recorded, case):
    calls, _ = recorded[case]
    assert [n for n, _ in calls].count("conv") == 74 and [n for n, _ in calls].count("pool") == 1
    assert [n for n, _ in calls].count("up") == 2 and calls[0][0] == "focus"
    shares, kinds = [], {"silu": 0, "none": 0}
    for i, (name, a) in enumerate(calls):
        if name == "focus":
            img = a["image"].float().cpu().numpy().astype(np.float32)
            inv = np.float32(1.0) / np.float32(a["scale"])
            q = np.clip(np.rint((img * inv).astype(np.float32)), -127, 127).astype(np.int8)
            tl, tr, bl, br = q[..., ::2, ::2], q[..., ::2, 1::2], q[..., 1::2, ::2], q[..., 1::2, 1::2]
            got = _nhwc(a["out"])
            assert np.array_equal(got[..., :12], np.concatenate((tl, bl, tr, br), axis=1).transpose(0, 2, 3, 1))
            assert not got[..., 12:].any() and got.dtype == np.int8
        elif name == "pool":
            x = a["x"].float()
            want = torch.cat([F.max_pool2d(x, k, 1, k // 2) for k in a["ks"]], dim=1)
            assert a["out"].dtype == torch.int8 and torch.equal(a["out"].float(), want)
        elif name == "up":
            assert a["out"].dtype == torch.int8
            assert torch.equal(a["out"], a["x"].repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))
        else:
            x, w = _nhwc(a["x"]), a["w"].cpu().numpy()
            k = w.shape[1]
            acc = S.sums(x, w, k, a["stride"])
            ws, b = a["ws"].cpu().numpy(), a["b"].cpu().numpy()
            res = None if a["res"] is None else _nhwc(a["res_before"])
            got = _nhwc(a["out"])
            act = ACT_CODE[a["act"]]
            kinds["silu" if act == 2 else "none"] += 1
            if act == 2:
                assert got.dtype == np.int8
                _, _, lo, hi = S.silu_interval(acc, a["sx"], 1.0, ws, b, res, a["sr"], a["so"])
                shares.append(S.check_interval(got, lo, hi))
            else:
                out = "int8" if got.dtype == np.int8 else "fp16"
                want = S.exact_output(acc, a["sx"], 1.0, ws, b, act, res, a["sr"], a["so"], out)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"call {i}"
    assert kinds == {"silu": 71, "none": 3}
    print(f"{case}: share of outputs within delta of a half-integer per SiLU layer: max {max(shares):.4%}, "
          f"mean {np.mean(shares):.4%}")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_buffers_are_written_before_read_with_one_scale(built, recorded, case):
    calls, _ = recorded[case]
    written = {}                                    # storage address -> {channel: scale its writer used}

    def key(t):
        return t.untyped_storage().data_ptr(), t.storage_offset(), t.shape[1]

    def read(t, scale, what):
        buf, c0, C = key(t)
        have = written.get(buf, {})
        for ch in range(c0, c0 + C):
            assert ch in have, f"{what}: channel {ch} read before it was written"
            assert scale is None or have[ch] == scale, f"{what}: channel {ch} written with {have[ch]}, read with {scale}"
        return {have[ch] for ch in range(c0, c0 + C)}

    def write(t, scale):
        buf, c0, C = key(t)
        assert t.dtype == (torch.float16 if scale is None else torch.int8)
        written.setdefault(buf, {}).update({ch: scale for ch in range(c0, c0 + C)})

    for i, (name, a) in enumerate(calls):
        if name == "focus":
            write(a["out"], a["scale"])
        elif name == "conv":
            read(a["x"], a["sx"], f"call {i} x")
            if a["res"] is not None:
                read(a["res"], a["sr"], f"call {i} identity")
            write(a["out"], a["so"])
        else:                                       # the data movers keep their input's scale
            scales = read(a["x"], None, f"call {i} {name}")
            assert len(scales) == 1
            write(a["out"], scales.pop())
    # every buffer complete, and the scales in use are the model's group scales
    used = set()
    for buf, chans in written.items():
        assert sorted(chans) == list(range(len(chans)))
        used |= {s for s in chans.values() if s is not None}
    assert used <= set(built["model"].group_scales)
    assert len(written) == 62                       # the plan's buffers: 59 int8, 3 packed fp16 outputs


@pytest.mark.parametrize("case", CASES, ids=str)
def test_int8_path_is_as_close_to_fp32_as_its_fake_quant_statement(built, recorded, case):
    model, img = built["model"], built["images"][case]
    got = recorded[case][1]
    emu = model.fake_quant_reference(img)
    B, _, H, W = case
    for i, (name, g, e, r) in enumerate(zip(NAMES, got, emu, built["ref"][case])):
        s = (8, 16, 32)[i % 3]
        assert g.shape == (B, (80, 4, 1)[i // 3], H // s, W // s) and g.dtype == torch.float16 and e.dtype == torch.float32
        rms = lambda t: float((t.double() - r.double()).pow(2).mean().sqrt())    # noqa: E731
        mx = lambda t: float((t.float() - r).abs().max())                        # noqa: E731
        bar = BAR * max(1.0, float(r.abs().max()))
        flips = float((g.float() - e).abs().gt(1e-3 * float(r.abs().max())).float().mean())
        print(f"{case} {name}: |ref|max {float(r.abs().max()):.3f}; rms error int8 {rms(g):.4e}, fake-quant {rms(e):.4e} "
              f"(ratio {rms(g) / rms(e):.3f}); max error int8 {mx(g):.4e}, fake-quant {mx(e):.4e}, bar {bar:.3e} "
              f"(int8 at {mx(g) / bar:.2f} of it); {flips:.2%} of the elements differ from the fake-quant statement")
        assert float(r.max() - r.min()) > 1e-3 and rms(e) > 0
        assert rms(g) <= 1.25 * rms(e), name


@pytest.mark.parametrize("case", CASES, ids=str)
def test_two_runs_and_the_replay_give_equal_bits(built, recorded, case):
    from bevformer_tensorrt_amd.yolox import YOLOXRunner, num_priors
    model, img = built["model"], built["images"][case]
    a = recorded[case][1]
    b = model(img)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    runner = YOLOXRunner(model, case[0], *case[2:])
    for _ in range(2):
        out = runner.step(img)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, runner.head_outputs):
        assert torch.equal(_bits(x), _bits(y)), name
    assert len(out) == 4 and out[0].shape == (case[0], num_priors(*case[2:]), 4) and out[3].dtype == torch.int32
    metas = [dict(scale_factor=[0.5, 0.5, 0.5, 0.5]) for _ in range(case[0])]
    boxes = model.get_bboxes(b, metas, rescale=True)
    assert len(boxes) == case[0] and all(bb.shape[1] == 5 and ll.dtype == torch.int64 for bb, ll in boxes)
    assert sum(bb.shape[0] for bb, _ in boxes) > 0 and sum(bb.shape[0] for bb, _ in boxes) == int(out[3].sum())


class _Counter:
    """Monkey-patch probes (the style of tests/test_yolox_gpu.py): the library entries of the plain path, and the
    dtype conversions."""
    NAMES = (("conv2d", F), ("max_pool2d", F), ("interpolate", F), ("silu", F), ("sigmoid", torch), ("cat", torch),
             ("to", torch.Tensor), ("half", torch.Tensor), ("float", torch.Tensor), ("char", torch.Tensor),
             ("type", torch.Tensor))

    def __init__(self, monkeypatch):
        self.counts = {n: 0 for n, _ in self.NAMES}
        for name, mod in self.NAMES:
            monkeypatch.setattr(mod, name, self._wrap(name, getattr(mod, name)))

    def _wrap(self, name, inner):
        def probe(*args, **kwargs):
            self.counts[name] += 1
            return inner(*args, **kwargs)
        return probe


def test_no_library_call_no_concatenation_no_conversion_on_the_int8_path(built, monkeypatch):
    from bevformer_tensorrt_amd.functions import conv as C
    model, img = built["model"], built["images"][CASES[1]]
    model(img)
    misses = list(C.CONV_MISSES)
    counter = _Counter(monkeypatch)
    outs = model(img)
    torch.cuda.synchronize()
    print("int8:", counter.counts)
    assert counter.counts == {n: 0 for n, _ in _Counter.NAMES}
    assert C.CONV_MISSES == misses and len(outs) == 9
    model.fake_quant_reference(img)                          # the probes see the torch statement
    assert counter.counts["conv2d"] == 74 and counter.counts["cat"] >= 2


def test_fp16_model_keeps_its_bits_and_the_plan_is_its_fast_path(built):
    from bevformer_tensorrt_amd import yolox_int8 as YI
    import bevformer_tensorrt_amd.functions as fn
    fp = built["fp"]
    assert built["model"].fp is fp
    for c in CASES:
        again = fp(built["images"][c])
        packed = YI.run_plan(built["model"].plan, built["images"][c], "fp16", fn, fp.operands())
        via_plan = YI.split_outputs(packed, fp.operands()["slices"])
        for name, x, y, z in zip(NAMES, built["before"][c], again, via_plan):
            assert torch.equal(_bits(x), _bits(y)), name
            assert torch.equal(_bits(x), _bits(z)), name


def test_capture_guard_weight_reload_and_device_calibrator_cache(built, tmp_path):
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd import yolox_int8 as YI
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    fp = YOLOX(YOLOX_S, seed=3).cuda().half()
    img = built["images"][CASES[0]]
    path = str(tmp_path / "yolox_s.npz")
    model, note = Q.build_int8_yolox(fp, torch.device("cuda"), [img], calibrator="entropy_device", calibration_cache=path)
    assert note["calibration_frames"] == 1
    again, note2 = Q.build_int8_yolox(fp, torch.device("cuda"), [], calibrator="entropy_device", calibration_cache=path)
    assert note2["calibration_frames"] == 0 and again.group_scales == model.group_scales
    # the capture guard raises before anything is launched when the quantised operands are missing
    assert model.operands(build=False) is None
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)
        with pytest.raises(RuntimeError):
            model.prepare()
    del graph
    eager = [o.clone() for o in model(img)]
    ops0 = model.operands(build=False)
    assert ops0 is not None
    # new weights: level 2's objectness predictor becomes the constant 0.5; the int8 operands are stale and rebuilt
    with torch.no_grad():
        fp.bbox_head.conv_obj[1].weight.zero_()
        fp.bbox_head.conv_obj[1].bias.fill_(0.5)
    assert model.operands(build=False) is None
    new = model(img)
    assert model.operands(build=False) is not ops0 and bool((new[7] == 0.5).all())
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        assert torch.equal(_bits(new[i]), _bits(eager[i])), NAMES[i]


# sha-256 (tests/test_int8_plan_gpu.py's scale_list_digest) of the sorted (site, scale) list of `built`'s model, taken from
# a build of the commit before int8_plan.py on an MI355X (two runs, one value): the calibrate-or-cache path of
# quantization.build_int8_yolox keeps its statistics and its scales
PARENT_SCALE_LIST_DIGEST = "20453094692e5ee341ac57e83579acba2a0c0a27b9eebe3966ce7a2c492a6e51"


def test_the_calibrated_scales_keep_the_parent_commits_values(built):
    from test_int8_plan_gpu import scale_list_digest
    from bevformer_tensorrt_amd.yolox_int8 import group_site
    got = scale_list_digest({group_site(g): s for g, s in enumerate(built["model"].group_scales)})
    print("scale list:", got)
    assert got == PARENT_SCALE_LIST_DIGEST
