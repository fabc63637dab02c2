"""The INT8 build of a use_depthwise YOLOX (quantization.build_int8_yolox(depthwise="int8"), yolox_int8.py) on the GPU:
YOLOX(YOLOX_NANO) at [2, 3, 96, 128], min-max calibration on two random frames.

* every dwsep_conv_q_taps call of one forward against its own float64 statement from the int8 operands it received:
  stage 1 inside test_dwsep_conv_s8_gpu.stage1_interval, stage 2 inside util_conv_slice_s8.silu_interval.  t is never
  visible, so a pixel with channels of t within delta of a half-integer is checked against every combination of them;
* the model gate of tests/test_yolox_int8_gpu.py: rms error against the fp32 plain path <= 1.25 x the fake-quant statement's;
* equal bits eagerly and from YOLOXRunner; no library call on the int8 path; the fp16 model's bits; a dense model builds
  the same with the keyword; weight reload, capture guard, calibration cache."""
import copy
import itertools
import types

import numpy as np
import pytest
import torch

import util_conv_slice_s8 as S
from test_dwsep_conv_s8_gpu import dw_sums, stage1_interval, stage2_sums
from test_yolox_int8_gpu import BAR, NAMES, _Counter, _bits, _nhwc

pytestmark = pytest.mark.gpu
CASE = (2, 3, 96, 128)


def _build(fp, frames, **kw):
    from bevformer_tensorrt_amd import quantization as Q
    return Q.build_int8_yolox(fp, torch.device("cuda"), frames, calibrator="minmax", depthwise="int8", **kw)


@pytest.fixture(scope="module")
def built():
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    base = YOLOX(YOLOX_NANO, seed=0, ops=types.SimpleNamespace())
    ref32 = copy.deepcopy(base).cuda()
    fp = base.cuda().half()
    fp.ops = fn
    ref32.load_state_dict({k: v.float() for k, v in fp.state_dict().items()})
    g = torch.Generator().manual_seed(11)
    image = torch.randn(CASE, generator=g).cuda().half()
    before = tuple(o.clone() for o in fp(image))
    frames = [torch.randn(CASE, generator=g).cuda().half() for _ in range(2)]
    model, note = _build(fp, frames)
    calls = []

    def probe(*a, **kw):
        res_before = None if a[11] is None else a[11].clone()
        calls.append((a, res_before, fn.dwsep_conv_q_taps(*a, **kw)))
        return calls[-1][2]

    model.ops = types.SimpleNamespace(**{k: getattr(fn, k) for k in fn.__all__})
    model.ops.dwsep_conv_q_taps = probe
    got = tuple(o.clone() for o in model(image))
    model.ops = fn
    return dict(fp=fp, model=model, note=note, image=image, before=before, ref=ref32(image.float()), got=got, calls=calls,
                frames=frames)


def test_note_and_sites(built):
    m = built["model"]
    assert built["note"] == {"int8_layers": 77, "scale_groups": 57, "calibration_frames": 2, "depthwise_layers": 30}
    assert len(m.dw_scales) == 30 and len(m.scales) == 87 and all(0 < v < 1e3 for v in m.scales.values())


def test_every_depthwise_call_against_its_own_statement(built):
    assert len(built["calls"]) == 30
    shares = []
    for i, (a, res_before, out) in enumerate(built["calls"]):
        x, sx, wd, sd, bd, st, wp, sp, bp, a1, a2, _, sr, stride, _, so, dt = a
        assert (a1, a2, dt) == ("silu", "silu", torch.int8)
        x, got = _nhwc(x), _nhwc(out)
        wd, sd, bd, wp, sp, bp = (t.cpu().numpy() for t in (wd, sd, bd, wp, sp, bp))
        res = None if res_before is None else _nhwc(res_before)
        lo1, hi1 = stage1_interval(dw_sums(x, wd, stride), sx, sd, bd, st)
        interval = lambda t, r: S.silu_interval(stage2_sums(t, wp), st, 1.0, sp, bp, r, sr, so)[2:]      # noqa: E731
        lo, hi = interval(lo1, res)
        open_px = np.argwhere((lo1 != hi1).any(-1))
        for px in map(tuple, open_px):                    # every combination of the undecided channels of t at this pixel
            ch = np.flatnonzero(lo1[px] != hi1[px])
            assert len(ch) <= 10
            ends = []
            for pick in itertools.product((0, 1), repeat=len(ch)):
                t = lo1[px].copy()
                t[ch] = np.where(pick, hi1[px][ch], lo1[px][ch])
                ends.append(interval(t[None], None if res is None else res[px][None]))
            lo[px], hi[px] = np.min([e[0][0] for e in ends], 0), np.max([e[1][0] for e in ends], 0)
        assert not ((got < lo) | (got > hi)).any(), f"call {i}"
        decided = np.ones(got.shape[:3], bool)
        decided[tuple(open_px.T)] = False
        shares.append((S.check_interval(got[decided], lo[decided], hi[decided]), 1 - decided.mean()))
    print(f"per layer: outputs within delta of a half-integer max {max(s for s, _ in shares):.4%}; pixels with an "
          f"undecided channel of t max {max(p for _, p in shares):.3%}")


def test_int8_path_is_as_close_to_fp32_as_its_fake_quant_statement(built):
    emu = built["model"].fake_quant_reference(built["image"])
    for name, g, e, r in zip(NAMES, built["got"], emu, built["ref"]):
        rms = lambda t: float((t.double() - r.double()).pow(2).mean().sqrt())    # noqa: E731
        mx, bar = float((g.float() - r).abs().max()), BAR * max(1.0, float(r.abs().max()))
        print(f"{name}: |ref|max {float(r.abs().max()):.3f}; rms error int8 {rms(g):.4e}, fake-quant {rms(e):.4e} (ratio "
              f"{rms(g) / rms(e):.3f}); max error int8 {mx:.4e}, bar {bar:.3e} (int8 at {mx / bar:.2f} of it)")
        assert g.dtype == torch.float16 and float(r.max() - r.min()) > 1e-3 and rms(e) > 0
        assert rms(g) <= 1.25 * rms(e), name


def test_runs_replay_probes_and_the_fp16_bits(built, monkeypatch):
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    model, img = built["model"], built["image"]
    runner = YOLOXRunner(model, CASE[0], *CASE[2:])
    for _ in range(2):
        runner.step(img)
    torch.cuda.synchronize()
    for name, x, y, z in zip(NAMES, built["got"], model(img), runner.head_outputs):
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z)), name
    counter = _Counter(monkeypatch)                       # no library convolution, torch.cat or dtype conversion
    model(img)
    torch.cuda.synchronize()
    assert counter.counts == {n: 0 for n, _ in _Counter.NAMES}
    for name, x, y in zip(NAMES, built["before"], built["fp"](img)):
        assert torch.equal(_bits(x), _bits(y)), name


def test_a_dense_model_builds_the_same_with_the_keyword():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    fp = YOLOX(YOLOX_S, seed=2).cuda().half()
    img = torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(4)).cuda().half()
    a, na = Q.build_int8_yolox(fp, torch.device("cuda"), [img], calibrator="minmax")
    b, nb = _build(fp, [img])
    assert na == nb and a.scales == b.scales and b.dw_scales == []
    for x, y in zip(a(img), b(img)):
        assert torch.equal(_bits(x), _bits(y))


def test_weight_reload_capture_guard_and_calibration_cache(built, tmp_path):
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_NANO
    fp = YOLOX(YOLOX_NANO, seed=3).cuda().half()
    img, path = built["image"], str(tmp_path / "nano.npz")
    model, note = _build(fp, built["frames"][:1], calibration_cache=path)
    again, note2 = _build(fp, [], calibration_cache=path)           # the cache rebuilds the model without a frame
    assert (note["calibration_frames"], note2["calibration_frames"]) == (1, 0) and again.scales == model.scales
    assert model.operands(build=False) is None
    scratch = torch.zeros(8, device="cuda")
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)
        with pytest.raises(RuntimeError):
            model.prepare()
    eager = [o.clone() for o in model(img)]
    ops0 = model.operands(build=False)
    dw = fp.bbox_head.reg_convs[1][1]                     # a new depthwise weight: the int8 operands are stale and rebuilt
    with torch.no_grad():
        dw.depthwise_conv.weight.mul_(-1.0)
    assert ops0 is not None and model.operands(build=False) is None
    new = model(img)
    assert model.operands(build=False) is not ops0 and torch.equal(model.operands()[dw][0], -ops0[dw][0])
    assert not torch.equal(_bits(new[4]), _bits(eager[4])) and torch.equal(_bits(new[0]), _bits(eager[0]))
