"""quantization.build_int8_centernet on the GPU: the synthetic CenterNet(seed=0), min-max calibration on four random
frames (two of each shape), both neck modes, at (1, 3, 128, 128) -- the neck's DCN packs see 4 x 4, 8 x 8 and 16 x 16
maps, fewer pixels than one tile of the int8 DCN block for the first two -- and (2, 3, 160, 224).

* every convolution and deconvolution call of one forward replayed against its own float64 statement from the int8
  inputs the kernel actually received (exact outside the derived near-tie interval of tests/util_centernet_int8.py); the
  DCN calls against exact=True on the same operands within the bars of tests/test_int8_chain_gpu.py; every tensor read
  with the scale it was written with;
* the backbone gate: rms error against the fp32 plain path at most 1.25 x that of `fake_quant_reference` (the project's
  YOLOX gate with the same argument: the kernels and the statement quantise the same tensors with the same scales, only
  tie flips differ);
* the head-output gate: the same ratio for the three head outputs, MEASURED on the GPU (the int8 DCN's 8-bit area weights
  are not in the fake-quant statement, so it cannot be derived in advance) and gated at the measured ratio plus the same
  quarter.  Measured (rms error of the int8 kernels over that of the fake-quant statement, both against fp32; heat map,
  wh, offset): neck="int8" 1.111 / 1.143 / 1.115 at (1, 3, 128, 128) and 1.083 / 1.080 / 1.070 at (2, 3, 160, 224);
  neck="fp16" 1.053 / 1.036 / 1.080 and 1.024 / 1.020 / 1.016 -- none above 2, so no site needs an attribution.  The
  position against the fp16 model's 3e-2 bar is printed, not gated (min-max scales on a synthetic model with random
  weights: the int8 heat map is up to 0.8 from fp32, the statement's own error);
* eager / eager / CenterNetRunner replay bit equality with the decode, the capture guard, the weight reload, no library
  convolution / pooling / dtype conversion on the neck="int8" path, the calibration cache, and the fp16 CenterNet
  beside the build giving the bits it gave before."""
import pytest
import torch

import test_centernet_gpu as TC
import util_centernet_int8 as U
import util_conv_slice_s8 as S
import util_deconv_s8 as D

pytestmark = pytest.mark.gpu

SHAPES = ((1, 3, 128, 128), (2, 3, 160, 224))
NECKS = ("int8", "fp16")
NAMES = TC.NAMES
# rms(int8 kernels - fp32 plain) / rms(fake-quant statement - fp32 plain) per head output, measured on MI355X (the larger
# of the two shapes' ratios, rounded up to two decimals); the gate is this plus a quarter
HEAD_RATIOS = {"int8": (1.12, 1.15, 1.12), "fp16": (1.06, 1.04, 1.08)}


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    import types
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd import centernet as C
    from bevformer_tensorrt_amd.quantization import build_int8_centernet
    fp = C.CenterNet(seed=0).cuda().half()
    plain_ops = types.SimpleNamespace(modulated_deformable_conv2d=fn.modulated_deformable_conv2d)
    ref32 = C.CenterNet(seed=1, ops=plain_ops).cuda()
    ref32.load_state_dict({k: v.float() for k, v in fp.state_dict().items()})      # the fp16 weights, exactly
    g = torch.Generator().manual_seed(21)
    images = {s: torch.randn(s, generator=g).cuda().half() for s in SHAPES}
    before = {s: [o.clone() for o in fp(images[s])] for s in SHAPES}
    frames = [torch.randn(SHAPES[i % 2], generator=g).cuda().half() for i in range(4)]
    cache = str(tmp_path_factory.mktemp("calib") / "centernet.calib")
    models, notes = {}, {}
    models["int8"], notes["int8"] = build_int8_centernet(fp, "cuda", frames, "minmax", calibration_cache=cache, neck="int8")
    models["fp16"], notes["fp16"] = build_int8_centernet(fp, "cuda", [], "minmax", calibration_cache=cache, neck="fp16")
    ref = {s: tuple(o.clone() for o in ref32(images[s].float())) for s in SHAPES}
    with torch.no_grad():
        ref_bb = {s: ref32.backbone(images[s].float())[0].clone() for s in SHAPES}
    return dict(fp=fp, ref32=ref32, images=images, before=before, frames=frames, cache=cache, models=models, notes=notes,
                ref=ref, ref_bb=ref_bb)


def test_notes_and_cache(built):
    """Layer and site counts as tests/test_centernet_int8_cpu.py derives them; the second build loaded the first one's
    calibration cache (no frame run) and reads the same scales."""
    n8, n16 = built["notes"]["int8"], built["notes"]["fp16"]
    assert n8 == dict(int8_layers=30, scale_sites=33, calibration_frames=4, neck="int8")
    assert n16 == dict(int8_layers=21, scale_sites=21, calibration_frames=0, neck="fp16")
    m8, m16 = built["models"]["int8"], built["models"]["fp16"]
    assert all(m8.scales[s] == v for s, v in m16.scales.items())
    assert m8.cfg is built["fp"].cfg and m8.fp is built["fp"]


def test_fp16_model_keeps_its_bits(built):
    fp = built["fp"]
    assert not any(hasattr(d, "chain_cal") for d in fp.neck.dcn)
    for s in SHAPES:
        for name, a, b in zip(NAMES, built["before"][s], fp(built["images"][s])):
            assert torch.equal(_bits(a), _bits(b)), name


def test_fake_quant_reference_without_quantisation_is_the_fp32_plain_path(built):
    """The same layer list on the un-quantised weights: equal to CenterNet's plain path in fp32 up to the summation order
    of fp32 convolutions (the merged head sums 192 channels where the branches sum 64 each; the library picks its own
    algorithm per shape): 1e-4 of the output's range, three orders below the quantisation error."""
    s = SHAPES[1]
    for neck in NECKS:
        got = built["models"][neck].fake_quant_reference(built["images"][s].float(), quantize=False)
        for name, a, r in zip(NAMES, got, built["ref"][s]):
            err = float((a - r).abs().max())
            print(f"{neck} {name}: max |diff| {err:.3e} of |ref|max {float(r.abs().max()):.3f}")
            assert a.dtype == torch.float32 and err <= 1e-4 * max(1.0, float(r.abs().max())), name


def _nhwc_np(t):
    return t.permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _replay(name, args, kwargs, out):
    """One recorded call against its float64 statement.  -> (share excused, share differing from the rounding)."""
    got = _nhwc_np(out)
    if name == "conv_slice_q_taps":
        x, sx, w, ws, b, act, res, sres, stride, _, sout, odt = args
        acc = S.sums(_nhwc_np(x), w.cpu().numpy(), w.shape[1], stride)
        t = U.epilogue_interval(acc, sx, ws.cpu().numpy(), b.cpu().numpy(), None if res is None else _nhwc_np(res), sres,
                                act == "relu", sout if odt == torch.int8 else None)
        assert kwargs["res_first"] == (res is not None)
    elif name == "conv_int8_chain_nhwc":
        x, sx, w, ws, b, relu, stride, odt, sout = args
        acc = S.sums(_nhwc_np(x), w.cpu().numpy(), w.shape[1], stride)
        t = U.epilogue_interval(acc, sx, ws.cpu().numpy(), b.cpu().numpy(), None, 1.0, relu, None, unfused=True)
    else:
        x, sx, w, ws, b, relu, sout, odt = args
        acc = D.sums(_nhwc_np(x), w.cpu().numpy())
        t = U.epilogue_interval(acc, sx, ws.cpu().numpy(), b.cpu().numpy(), None, 1.0, relu, sout)
    return U.check_output(got, *t)


@pytest.mark.parametrize("neck", NECKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_every_call_of_a_forward_against_its_own_statement(built, shape, neck):
    import bevformer_tensorrt_amd.functions as fn
    model, img = built["models"][neck], built["images"][shape]
    rec = U.ScaleRecorder(fn, keep_calls=True)
    packed = model.run(img.contiguous(), model.operands(), rec)          # (every read's scale is asserted as it happens)
    torch.cuda.synchronize()
    rec.check()
    assert len(rec.written) == (27 if neck == "int8" else 21) and packed.shape[1] == 88
    counts = {}
    for name, args, kwargs, out in rec.calls:
        counts[name] = counts.get(name, 0) + 1
        if name == "modulated_deformable_conv2d_int8_nhwc":
            exact = fn.modulated_deformable_conv2d_int8_nhwc(*args[:-1], True)
            df = (out.float() - exact.float()).abs()
            print(f"DCN {tuple(out.shape)}: fast against exact mean {float(df.mean()):.3f} max {float(df.max()):.0f} steps")
            assert float(df.mean()) <= 0.6 and float(df.max()) <= 8 and bool(out.any())
        else:
            share, off = _replay(name, args, kwargs, out)
            print(f"{name} {tuple(out.shape)}: {share:.4%} within delta of a boundary, {off:.4%} differ from the rounding")
    want = dict(conv_slice_q_taps=21)
    if neck == "int8":
        want.update(conv_int8_chain_nhwc=3, modulated_deformable_conv2d_int8_nhwc=3, conv_transpose2d_q_nhwc=3)
    assert counts == want


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backbone_gate(built, shape):
    """At the backbone's output: rms error of the int8 kernels against the fp32 plain path <= 1.25 x that of the
    fake-quant statement (same tensors, same scales, same weight quantisation: only tie flips differ)."""
    import bevformer_tensorrt_amd.functions as fn
    model, img = built["models"]["int8"], built["images"][shape]
    live, fq = {}, {}
    model.run(img.contiguous(), model.operands(), fn, tensors=live)
    model.fake_quant_reference(img.float(), tensors=fq)
    ref = built["ref_bb"][shape]
    got = live["s3.b1.out"].float() * model.scale("s3.b1.out")
    e_k, e_f = _rms(got, ref), _rms(fq["s3.b1.out"], ref)
    print(f"{shape} backbone output: rms error kernels {e_k:.4e}, fake-quant statement {e_f:.4e}, ratio {e_k / e_f:.3f}; "
          f"|ref| rms {float(ref.pow(2).mean().sqrt()):.3f}")
    assert e_f > 0 and e_k <= 1.25 * e_f


@pytest.mark.parametrize("neck", NECKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_output_gate(built, shape, neck):
    model, img = built["models"][neck], built["images"][shape]
    got = model(img)
    fq = model.fake_quant_reference(img.float())
    rows = []
    for name, g, f, r in zip(NAMES, got, fq, built["ref"][shape]):
        e_k, e_f = _rms(g.float(), r), _rms(f, r)
        scale = max(1.0, float(r.abs().max()))
        print(f"{shape} neck={neck} {name}: rms error kernels {e_k:.4e}, fake-quant {e_f:.4e}, ratio {e_k / e_f:.3f}; "
              f"max error {float((g.float() - r).abs().max()):.3e} (the fp16 model's bar {3e-2 * scale:.3e})")
        rows.append((name, e_k, e_f))
    for (name, e_k, e_f), measured in zip(rows, HEAD_RATIOS[neck]):
        assert measured is not None, "HEAD_RATIOS holds no measurement"
        assert e_f > 0 and e_k <= (measured + 0.25) * e_f, name
    assert float(got[0].min()) >= 0.0 and float(got[0].max()) <= 1.0


@pytest.mark.parametrize("neck", NECKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_two_runs_and_the_replay_give_equal_bits(built, shape, neck):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    from bevformer_tensorrt_amd.functions.decode2d import centernet_decode
    model, img = built["models"][neck], built["images"][shape]
    a = [o.clone() for o in model(img)]
    b = model(img)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
        assert x.shape == (shape[0], dict(zip(NAMES, (80, 2, 2)))[name], shape[2] // 4, shape[3] // 4) and x.dtype == torch.float16
    cfg = model.cfg["test_cfg"]
    dec = centernet_decode(*b, cfg["topk"], shape[2:], cfg["local_maximum_kernel"], padded=True)
    runner = CenterNetRunner(model, *shape[:1], *shape[2:])
    for _ in range(2):
        out = runner.step(img)
    torch.cuda.synchronize()
    for name, x, y in zip(NAMES, a, runner.head_outputs):
        assert torch.equal(_bits(x), _bits(y)), name
    for name, x, y in zip(("boxes", "scores", "labels", "count"), dec, out):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert int(out[3].min()) == cfg["topk"]


class _Conversions:
    """Probes in the style of tests/test_centernet_gpu.py's _Counter: calls of Tensor.to / half / float / char / type whose
    result has another dtype than their input."""

    def __init__(self, monkeypatch):
        self.count = 0
        for name in ("to", "half", "float", "char", "type"):
            monkeypatch.setattr(torch.Tensor, name, self._wrap(getattr(torch.Tensor, name)))

    def _wrap(self, inner):
        def probe(t, *args, **kwargs):
            out = inner(t, *args, **kwargs)
            self.count += int(isinstance(out, torch.Tensor) and out.dtype != t.dtype)
            return out
        return probe


def test_no_library_convolution_and_no_conversion_on_the_int8_path(built, monkeypatch):
    from bevformer_tensorrt_amd.functions import conv as C
    model, img = built["models"]["int8"], built["images"][SHAPES[1]]
    model(img)
    misses = list(C.CONV_MISSES)
    counter, conv = TC._Counter(monkeypatch), _Conversions(monkeypatch)
    model(img)
    torch.cuda.synchronize()
    print("int8:", counter.counts, "conversions:", conv.count)
    assert counter.counts == dict(conv2d=0, conv_transpose2d=0, max_pool2d=0, interpolate=0) and conv.count == 0
    assert C.CONV_MISSES == misses
    model.fake_quant_reference(img.float())                  # the probes see the torch statement
    assert counter.counts["conv2d"] == 1 + 19 + 3 + 2 and counter.counts["conv_transpose2d"] == 3
    assert counter.counts["max_pool2d"] == 1


def test_capture_guard_and_weight_reload(built):
    from bevformer_tensorrt_amd import centernet as C
    from bevformer_tensorrt_amd import centernet_int8 as CI
    fp = C.CenterNet(seed=3).cuda().half()
    src = built["models"]["int8"]
    model = CI.Int8CenterNet(fp, src.scales, neck="int8")
    img = built["images"][SHAPES[0]]
    scratch = torch.zeros(8, device="cuda")
    assert model.operands(build=False) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)                                            # (the capture holds one node of its own)
        with pytest.raises(RuntimeError, match="prepare"):
            model(img)                                               # raises before it launches anything
        with pytest.raises(RuntimeError):
            model.prepare()
    del graph
    assert model.operands(build=False) is None
    first = [o.clone() for o in model(img)]
    t0 = model.operands(build=False)
    assert t0 is not None and model.operands() is t0
    # new weights: the wh branch's final convolution becomes the constant 0.5; the operands are rebuilt
    with torch.no_grad():
        fp.heads["wh"][1].weight.zero_()
        fp.heads["wh"][1].bias.fill_(0.5)
    assert model.operands(build=False) is None                       # stale
    new = model(img)
    assert model.operands(build=False) is not t0
    assert bool((new[1] == 0.5).all())
    for i in (0, 2):
        assert torch.equal(_bits(new[i]), _bits(first[i])), NAMES[i]
    with pytest.raises(ValueError):
        model(img.float())
    with pytest.raises(ValueError):
        model(img[:, :, :100])


# sha-256 (tests/test_int8_plan_gpu.py's scale_list_digest) of the sorted (site, scale) list of `built`'s two models (the second one built from the first one's cache), taken from
# a build of the commit before int8_plan.py on an MI355X (two runs, one value): the calibrate-or-cache path of
# quantization.build_int8_centernet keeps its statistics and its scales
PARENT_SCALE_LIST_DIGEST = "4b88b482d69189bbf147ecd221531e065436d63188ad40d87b8bdb8aa4b1f53b"


def test_the_calibrated_scales_keep_the_parent_commits_values(built):
    from test_int8_plan_gpu import scale_list_digest
    got = scale_list_digest(built["models"]["int8"].scales, built["models"]["fp16"].scales)
    print("scale list:", got)
    assert got == PARENT_SCALE_LIST_DIGEST
