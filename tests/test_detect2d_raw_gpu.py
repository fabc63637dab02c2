"""YOLOXRunner / CenterNetRunner(raw_size=...): `step_raw` from raw uint8 camera frames (design/letterbox.md) on the
smallest models -- YOLOX_S from 90 x 120 frames (keep-ratio to 120 x 160, a 160 x 160 input) and CenterNet from 96 x 128
frames (a centred paste at (16, 16) into 160 x 160).  `step_raw` == `step` on image_letterbox's output followed by the
host-side border / rescale of *_get_bboxes; eager == replay; the replay follows `raw_buffer` without a re-capture; a
mismatching size raises; a runner with raw_size keeps `step`'s bits; one INT8 model runs `step_raw`."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

YOLOX_RAW, YOLOX_SCALE, YOLOX_NET = (90, 120), (160, 160), (160, 160)
CENTERNET_RAW, CENTERNET_SCALE, CENTERNET_NET = (96, 128), (128, 128), (160, 160)
NAMES = ("boxes", "scores", "labels", "count")


def _bits(t):
    return t.contiguous().view(torch.int32)


def frames(seed, n, size, batch=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (batch,) + size + (3,), generator=g, dtype=torch.uint8).cuda() for _ in range(n)]


@pytest.fixture(scope="module")
def yolox():
    """YOLOX_S with the synthetic weights, its stem divided by 64: the synthetic initialisation is balanced for a
    unit-normal image, the config's pipeline (mean 0, std 1) feeds raw 0 .. 255 values."""
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    model = YOLOX(YOLOX_S, seed=0, ops=types.SimpleNamespace())
    model.backbone.stem.conv.weight.data.mul_(1.0 / 64)
    model = model.cuda().half()
    model.ops = fn
    return model


@pytest.fixture(scope="module")
def centernet():
    from bevformer_tensorrt_amd.centernet import CenterNet
    return CenterNet(seed=0).cuda().half()


def host_rescale(boxes, geometry):
    """What *_get_bboxes do on the host to boxes in the network input's pixels: minus the border's (left, top), divided
    by the scale factors -> (want, tol).  The device does the same fp32 subtraction and division, so the two differ by
    at most the rounding of one subtraction and one division: 2 * 2^-24 relative to (|x| + border) / scale."""
    b = geometry.get("border")
    shift = torch.tensor([float(b[2]), float(b[0])] * 2 if b is not None else [0.0] * 4)
    scale = torch.tensor(geometry["scale_factor"].tolist(), dtype=torch.float32)
    boxes = boxes.float().cpu()
    return (boxes - shift) / scale, 2.0 ** -23 * (boxes.abs() + shift) / scale


def check_against_step(raw_runner, plain_runner, raw, pipeline):
    import bevformer_tensorrt_amd as bev
    got = raw_runner.step_raw(raw)
    image = bev.image_letterbox(raw, raw_runner.geometry, pipeline)
    assert torch.equal(raw_runner.image_buffer, image)                 # the first launch IS the letterbox
    ref = plain_runner.step(image)
    torch.cuda.synchronize()
    n_got, n_ref = got[3].cpu(), ref[3].cpu()
    assert torch.equal(n_got, n_ref) and int(n_got.max()) > 0
    for b, n in enumerate(n_got.tolist()):
        assert torch.equal(got[2][b, :n], ref[2][b, :n])
        assert torch.equal(_bits(got[1][b, :n]), _bits(ref[1][b, :n]))
        want, tol = host_rescale(ref[0][b, :n], raw_runner.geometry)
        diff = (got[0][b, :n].cpu() - want).abs()
        print(f"{pipeline} image {b}: {n} boxes, largest difference {float(diff.max()):.3e} "
              f"(largest allowed {float(tol.max()):.3e})")
        assert bool((diff <= tol).all())
    return got


def test_yolox_step_raw_equals_step_on_the_letterboxed_image(yolox):
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    raw = frames(1, 1, YOLOX_RAW, batch=2)[0]
    a = YOLOXRunner(yolox, 2, *YOLOX_NET, raw_size=YOLOX_RAW, img_scale=YOLOX_SCALE)
    b = YOLOXRunner(yolox, 2, *YOLOX_NET)
    g = a.geometry
    assert g["size"] == (120, 160) and g["offset"] == (0, 0) and g["pad_shape"] == (160, 160, 3)
    assert a.raw_buffer.shape == (2, 90, 120, 3) and a.raw_buffer.dtype == torch.uint8 and b.raw_buffer is None
    check_against_step(a, b, raw, "yolox")
    assert bool((a.image_buffer[:, :, 120:] == 114).all())                                        # the 114 padding
    with pytest.raises(RuntimeError):
        b.step_raw(raw)
    with pytest.raises(ValueError):
        a.step_raw(raw[:, :80])
    with pytest.raises(ValueError):
        a.step_raw(raw.float())


def test_centernet_step_raw_equals_step_on_the_letterboxed_image(centernet):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    raw = frames(2, 1, CENTERNET_RAW, batch=2)[0]
    a = CenterNetRunner(centernet, 2, *CENTERNET_NET, raw_size=CENTERNET_RAW, img_scale=CENTERNET_SCALE)
    b = CenterNetRunner(centernet, 2, *CENTERNET_NET)
    g = a.geometry
    assert g["size"] == (96, 128) and g["offset"] == (16, 16) and g["border"].tolist() == [16, 112, 16, 144]
    check_against_step(a, b, raw, "centernet")
    with pytest.raises(RuntimeError):
        b.step_raw(raw)
    with pytest.raises(ValueError):
        a.step_raw(raw[:, :, :100])


@pytest.mark.parametrize("which", ["yolox", "centernet"])
def test_eager_equals_replay_and_the_replay_follows_raw_buffer(which, yolox, centernet):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    if which == "yolox":
        make = lambda graph: YOLOXRunner(yolox, 1, *YOLOX_NET, graph=graph, raw_size=YOLOX_RAW, img_scale=YOLOX_SCALE)
        raws = frames(3, 3, YOLOX_RAW)
    else:
        make = lambda graph: CenterNetRunner(centernet, 1, *CENTERNET_NET, graph=graph, raw_size=CENTERNET_RAW,
                                             img_scale=CENTERNET_SCALE)
        raws = frames(4, 3, CENTERNET_RAW)
    run, eager = make(True), make(False)
    outs = [run.step_raw(r) for r in raws[:2]]
    graph = run._graph_raw
    assert graph is not None and run._graph is None
    assert not torch.equal(outs[0][0], outs[1][0])
    for r, o in zip(raws[:2], outs):
        for name, x, y in zip(NAMES, eager.step_raw(r), o):
            assert torch.equal(_bits(x), _bits(y)), name
    run.raw_buffer.copy_(raws[2])                                         # decode into the buffer, pass the buffer: no copy
    ptr = run.raw_buffer.data_ptr()
    got = run.step_raw(run.raw_buffer)
    assert run._graph_raw is graph and run.raw_buffer.data_ptr() == ptr and torch.equal(run.raw_buffer, raws[2])
    for name, x, y in zip(NAMES, eager.step_raw(raws[2]), got):
        assert torch.equal(_bits(x), _bits(y)), name
    assert len(run.head_outputs) == (9 if which == "yolox" else 3)


@pytest.mark.parametrize("which", ["yolox", "centernet"])
def test_a_mismatching_size_raises(which, yolox, centernet):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    if which == "yolox":
        make = lambda h, w, raw: YOLOXRunner(yolox, 1, h, w, raw_size=raw, img_scale=YOLOX_SCALE)
        good, raw = YOLOX_NET, YOLOX_RAW
    else:
        make = lambda h, w, raw: CenterNetRunner(centernet, 1, h, w, raw_size=raw, img_scale=CENTERNET_SCALE)
        good, raw = CENTERNET_NET, CENTERNET_RAW
    make(*good, raw)
    for h, w in ((good[0] + 32, good[1]), (good[0], good[1] - 32), (good[0] - 32, good[1] - 32)):
        with pytest.raises(ValueError):
            make(h, w, raw)


@pytest.mark.parametrize("which", ["yolox", "centernet"])
def test_step_keeps_its_bits_with_and_without_raw_size(which, yolox, centernet):
    from bevformer_tensorrt_amd.centernet import CenterNetRunner
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    g = torch.Generator().manual_seed(5)
    image = torch.randn((1, 3, 160, 160), generator=g).cuda().half()
    if which == "yolox":
        image = image * 64
        with_raw = YOLOXRunner(yolox, 1, *YOLOX_NET, raw_size=YOLOX_RAW, img_scale=YOLOX_SCALE)
        without = YOLOXRunner(yolox, 1, *YOLOX_NET)
    else:
        with_raw = CenterNetRunner(centernet, 1, *CENTERNET_NET, raw_size=CENTERNET_RAW, img_scale=CENTERNET_SCALE)
        without = CenterNetRunner(centernet, 1, *CENTERNET_NET)
    with_raw.step_raw(frames(6, 1, YOLOX_RAW if which == "yolox" else CENTERNET_RAW)[0])     # both graphs live side by side
    a, b = with_raw.step(image), without.step(image)
    assert int(a[3].max()) > 0
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(_bits(x), _bits(y)), name
    for x, y in zip(with_raw.head_outputs, without.head_outputs):
        assert torch.equal(x, y)


def test_int8_yolox_runs_step_raw(yolox):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.yolox import YOLOXRunner
    geo = bev.yolox_test_geometry(*YOLOX_RAW, img_scale=YOLOX_SCALE)
    raws = frames(7, 2, YOLOX_RAW)
    calib = [bev.image_letterbox(r, geo, "yolox") for r in raws]
    model, note = Q.build_int8_yolox(yolox, torch.device("cuda"), calib, calibrator="minmax")
    assert note["calibration_frames"] == 2 and note["int8_layers"] > 0
    run = YOLOXRunner(model, 1, *YOLOX_NET, raw_size=YOLOX_RAW, img_scale=YOLOX_SCALE)
    eager = YOLOXRunner(model, 1, *YOLOX_NET, graph=False, raw_size=YOLOX_RAW, img_scale=YOLOX_SCALE)
    for r in raws:
        got, want = run.step_raw(r), eager.step_raw(r)
        n = int(got[3][0])
        assert n > 0 and bool(torch.isfinite(got[0][0, :n]).all()) and bool(torch.isfinite(got[1][0, :n]).all())
        for name, x, y in zip(NAMES, want, got):
            assert torch.equal(_bits(x), _bits(y)), name
    assert run._graph_raw is not None
