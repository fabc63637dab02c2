"""bevops_image_letterbox (the 2-D detectors' camera front end: keep-ratio resize, paste into a constant canvas, normalise
in one launch) on the GPU against the numpy restatement (tests/util_letterbox.py), bit for bit: both arithmetics, fp32 and
fp16 output (== the RNE cast of the fp32 restatement), planes and channels-last, YOLOX's and CenterNet's constants, with
every buffer inside the guarded arena of tests/util_arena.py under both poisons (a store outside `output` disturbs a
guard, an unwritten pad element keeps the poison); sizes around the 64 x 8 tile; offsets, a paste that ends at the canvas
edge, tiles of padding alone; scale 1 == image_normalize_pad; the raw C entry and graph capture."""
import ctypes

import numpy as np
import pytest
import torch

import util_letterbox as U
from util_arena import Arena, POISONS

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 8          # csrc/image_letterbox.hip: kTW, kTH
MiB = 1 << 20

# name: (H0, W0), (Hs, Ws), canvas (Hp, Wp), offset (oy, ox) -- where this kernel can go wrong
CASES = {
    "one_pixel": ((1, 1), (1, 1), (32, 32), (0, 0)),
    "up_every_clamp": ((2, 3), (5, 7), (32, 32), (11, 16)),                 # 2.5 x up
    "odd_rows": ((45, 70), (36, 56), (64, 64), (0, 0)),                     # 3 * W0 % 4 != 0
    "up_two_tiles": ((37, 53), (64, 92), (96, 160), (7, 63)),               # the paste straddles three tile columns
    "area": ((64, 64), (32, 32), (32, 32), (0, 0)),                         # ends exactly at the canvas edge
    "area_offset": ((64, 64), (32, 32), (43, 96), (11, 64)),                # the first tile column is padding alone
    "half_one_axis": ((64, 66), (32, 32), (64, 96), (11, 16)),              # NOT the area form
    "ratio_3_4": ((100, 141), (29, 41), (36, 104), (7, 63)),                # ends exactly at the canvas edge
    "integer_taps": ((108, 192), (36, 64), (40, 200), (0, 0)),              # two tile columns of padding alone
}
CONSTANTS = {"yolox": U.YOLOX, "centernet": U.CENTERNET}


def bits(t):
    """Bit pattern of a float32 / float16 tensor or array (so that -0.0 != +0.0 and NaN == NaN)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def geometry(src, size, canvas, offset):
    return dict(ori_shape=src + (3,), size=size, pad_shape=canvas + (3,), offset=offset)


def check_guarded(img, size, canvas, offset, arith, const, forms=((torch.float32, False), (torch.float32, True),
                                                                  (torch.float16, False), (torch.float16, True))):
    """Every asked output form of one input inside a guarded arena, under both poisons, against the restatement."""
    import bevformer_tensorrt_amd as bev
    pipe = dict(const, arith=arith)
    want = U.letterbox(img, size, canvas, offset, arith, const["mean"], const["std"], const["to_rgb"], const["pad"])
    want16 = torch.from_numpy(want).half()
    n = img.shape[0]
    geo = geometry(img.shape[1:3], size, canvas, offset)
    for poison in POISONS:
        arena = Arena(4 * MiB, poison)
        raw = arena.place(torch.from_numpy(img), 1, "images")             # an odd address: rows off dword alignment
        for dt, cl in forms:
            out = arena.empty((n, 3) + canvas, dt, 4 if dt == torch.float32 else 2, f"out:{dt}:{cl}", channels_last=cl)
            got = bev.image_letterbox(raw, geo, pipe, channels_last=cl, out=out)
            assert got.data_ptr() == out.data_ptr()
            ref = want if dt == torch.float32 else want16
            assert np.array_equal(bits(out), bits(ref)), (arith, dt, cl, hex(poison))
        arena.check()
        assert torch.equal(raw.cpu(), torch.from_numpy(img))
    return want


@pytest.mark.parametrize("const", list(CONSTANTS))
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_cases_bit_exact(case, arith, const):
    src, size, canvas, offset = CASES[case]
    check_guarded(U.noise(7, 3, *src), size, canvas, offset, arith, CONSTANTS[const])     # batch 3, different images


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("Hs", [TILE_H - 1, TILE_H, TILE_H + 1])
def test_tile_edges(Hs, arith):
    """Resized and padded sizes of 63, 64, 65 x 7, 8, 9, from a source 1.25 x as large with an odd row length, at the three
    offsets; every third paste ends exactly at the canvas edge."""
    k = 0
    for Ws in (TILE_W - 1, TILE_W, TILE_W + 1):
        H0, W0 = -(-Hs * 5 // 4), (-(-Ws * 5 // 4)) | 1
        img = U.noise(Hs * 1000 + Ws, 2, H0, W0)
        for oy, ox in ((0, 0), (11, 16), (7, 63)):
            extra = ((0, 0), (1, 1), (TILE_H, TILE_W))[k % 3]
            k += 1
            canvas = (oy + Hs + extra[0], ox + Ws + extra[1])
            check_guarded(img, (Hs, Ws), canvas, (oy, ox), arith, U.CENTERNET if arith else U.YOLOX,
                          forms=((torch.float32, False), (torch.float16, True)))


def test_identity_canvas_sizes_around_the_tile():
    """Scale 1 into canvases of exactly 63, 64, 65 x 7, 8, 9: the padded size itself at the tile edges."""
    for Hp in (TILE_H - 1, TILE_H, TILE_H + 1):
        for Wp in (TILE_W - 1, TILE_W, TILE_W + 1):
            img = U.noise(Hp * 100 + Wp, 1, Hp - 2, Wp - 3)
            check_guarded(img, (Hp - 2, Wp - 3), (Hp, Wp), (1, 2), 0, U.YOLOX, forms=((torch.float32, True),))


@pytest.mark.parametrize("arith", [0, 1])
def test_scale_one_equals_image_normalize_pad(arith):
    import bevformer_tensorrt_amd as bev
    dev = torch.from_numpy(U.noise(3, 2, 45, 71)).cuda()
    Hp, Wp = bev.padded_size(45, 71)
    geo = geometry((45, 71), (45, 71), (Hp, Wp), (0, 0))
    for const in (U.YOLOX, U.CENTERNET):
        pipe = dict(const, arith=arith, pad=(0.0, 0.0, 0.0))
        for cl in (False, True):
            for dt in (torch.float32, torch.float16):
                a = bev.image_letterbox(dev, geo, pipe, dtype=dt, channels_last=cl)
                b = bev.image_normalize_pad(dev, mean=const["mean"], std=const["std"], to_rgb=const["to_rgb"], dtype=dt,
                                            channels_last=cl)
                assert a.shape == b.shape and a.dtype == dt
                inside = (slice(None), slice(None), slice(0, 45), slice(0, 71))
                assert np.array_equal(bits(a[inside].contiguous()), bits(b[inside].contiguous()))
                if const is U.YOLOX:            # mean 0: the normalised pad value 0 is image_normalize_pad's +0.0 padding
                    assert np.array_equal(bits(a.contiguous()), bits(b.contiguous()))


@pytest.mark.parametrize("channels_last", [False, True])
def test_arith_1_shares_its_taps_with_image_normalize_resize_pad(channels_last):
    """The two entries share their taps and arithmetic leaves (csrc/image_resample.h).  With mean 0 and std 1 both
    normalisation orders are exact, so arith 1 pasted at (0, 0) into a zero canvas IS image_normalize_resize_pad:
    45 x 70 -> 36 x 56 in 64 x 64, bit for bit (and the two numpy restatements agree on it)."""
    import bevformer_tensorrt_amd as bev
    import util_image_scale as S
    zero, one = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    img = U.noise(11, 2, 45, 70)
    want = U.letterbox(img, (36, 56), (64, 64), (0, 0), 1, zero, one, False, zero)
    assert np.array_equal(bits(want), bits(S.normalize_resize_pad(img, (36, 56), zero, one, False, size_divisor=32)))
    dev = torch.from_numpy(img).cuda()
    a = bev.image_letterbox(dev, geometry((45, 70), (36, 56), (64, 64), (0, 0)),
                            dict(arith=1, mean=zero, std=one, to_rgb=False, pad=zero), dtype=torch.float32,
                            channels_last=channels_last)
    b = bev.image_normalize_resize_pad(dev, size=(36, 56), mean=zero, std=one, to_rgb=False, size_divisor=32,
                                       dtype=torch.float32, channels_last=channels_last)
    assert tuple(a.shape) == tuple(b.shape) == (2, 3, 64, 64)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(want))


@pytest.mark.parametrize("name", ["yolox", "centernet"])
def test_camera_frame_through_the_test_geometry(name):
    """2 x 900 x 1600 uint8 through each detector's own geometry and constants (ratio 2.5: 360 x 640 in 640^2 / at
    (12, 16) in 672^2), bit for bit."""
    import bevformer_tensorrt_amd as bev
    geo = (bev.yolox_test_geometry if name == "yolox" else bev.centernet_test_geometry)(900, 1600)
    assert geo["size"] == (360, 640) and geo["offset"] == ((0, 0) if name == "yolox" else (12, 16))
    img = U.noise(1, 2, 900, 1600)
    c = U.PIPELINES[name]
    want = U.letterbox(img, geo["size"], geo["pad_shape"][:2], geo["offset"], c["arith"], c["mean"], c["std"], c["to_rgb"],
                       c["pad"])
    dev = torch.from_numpy(img).cuda()
    got = bev.image_letterbox(dev, geo, name, dtype=torch.float32)
    assert np.array_equal(bits(got), bits(want))
    half = bev.image_letterbox(dev, geo, name, channels_last=True)
    assert half.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bits(half), bits(torch.from_numpy(want).half()))


def test_operator_argument_checks():
    import bevformer_tensorrt_amd as bev
    dev = torch.from_numpy(U.noise(5, 2, 45, 70)).cuda()
    geo = bev.yolox_test_geometry(45, 70, img_scale=(64, 64))
    assert geo["size"] == (41, 64) and geo["pad_shape"] == (64, 64, 3)
    out = bev.image_letterbox(dev, geo, "yolox")
    assert out.dtype == torch.float16 and tuple(out.shape) == (2, 3, 64, 64)
    want = U.letterbox(dev.cpu().numpy(), (41, 64), (64, 64), (0, 0), **{k: U.YOLOX[k] for k in ("arith", "mean", "std", "to_rgb", "pad")})
    assert np.array_equal(bits(out), bits(torch.from_numpy(want).half()))
    with pytest.raises(TypeError):
        bev.image_letterbox(dev.float(), geo, "yolox")
    with pytest.raises(ValueError):
        bev.image_letterbox(dev[:, :40], geo, "yolox")                                  # another source size
    with pytest.raises(ValueError):
        bev.image_letterbox(dev, geo, "yolox", out=torch.zeros(2, 3, 32, 32, device="cuda", dtype=torch.float16))
    with pytest.raises(ValueError):
        bev.image_letterbox(dev, geo, "yolox", channels_last=True, out=torch.zeros(2, 3, 64, 64, device="cuda"))


def test_raw_entry_and_graph_capture():
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    (H0, W0), (Hs, Ws), (Hp, Wp), (oy, ox) = (37, 53), (29, 42), (64, 96), (11, 16)
    imgs = [U.noise(20 + k, 2, H0, W0) for k in range(2)]
    raw = torch.from_numpy(imgs[0]).cuda()
    out = torch.full((2, 3, Hp, Wp), 5.0, device="cuda")
    D3 = ctypes.c_double * 3
    c = U.CENTERNET
    mean, std, pad = D3(*c["mean"]), D3(*c["std"]), D3(10.0, 20.0, 30.0)
    restate = lambda img, arith: U.letterbox(img, (Hs, Ws), (Hp, Wp), (oy, ox), arith, c["mean"], c["std"], True, (10.0, 20.0, 30.0))

    def call(stream, arith=1, hp=Hp, x=ox):
        return handle.bevops_image_letterbox(arith, raw.data_ptr(), L.F32, out.data_ptr(), 2, H0, W0, Hs, Ws, hp, Wp, oy, x,
                                             pad, mean, std, 1, 0, stream)

    st = L.current_stream_ptr(raw.device)
    assert call(st, hp=oy + Hs - 1) == L.BAD_PARAM and call(st, x=Wp - Ws + 1) == L.BAD_PARAM
    assert call(st, arith=2) == L.NOT_SUPPORTED
    assert (out == 5.0).all()                                               # refused before any device call
    for arith in (0, 1):
        assert call(st, arith=arith) == L.SUCCESS
        assert np.array_equal(bits(out), bits(restate(imgs[0], arith)))
    out.fill_(5.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert call(s.cuda_stream, arith=0) == L.SUCCESS                 # legal under capture: launch only
    torch.cuda.current_stream().wait_stream(s)
    for k in (1, 0):
        raw.copy_(torch.from_numpy(imgs[k]).cuda())                          # the replay follows the raw buffer
        graph.replay()
        assert np.array_equal(bits(out), bits(restate(imgs[k], 0)))
