"""bevops_image_normalize_resize_pad (the BEVFormer tiny / small camera front end: normalise, rescale, pad in one launch)
on the GPU against the numpy restatement (tests/util_image_scale.py): fp32 output bit for bit in both layouts, fp16 output
== the RNE cast of it, +0.0 padding, `out=` inside a guarded buffer; output sizes around the 64 x 8 tile edges from
sources with odd row lengths; scale = 1 == image_normalize_pad; the nuScenes geometry of tiny (area form) and small; the
raw C entry and graph capture; FrameRunner(raw_size=...)."""
import ctypes

import numpy as np
import pytest
import torch

import util_image_scale as U

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 8          # csrc/image_scale.hip: kTW, kTH


def bits(t):
    """Bit pattern of a float32 / float16 tensor or array (so that -0.0 != +0.0 and NaN == NaN)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def check_all_forms(img, size, norm, want=None):
    """Every output form of one input against the restatement; returns the restatement."""
    import bevformer_tensorrt_amd as bev
    if want is None:
        want = U.normalize_resize_pad(img, size, **norm)
    dev = torch.from_numpy(img).cuda()
    n, shape = img.shape[0], want.shape
    for cl in (False, True):
        f = bev.image_normalize_resize_pad(dev, size=size, dtype=torch.float32, channels_last=cl, **norm)
        h = bev.image_normalize_resize_pad(dev, size=size, channels_last=cl, **norm)            # fp16 is the default
        fmt = torch.channels_last if cl else torch.contiguous_format
        assert tuple(f.shape) == shape and f.is_contiguous(memory_format=fmt) and h.is_contiguous(memory_format=fmt)
        assert f.dtype == torch.float32 and h.dtype == torch.float16
        assert np.array_equal(bits(f), bits(want)), f"fp32, channels_last={cl}"                  # (padding: +0.0 bits)
        assert np.array_equal(bits(h), bits(torch.from_numpy(want).half())), f"fp16, channels_last={cl}"
        # out= a slice of a larger buffer: the guard images in front and behind stay untouched
        big = torch.full((n + 2,) + shape[1:], 7.0, device="cuda", dtype=torch.float32).contiguous(memory_format=fmt)
        r = bev.image_normalize_resize_pad(dev, size=size, channels_last=cl, out=big[1:n + 1], **norm)
        assert r.data_ptr() == big[1].data_ptr()
        assert np.array_equal(bits(big[1:n + 1]), bits(want))
        assert (big[0] == 7.0).all() and (big[n + 1] == 7.0).all()
    return want


@pytest.mark.parametrize("norm", ["base", "tiny"])
@pytest.mark.parametrize("src", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("case", list(U.CASES))
def test_cases_bit_exact(case, src, norm):
    (H0, W0), size = U.CASES[case]
    check_all_forms(U.noise(7, 2, H0, W0, dtype=src), size, U.NORMS[norm])


def test_scale_argument_is_scaled_size():
    import bevformer_tensorrt_amd as bev
    img = U.noise(5, 2, 45, 70)
    for s in (0.8, 0.5):
        want = U.normalize_resize_pad(img, U.scaled_size(45, 70, s), **U.TINY_NORM)
        got = bev.image_normalize_resize_pad(torch.from_numpy(img).cuda(), scale=s, dtype=torch.float32, **U.TINY_NORM)
        assert np.array_equal(bits(got), bits(want))
    with pytest.raises(ValueError):
        bev.image_normalize_resize_pad(torch.from_numpy(img).cuda(), scale=0.5, size=(22, 35))
    with pytest.raises(TypeError):
        bev.image_normalize_resize_pad(torch.from_numpy(img).cuda().half(), scale=0.5)
    with pytest.raises(ValueError):
        bev.image_normalize_resize_pad(torch.from_numpy(img).cuda(), scale=0.5,
                                       out=torch.zeros(2, 3, 32, 32, device="cuda", dtype=torch.float16))


@pytest.mark.parametrize("Hs", [TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1])
def test_tile_edges(Hs):
    """Output sizes around the tile edges, from a source 1.25 x as large whose odd W0 leaves raw rows off dword
    alignment (3 * W0 is odd)."""
    import bevformer_tensorrt_amd as bev
    for Ws in (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1):
        H0, W0 = -(-Hs * 5 // 4), (-(-Ws * 5 // 4)) | 1
        img = U.noise(Hs * 1000 + Ws, 2, H0, W0)
        want = U.normalize_resize_pad(img, (Hs, Ws), **U.TINY_NORM)
        dev = torch.from_numpy(img).cuda()
        for cl in (False, True):
            got = bev.image_normalize_resize_pad(dev, size=(Hs, Ws), dtype=torch.float32, channels_last=cl, **U.TINY_NORM)
            assert np.array_equal(bits(got), bits(want)), (Hs, Ws, cl)


@pytest.mark.parametrize("src", [np.uint8, np.float32], ids=["u8", "f32"])
def test_scale_one_equals_image_normalize_pad(src):
    import bevformer_tensorrt_amd as bev
    dev = torch.from_numpy(U.noise(3, 2, 45, 71, dtype=src)).cuda()
    for norm in (U.BASE_NORM, U.TINY_NORM):
        for cl in (False, True):
            for dt in (torch.float32, torch.float16):
                a = bev.image_normalize_resize_pad(dev, dtype=dt, channels_last=cl, **norm)
                b = bev.image_normalize_pad(dev, dtype=dt, channels_last=cl, **norm)
                assert a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_nuscenes_geometry(name):
    """6 x 900 x 1600 uint8 through the tiny (0.5: area form) and the small (0.8) pipeline, bit for bit."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.bevformer import CONFIGS
    p = bev.BEVFORMER_IMAGE_PIPELINES[name]
    img = U.noise(1, 6, 900, 1600)
    size = bev.scaled_size(900, 1600, p["scale"])
    want = U.normalize_resize_pad(img, size, p["mean"], p["std"], p["to_rgb"], p["size_divisor"])
    assert want.shape == (6, 3) + tuple(CONFIGS[name]["image"])
    assert U.is_area(900, 1600, *size) == (name == "tiny")
    dev = torch.from_numpy(img).cuda()
    kw = dict(scale=p["scale"], mean=p["mean"], std=p["std"], to_rgb=p["to_rgb"], size_divisor=p["size_divisor"])
    got = bev.image_normalize_resize_pad(dev, dtype=torch.float32, **kw)
    assert np.array_equal(bits(got), bits(want))
    half = bev.image_normalize_resize_pad(dev, channels_last=True, **kw)
    assert np.array_equal(bits(half), bits(torch.from_numpy(want).half()))


def test_raw_entry_and_graph_capture():
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    (H0, W0), (Hs, Ws) = (37, 53), (29, 42)
    Hp, Wp = U.padded(Hs, Ws)
    imgs = [U.noise(20 + k, 2, H0, W0) for k in range(2)]
    raw = torch.from_numpy(imgs[0]).cuda()
    out = torch.full((2, 3, Hp, Wp), 5.0, device="cuda")
    D3 = ctypes.c_double * 3
    mean, std = D3(*U.TINY_NORM["mean"]), D3(*U.TINY_NORM["std"])

    def call(stream, hp=Hp):
        return handle.bevops_image_normalize_resize_pad(L.U8, raw.data_ptr(), L.F32, out.data_ptr(), 2, H0, W0, Hs, Ws, hp,
                                                        Wp, mean, std, 1, 0, stream)

    assert call(L.current_stream_ptr(raw.device), hp=Hs - 1) == L.BAD_PARAM
    assert (out == 5.0).all()                                               # refused before any device call
    assert call(L.current_stream_ptr(raw.device)) == L.SUCCESS
    assert np.array_equal(bits(out), bits(U.normalize_resize_pad(imgs[0], (Hs, Ws), **U.TINY_NORM)))
    out.fill_(5.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert call(s.cuda_stream) == L.SUCCESS                          # legal under capture: launch only
    torch.cuda.current_stream().wait_stream(s)
    for k in (1, 0):
        raw.copy_(torch.from_numpy(imgs[k]).cuda())                          # the replay follows the raw buffer
        graph.replay()
        assert np.array_equal(bits(out), bits(U.normalize_resize_pad(imgs[k], (Hs, Ws), **U.TINY_NORM)))


# --------------------------------------------------------------------------- FrameRunner(raw_size=...)
@pytest.fixture(scope="module")
def tiny():
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    dev = torch.device("cuda")
    model = B.BEVFormer("tiny", seed=0).to(dev, torch.float16)
    g = torch.Generator().manual_seed(0)
    raws = [torch.randint(0, 256, (6, 900, 1600, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(3)]
    l2i = G.synthetic_lidar2img((900, 1600))          # the UNSCALED dataset calibration
    return model, dev, raws, l2i


def prepared(raw):
    import bevformer_tensorrt_amd as bev
    p = bev.BEVFORMER_IMAGE_PIPELINES["tiny"]
    return bev.image_normalize_resize_pad(raw, scale=p["scale"], mean=p["mean"], std=p["std"], to_rgb=p["to_rgb"],
                                          size_divisor=p["size_divisor"], dtype=torch.float16)


def test_frame_runner_step_raw_from_raw_frames(tiny):
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import bevformer as B
    model, dev, raws, l2i = tiny
    a = B.FrameRunner(model, dev, torch.float16, raw_size=(900, 1600))
    b = B.FrameRunner(model, dev, torch.float16)
    assert a.raw_buffer.shape == (6, 900, 1600, 3) and a.raw_buffer.dtype == torch.uint8 and b.raw_buffer is None
    cls_a, crd_a = a.step_raw(raws[0], torch.zeros(18), l2i, "s")
    pre = prepared(raws[0])
    assert torch.equal(a.image_buffer[0], pre)                      # the pre-processing itself is bit-identical
    scaled = bev.scale_lidar2img(l2i, 0.5)
    assert np.array_equal(bits(a._in["lidar2img"]), bits(scaled.reshape(1, 6, 4, 4)))
    cls_b, crd_b = b.step(pre[None], torch.zeros(18), scaled, "s")
    # the bars of tests/test_image_gpu.py for the same comparison (two runners may pick other library algorithms)
    assert (cls_a.float() - cls_b.float()).abs().max().item() <= 5e-2
    assert (crd_a.float() - crd_b.float()).abs().max().item() <= 0.5
    with pytest.raises(ValueError):
        a.step_raw(raws[0][:, :450], torch.zeros(18), l2i, "s")
    with pytest.raises(ValueError):
        a.step_raw(raws[0].float(), torch.zeros(18), l2i, "s")


def test_frame_runner_raw_graph_follows_the_raw_buffer(tiny):
    from bevformer_tensorrt_amd import bevformer as B
    model, dev, raws, l2i = tiny
    run = B.FrameRunner(model, dev, torch.float16, graph=True, raw_size=(900, 1600))
    eager = B.FrameRunner(model, dev, torch.float16, raw_size=(900, 1600))
    # every frame opens a new scene, so each one replays the SAME ("no history") graph
    outs = [run.step_raw(raws[k], torch.zeros(18), l2i, f"scene{k}") for k in range(2)]
    assert list(run._graphs_raw) == [0.0] and run._graphs == {}    # one capture, beginning with the prepare launch
    assert torch.equal(run.image_buffer[0], prepared(raws[1]))
    assert not torch.equal(outs[0][0], outs[1][0])
    run.raw_buffer.copy_(raws[2])
    ptr = run.raw_buffer.data_ptr()
    cls_g, crd_g = run.step_raw(run.raw_buffer, torch.zeros(18), l2i, "scene2")       # the buffer itself: no copy
    assert run.raw_buffer.data_ptr() == ptr and torch.equal(run.raw_buffer, raws[2])
    assert torch.equal(run.image_buffer[0], prepared(raws[2]))
    cls_e, crd_e = eager.step_raw(raws[2], torch.zeros(18), l2i, "scene2")
    assert (cls_g.float() - cls_e.float()).abs().max().item() <= 5e-2
    assert (crd_g.float() - crd_e.float()).abs().max().item() <= 0.5


def test_frame_runner_rejects_a_mismatching_raw_size(tiny):
    from bevformer_tensorrt_amd import bevformer as B
    model, dev, _, _ = tiny
    for bad in ((450, 800), (900, 1665), (1000, 1600)):
        with pytest.raises(ValueError):
            B.FrameRunner(model, dev, torch.float16, raw_size=bad)
