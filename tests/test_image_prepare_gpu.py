"""bevops_image_resize_crop_normalize (BEVDet's camera front end: PIL-exact resize, crop, flip, normalise in one
launch) on the GPU: the canvases the reference's pipeline produced with PIL (tests/golden/image_prepare.npz) and the
numpy restatement (tests/util_image_prepare.py), bit for bit; the normalised output bit-equal to oracle/image_ref.py on
the canvas, fp16 == its RNE cast; tile edges (the kernel's tile is 32 x 16); the R50 geometry at full size; graph
capture; BEVDetRunner.step_raw.  Neither PIL nor the reference tree is read here."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
import util_image_prepare as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return golden("image_prepare")


def _geometry(gold, name):
    g = [int(v) for v in gold[f"{name}_geometry"]]
    return (g[0], g[1]), tuple(g[2:6]), bool(g[6])


def _check_all_forms(bev, raw, plan, flip, canvas_want):
    """Every output form of one call against the canvas: uint8 canvas, fp32 / fp16, planes / channels-last, out=."""
    want = U.normalized(canvas_want)
    want_t = torch.from_numpy(want)
    n = raw.shape[0]
    got, canvas = bev.image_resize_crop_normalize(raw, plan, flip=flip, dtype=torch.float32, canvas=True)
    assert canvas.dtype == torch.uint8 and np.array_equal(canvas.cpu().numpy(), canvas_want)
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for cl in (False, True):
        fmt = torch.channels_last if cl else torch.contiguous_format
        f = bev.image_resize_crop_normalize(raw, plan, flip=flip, dtype=torch.float32, channels_last=cl)
        h = bev.image_resize_crop_normalize(raw, plan, flip=flip, channels_last=cl)             # fp16 is the default
        assert f.is_contiguous(memory_format=fmt) and h.is_contiguous(memory_format=fmt) and h.dtype == torch.float16
        assert torch.equal(f.cpu(), want_t)
        assert torch.equal(h.cpu(), want_t.half())                                              # the RNE cast of the fp32
        big = torch.full((n + 2,) + tuple(want.shape[1:]), 7.0, dtype=torch.float16, device="cuda").contiguous(memory_format=fmt)
        filled = torch.zeros((n,) + tuple(canvas_want.shape[1:]), dtype=torch.uint8, device="cuda")
        r = bev.image_resize_crop_normalize(raw, plan, flip=flip, channels_last=cl, out=big[1:n + 1], canvas=filled)
        assert r[0].data_ptr() == big[1].data_ptr() and r[1] is filled
        assert torch.equal(big[1:n + 1].cpu(), want_t.half()) and np.array_equal(filled.cpu().numpy(), canvas_want)
        assert bool((big[0] == 7).all()) and bool((big[n + 1] == 7).all())                      # nothing outside the slice


@pytest.mark.parametrize("kind", ["noise", "checker"])
@pytest.mark.parametrize("name", list(U.CASES))
def test_fixture_cases_bit_exact(gold, name, kind):
    import bevformer_tensorrt_amd as bev
    dims, crop, flip = _geometry(gold, name)
    raw, want = gold[f"{name}_{kind}_raw"], gold[f"{name}_{kind}_canvas"]
    plan = bev.image_resize_plan(raw.shape[1], raw.shape[2], dims, crop, "cuda")
    _check_all_forms(bev, torch.from_numpy(raw).cuda(), plan, flip, want)


def test_raw_ctypes_call(gold):
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    name = "resize_test_flip"
    dims, crop, flip = _geometry(gold, name)
    raw, want = gold[f"{name}_checker_raw"], gold[f"{name}_checker_canvas"]
    n, H0, W0, _ = raw.shape
    geom = (H0, W0) + dims + crop
    size = handle.bevops_image_resize_plan_size(*geom)
    host = torch.empty(size // 4, dtype=torch.int32)
    assert handle.bevops_image_resize_plan_build(*geom, host.data_ptr(), size) == 0
    plan, img = host.cuda(), torch.from_numpy(raw).cuda()
    fH, fW = want.shape[1:3]
    out = torch.empty(n, 3, fH, fW, device="cuda")
    canvas = torch.empty(n, fH, fW, 3, dtype=torch.uint8, device="cuda")
    m, s = (ctypes.c_double * 3)(*U.MEAN), (ctypes.c_double * 3)(*U.STD)
    stream = torch.cuda.current_stream().cuda_stream
    st = handle.bevops_image_resize_crop_normalize(img.data_ptr(), plan.data_ptr(), size, L.F32, out.data_ptr(),
                                                   canvas.data_ptr(), n, *geom, 0, m, s, 1, int(flip), 0, stream)
    assert st == 0
    assert np.array_equal(canvas.cpu().numpy(), want)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), U.normalized(want).view(np.uint32))
    # a plan of another size is refused, and the output stays as it is
    out.fill_(3.0)
    st = handle.bevops_image_resize_crop_normalize(img.data_ptr(), plan.data_ptr(), size - 4, L.F32, out.data_ptr(),
                                                   None, n, *geom, 0, m, s, 1, int(flip), 0, stream)
    assert st == 2 and bool((out == 3).all())


def test_tile_edges_sweep():
    """Output sizes below, at and above the 32 x 16 tile (and 1, 2, 3: one column / row of taps spans the whole source)
    from a 50 x 90 source, an unaligned batch of two; a few crops and flips on top."""
    import bevformer_tensorrt_amd as bev
    raw = np.concatenate([U.noise(3, 1, 50, 90), U.checkerboard(1, 50, 90)])
    dev = torch.from_numpy(raw).cuda()
    hcache, cases = {}, []
    for W in (1, 2, 3, 31, 32, 33, 63, 64, 65, 70):
        for H in (1, 2, 15, 16, 17, 24):
            cases.append((W, H, (0, 0, W, H), False))
    cases += [(65, 33, (1, 1, 64, 33), True), (70, 24, (33, 15, 66, 17), True), (33, 17, (32, 16, 33, 17), False),
              (180, 100, (10, 3, 171, 99), True)]
    for W, H, crop, flip in cases:
        if W not in hcache:                        # the horizontal pass is shared by every height
            hcache[W] = [U.pass1d(r, W) for r in raw]
        want = np.stack([U.pass1d(np.ascontiguousarray(t.transpose(1, 0, 2)), H).transpose(1, 0, 2)[crop[1]:crop[3], crop[0]:crop[2]]
                         for t in hcache[W]])
        want = np.ascontiguousarray(want[:, :, ::-1] if flip else want)
        plan = bev.image_resize_plan(50, 90, (W, H), crop, "cuda")
        got, canvas = bev.image_resize_crop_normalize(dev, plan, flip=flip, dtype=torch.float32, canvas=True)
        assert np.array_equal(canvas.cpu().numpy(), want), (W, H, crop, flip)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), U.normalized(want).view(np.uint32)), (W, H, crop, flip)


def test_r50_geometry_full_size():
    """900 x 1600 -> rows 140 .. 395 of 704 x 396, six cameras in one call (two distinct images)."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.bevdet import DATA_CONFIG_R50
    _, dims, crop, flip, _ = bev.bevdet_test_augmentation(900, 1600, DATA_CONFIG_R50)
    assert (dims, crop, flip) == ((704, 396), (0, 140, 704, 396), False)
    two = np.concatenate([U.noise(11, 1, 900, 1600), U.checkerboard(1, 900, 1600)])
    want2 = np.stack([U.prepare(r, dims, crop, False) for r in two])
    assert (want2[1] == 0).any() and (want2[1] == 255).any()
    order = [0, 1, 1, 0, 0, 1]
    raw = torch.from_numpy(two).cuda()[order].contiguous()
    plan = bev.image_resize_plan(900, 1600, dims, crop, "cuda")
    out, canvas = bev.image_resize_crop_normalize(raw, plan, channels_last=True, canvas=True)
    want = want2[order]
    assert np.array_equal(canvas.cpu().numpy(), want)
    assert torch.equal(out.cpu(), torch.from_numpy(U.normalized(want)).half())
    flipped = bev.image_resize_crop_normalize(raw[:1], plan, flip=True, dtype=torch.float32)
    assert torch.equal(flipped.cpu(), torch.from_numpy(U.normalized(want[:1, :, ::-1])))


def test_graph_capture_follows_the_raw_buffer(gold):
    import bevformer_tensorrt_amd as bev
    name = "crop_h_scale"
    dims, crop, flip = _geometry(gold, name)
    frames = [(gold[f"{name}_{k}_raw"], gold[f"{name}_{k}_canvas"]) for k in ("noise", "checker")]
    plan = bev.image_resize_plan(90, 160, dims, crop, "cuda")
    raw = torch.from_numpy(frames[0][0]).cuda()
    out = torch.zeros(raw.shape[0], 3, 24, 70, dtype=torch.float16, device="cuda")
    canvas = torch.zeros(raw.shape[0], 24, 70, 3, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bev.image_resize_crop_normalize(raw, plan, flip=flip, out=out, canvas=canvas)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):             # a synchronisation or an allocation by the call would fail the capture
        bev.image_resize_crop_normalize(raw, plan, flip=flip, out=out, canvas=canvas)
    for src, want in (frames[1], frames[0], frames[1]):
        raw.copy_(torch.from_numpy(src))
        out.zero_()
        canvas.zero_()
        graph.replay()
        assert np.array_equal(canvas.cpu().numpy(), want)
        assert torch.equal(out.cpu(), torch.from_numpy(U.normalized(want)).half())


@pytest.fixture
def reproducible_dispatch():
    """Frames are compared bit for bit below: the rule-based dispatch of the dense layers (functions/linear.py:
    DETERMINISTIC) is a function of the problem alone, as in tests/test_lss_prepare_gpu.py."""
    from bevformer_tensorrt_amd.functions import linear as Ln
    was = Ln.DETERMINISTIC["enabled"]
    Ln.DETERMINISTIC["enabled"] = True
    try:
        yield
    finally:
        Ln.DETERMINISTIC["enabled"] = was


def test_runner_step_raw(reproducible_dispatch):
    """A 450 x 800 raw frame -> resize 0.88 -> 704 x 396 -> rows 140 .. 395, flipped: step_raw == step on the prepared
    image with the post-transform the augmentation implies; `step` on a runner without raw_size is what it was."""
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDetRunner, synthetic_rig
    dev = torch.device("cuda")
    model = BEVDet(seed=0).cuda().half()
    s2e, e2g, K, _, _, bda = synthetic_rig(model.view)
    raws = [torch.from_numpy(np.concatenate([U.noise(20 + k, 3, 450, 800), U.checkerboard(3, 450, 800, 7 + k)])).cuda()
            for k in range(2)]
    runner = BEVDetRunner(model, dev, graph=True, post="bboxes", raw_size=(450, 800), flip=True)
    assert (runner.resize, runner.resize_dims, runner.crop, runner.flip) == (0.88, (704, 396), (0, 140, 704, 396), True)
    post_rot, post_tran = bev.bevdet_post_transform(0.88, (0, 140, 704, 396), True)
    assert torch.equal(runner.post_rot, post_rot) and torch.equal(runner.post_tran, post_tran)
    assert post_rot[0, 0] == -torch.tensor(0.88) and post_tran.tolist() == [704.0, -140.0, 0.0]
    post_rots, post_trans = post_rot.view(1, 1, 3, 3).repeat(1, 6, 1, 1), post_tran.view(1, 1, 3).repeat(1, 6, 1)
    plain = BEVDetRunner(model, dev, graph=True, post="bboxes")
    plan = bev.image_resize_plan(450, 800, (704, 396), (0, 140, 704, 396), dev)
    for k in (0, 1):
        got = runner.step_raw(raws[k], s2e, e2g, K, bda)
        prepared = bev.image_resize_crop_normalize(raws[k], plan, flip=True)[None]
        assert torch.equal(runner.image_buffer, prepared)
        assert torch.equal(runner.raw_buffer, raws[k])
        want = runner.step(prepared, s2e, e2g, K, post_rots, post_trans, bda)
        base = plain.step(prepared, s2e, e2g, K, post_rots, post_trans, bda)
        assert len(got) == len(want) == len(base) == 11
        for a, b, c in zip(got, want, base):
            assert torch.equal(a, b) and torch.equal(b, c)
    assert plain.raw_buffer is None and plain._graph is not None and plain._graph_raw is None
    assert runner._graph is not None and runner._graph_raw is not None
    with pytest.raises(RuntimeError):
        plain.step_raw(raws[0], s2e, e2g, K, bda)
    # the caller may fill the static raw buffer itself
    runner.raw_buffer.copy_(raws[1])
    again = runner.step_raw(runner.raw_buffer, s2e, e2g, K, bda)
    for a, b in zip(again, runner.step_raw(raws[1], s2e, e2g, K, bda)):
        assert torch.equal(a, b)
