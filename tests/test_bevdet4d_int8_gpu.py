"""quantization.build_int8_bevdet(<temporal model>, bev_half="int8") on the GPU at the configuration and the drive of
tests/test_bevdet4d_gpu.py: the model gate over a three-frame drive (rms error against the fp32 plain path at most 1.25 x
the fp32 fake-quant statement's, per head map), a frame's alignment call against its statement, BEVDet4DRunner's replay
against eager frames with the INT8 ring, the capture guard with a weight reload, BEVDEPTH4D_R50, and the fp16 temporal
model and the INT8 BEVDET_R50 keeping the bits they gave before the INT8 temporal model existed in the process."""
import pytest
import torch

import test_bevdet4d_gpu as T4
import util_bev_align as U

pytestmark = pytest.mark.gpu

NAMES = T4.NAMES


def _metas(view, rigs, T):
    """Per frame of the drive: (meta, transforms, slots, valid); slice t is frame f - t, invalid before the drive began."""
    from bevformer_tensorrt_amd.functions import bev_align_transform, pack_bev_align_meta
    out = []
    for f, rig in enumerate(rigs):
        tf = torch.zeros(1, T, 2, 3)
        slots, valid = [(f - t) % (T + 1) for t in range(1, T + 1)], [t <= f for t in range(1, T + 1)]
        for t in range(1, T + 1):
            if valid[t - 1]:
                tf[:, t - 1] = bev_align_transform(rig[0], rig[1], rigs[f - t][0], rigs[f - t][1], rig[5],
                                                   view.grid_lower_bound, view.grid_interval)
        out.append((pack_bev_align_meta(tf, slots, valid, f % (T + 1)), tf, slots, valid))
    return out


def _frames(fp, rigs, gen, depth):
    frames = []
    for rig in rigs[:2]:
        extra = (fp.view.get_mlp_input(*rig).cuda(),) if depth else ()
        frames.append((torch.randn(1, 6, 3, 256, 704, generator=gen).cuda().half(),
                       *(r.cuda() for r in fp.view.get_bev_pool_input(*rig)), *extra))
    return frames


@pytest.fixture(scope="module")
def imgs():
    return torch.randn(3, 1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()


@pytest.fixture(scope="module")
def before(imgs):
    """The fp16 BEVDET4D_R50 frame and the INT8 BEVDET_R50 frame, made before any INT8 temporal model is constructed."""
    from bevformer_tensorrt_amd.bevdet import BEVDet
    from bevformer_tensorrt_amd.functions import pack_bev_align_meta
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    fp4 = T4._build(1, "hip", torch.float16)
    rig = T4._drive(fp4.view, 1)[0]
    calib = fp4.view.calibration_matrices(*rig).cuda()
    meta = pack_bev_align_meta(torch.zeros(1, 1, 2, 3), [1], [0], 0).cuda()
    run4 = lambda: [o.clone() for o in fp4.forward_temporal(imgs[0], calib, fp4.new_history(1, "cuda", torch.float16), meta)]
    still = BEVDet(seed=0, bev_half="hip").cuda().half()
    q, _, _ = build_int8_bevdet(still, "cuda", _frames(still, [rig, rig], torch.Generator().manual_seed(2), False), "minmax",
                                bev_half="int8")
    runq = lambda: [o.clone() for o in q.forward_calibrated(imgs[0], calib)]
    return dict(run4=run4, runq=runq, bits4=run4(), bitsq=runq())


@pytest.fixture(scope="module", params=[1, 2])
def built(request, before, tmp_path_factory):
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    T = request.param
    fp = T4._build(T, "hip", torch.float16)
    rigs = T4._drive(fp.view)
    cache = str(tmp_path_factory.mktemp("calib") / "bevdet4d.calib")
    frames = _frames(fp, rigs, torch.Generator().manual_seed(3), False)
    model, _, note = build_int8_bevdet(fp, "cuda", frames, "minmax", bev_half="int8", calibration_cache=cache)
    again, _, note2 = build_int8_bevdet(fp, "cuda", [], "minmax", bev_half="int8", calibration_cache=cache)
    assert again.scales == model.scales and note2["calibration_frames"] == 0
    return dict(T=T, fp=fp, rigs=rigs, model=model, note=note)


def test_model_gate_over_a_drive_and_the_alignment_call(built, imgs):
    """Three frames through the int8 kernels, the fp32 fake-quant statement and the fp32 plain path, each with its own
    ring; the last frame's maps are gated.  The last frame's alignment call, replayed on the kernels' own operands:
    every byte within 0.5 + 8 * 2^-24 * sum_k w_k |p_k| of the float64 blend (design/bevdet4d_int8.md section 4)."""
    model, T, rigs = built["model"], built["T"], built["rigs"]
    n = built["note"]
    assert (n["int8_bev_half_layers"], n["bev_half_scale_sites"], n["calibration_frames"]) == (28, 30, 2)
    view = model.view
    rings = [model.new_history(1, "cuda"), model.new_history(1, "cuda"),
             torch.zeros(T + 1, 1, 64, 128, 128, device="cuda")]
    assert rings[0].dtype == torch.int8 and rings[0][0].is_contiguous(memory_format=torch.channels_last)
    for f, (rig, (meta, tf, slots, valid)) in enumerate(zip(rigs, _metas(view, rigs, T))):
        x = model._features(imgs[f])
        ranks = [r.cuda() for r in view.get_bev_pool_input(*rig)]
        ring_before, live = rings[0].clone(), {"hist": rings[0], "meta": meta.cuda()}
        got = model.bev_half_calibrated(x, view.calibration_matrices(*rig).cuda(), live)
        fq = model.fake_quant_reference(x, ranks, tensors={"hist": rings[1], "meta": meta})
        ref = model.fake_quant_reference(x, ranks, quantize=False, tensors={"hist": rings[2], "meta": meta})
    assert all(valid) and tf[0, 0, 0, 2].abs() > 1 and bool(rings[0].any()) and bool(rings[2].any())
    for name, g, q, r in zip(NAMES, got, fq, ref):
        e_k, e_f = _rms(g.float(), r), _rms(q, r)
        print(f"num_adj {T} {name}: rms error kernels {e_k:.4e}, fake-quant statement {e_f:.4e}, ratio {e_k / e_f:.3f}; max "
              f"error {float((g.float() - r).abs().max()):.3e} (the fp16 model's bar {3e-2 * max(1.0, float(r.abs().max())):.3e})")
    for name, g, q, r in zip(NAMES, got, fq, ref):
        assert 0 < _rms(q, r) and _rms(g.float(), r) <= 1.25 * _rms(q, r), name
    k = model._align_index("test")
    curr, stack = live[model.plan.layers[k].src].cpu(), live["stack"].cpu()
    exact, mag = U.ref_align(curr, ring_before.cpu(), tf.tolist(), [slots], [valid])
    err = (stack.double() - exact).abs()
    print(f"num_adj {T} alignment call: max error {err.max().item():.6f}, inside {(mag[:, 64:] > 0).double().mean().item():.2f}")
    assert stack.dtype == torch.int8 and bool((err <= 0.5 + 8 * 2.0 ** -24 * mag).all()) and bool((mag[:, 64:] > 0).any())
    assert torch.equal(stack[:, :64], curr) and torch.equal(rings[0][(len(rigs) - 1) % (T + 1)].cpu(), curr)


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def test_runner_replay_equals_eager_over_a_drive(built, imgs):
    from bevformer_tensorrt_amd.bevdet import BEVDet4DRunner
    model, rigs = built["model"], built["rigs"]
    runner = BEVDet4DRunner(model, torch.device("cuda"), graph=True)
    eager = BEVDet4DRunner(model, torch.device("cuda"), graph=False)
    assert runner.hist.dtype == torch.int8
    for i, f in enumerate((0, 1, 2, 1)):                        # the last one restarts the sequence
        out = runner.step(imgs[f], *rigs[f], start_of_sequence=i == 3)
        want = eager.step(imgs[f], *rigs[f], start_of_sequence=i == 3)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, out, want):
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), (f, n)
        assert torch.equal(runner.hist, eager.hist) and bool(runner.hist.any())
    graph = runner._graph
    with T4._Uploads() as probe:
        runner.step(runner.image_buffer, *rigs[2])
    assert probe.count == 1 and runner._graph is graph


def test_capture_guard_and_weight_reload(built, imgs):
    from bevformer_tensorrt_amd.functions import pack_bev_align_meta
    model, T = built["model"], built["T"]
    calib = model.view.calibration_matrices(*built["rigs"][0]).cuda()
    meta = pack_bev_align_meta(torch.zeros(1, T, 2, 3), list(range(1, T + 1)), [0] * T, 0).cuda()
    a = [o.clone() for o in model.forward_temporal(imgs[0], calib, model.new_history(1, "cuda"), meta)]
    with torch.no_grad():
        model.fp.pre_process_net[1].conv2.weight.mul_(0.5)
    assert model.operands(build=False) is None
    scratch, hist = torch.zeros(8, device="cuda"), model.new_history(1, "cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.forward_temporal(imgs[0], calib, hist, meta)
    del graph
    b = model.forward_temporal(imgs[0], calib, hist, meta)
    assert not torch.equal(a[5], b[5])
    with torch.no_grad():
        model.fp.pre_process_net[1].conv2.weight.mul_(2.0)


def test_bevdepth4d_builds_and_runs_a_frame(before, imgs):
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDEPTH4D_R50
    from bevformer_tensorrt_amd.functions import pack_bev_align_meta
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    fp = BEVDet(BEVDEPTH4D_R50, seed=0, bev_half="hip").cuda().half()
    rig = T4._drive(fp.view, 1)[0]
    model, _, note = build_int8_bevdet(fp, "cuda", _frames(fp, [rig, rig], torch.Generator().manual_seed(4), True), "minmax",
                                       bev_half="int8")
    assert model.num_adj == 1 and note["bev_half_scale_sites"] == len(model.plan.sites) == len(model.scales)
    hist = model.new_history(1, "cuda")
    meta = pack_bev_align_meta(torch.zeros(1, 1, 2, 3), [1], [0], 0).cuda()
    calib = fp.view.calibration_matrices(*rig).cuda()
    out = model.forward_temporal(imgs[0], calib, hist, meta)
    curr = model.bev_feature_calibrated(imgs[0], calib)
    assert curr.dtype == torch.int8 and tuple(curr.shape) == (1, 64, 128, 128) and torch.equal(hist[0], curr)
    assert all(o.dtype == torch.float16 and o.shape[2:] == (128, 128) and bool(o.isfinite().all()) for o in out)
    assert float(out[5].float().abs().max()) > 0


def test_the_other_models_keep_their_bits(before, built):
    for key, run in (("bits4", "run4"), ("bitsq", "runq")):
        for name, a, b in zip(NAMES, before[key], before[run]()):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (key, name)
