"""BEVDet(BEVDET4D_R50): bev_align_stack between the pooling and the widened BEV encoder.  forward_temporal on the fast
path (bev_half="hip") against the fp32 plain path at the bar of tests/test_bevdepth_gpu.py (3e-2 max(1, max|fp32|) per
map), num_adj 1 and 2; BEVDet4DRunner over a three-frame drive: replay equal to eager bit for bit, start_of_sequence,
one upload per frame; the capture guard and the two refusals.  256 x 704, six cameras: the sizes of that file."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("reg", "height", "dim", "rot", "vel", "heatmap")


def _cfg(num_adj):
    from bevformer_tensorrt_amd.bevdet import BEVDET4D_R50
    return dict(BEVDET4D_R50, temporal=dict(num_adj=num_adj, pre_process=True))


def _build(num_adj, bev_half, dtype, state=None):
    from bevformer_tensorrt_amd.bevdet import BEVDet
    m = BEVDet(_cfg(num_adj), seed=0, bev_half=bev_half).cuda().to(dtype)
    if state is not None:
        m.load_state_dict({k: v.to(dtype) for k, v in state.items()})
    return m


def _drive(view, frames=3):
    """The synthetic rig on an ego that drives forward and turns: per frame the six tensors of a rig."""
    import math
    from bevformer_tensorrt_amd.bevdet import synthetic_rig
    rigs = []
    for f in range(frames):
        s2e, e2g, K, pr, pt, bda = synthetic_rig(view)
        yaw = 0.04 * f
        pose = torch.eye(4)
        pose[0, 0], pose[0, 1], pose[1, 0], pose[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
        pose[0, 3], pose[1, 3] = 2.3 * f, 0.4 * f
        rigs.append((s2e, pose.view(1, 1, 4, 4).repeat(1, 6, 1, 1), K, pr, pt, bda))
    return rigs


@pytest.fixture(scope="module")
def imgs():
    return torch.randn(3, 1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda()


@pytest.mark.parametrize("num_adj", [1, 2])
def test_fast_path_against_the_fp32_plain_path(imgs, num_adj):
    from bevformer_tensorrt_amd.bevdet import HEADS_R50
    from bevformer_tensorrt_amd.functions import bev_align_transform, pack_bev_align_meta
    hip = _build(num_adj, "hip", torch.float16)
    ref = _build(num_adj, "torch", torch.float32, state=hip.state_dict())
    assert hip.bev_stages[0][0].conv1.in_channels == (num_adj + 1) * 64 and len(hip.pre_process_net) == 2
    rigs = _drive(hip.view)
    outs = {}
    for name, model, dtype in (("hip", hip, torch.float16), ("ref", ref, torch.float32)):
        hist = model.new_history(1, "cuda", dtype)
        for f, rig in enumerate(rigs):                 # frame f: slice t is frame f - t, invalid before the drive began
            tf = torch.zeros(1, num_adj, 2, 3)
            slots = [(f - t) % (num_adj + 1) for t in range(1, num_adj + 1)]
            valid = [t <= f for t in range(1, num_adj + 1)]
            for t in range(1, num_adj + 1):
                if valid[t - 1]:
                    tf[:, t - 1] = bev_align_transform(rig[0], rig[1], rigs[f - t][0], rigs[f - t][1], rig[5],
                                                       model.view.grid_lower_bound, model.view.grid_interval)
            meta = pack_bev_align_meta(tf, slots, valid, f % (num_adj + 1)).cuda()
            calib = model.view.calibration_matrices(*rig).cuda()
            outs[name] = model.forward_temporal(imgs[f].to(dtype), calib, hist, meta)
        assert tf[0, 0, 0, 2].abs() > 1 and hist.abs().sum() > 0          # the ego moved by cells; the ring is filled
    torch.cuda.synchronize()
    for (n, c), a, b in zip(HEADS_R50, outs["hip"], outs["ref"]):
        assert a.shape == b.shape == (1, c, 128, 128) and a.dtype == torch.float16, n
        err, bar = (a.float() - b).abs().max().item(), 3e-2 * max(1.0, b.abs().max().item())
        print(f"num_adj {num_adj} {n}: hip vs fp32 plain {err:.4e} (bar {bar:.4e})")
        assert err <= bar, (n, err, bar)


class _Uploads(torch.overrides.TorchFunctionMode):
    """Counts Tensor.copy_ calls from a host tensor into a device tensor."""

    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if func is torch.Tensor.copy_ and args[0].is_cuda and not args[1].is_cuda:
            self.count += 1
        return func(*args, **(kwargs or {}))


def test_runner_replay_equals_eager_over_a_drive(imgs):
    from bevformer_tensorrt_amd.bevdet import BEVDet4DRunner
    model = _build(1, "hip", torch.float16)
    rigs, frames = _drive(model.view), imgs.half()
    runner = BEVDet4DRunner(model, torch.device("cuda"), graph=True)
    eager = BEVDet4DRunner(model, torch.device("cuda"), graph=False)
    seen = []
    for f in (0, 1, 2, 1):                                      # the last one restarts the sequence
        restart = len(seen) == 3
        out = runner.step(frames[f], *rigs[f], start_of_sequence=restart)
        want = eager.step(frames[f], *rigs[f], start_of_sequence=restart)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, out, want):
            assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), (f, n)
        assert torch.equal(runner.hist.contiguous().view(torch.int16), eager.hist.contiguous().view(torch.int16))
        seen.append(out[5].clone())
    graph = runner._graph
    with _Uploads() as probe:
        runner.step(runner.image_buffer, *rigs[2])
    assert probe.count == 1 and runner._graph is graph
    # start_of_sequence resets validity: frame 1 as a sequence's first frame is frame 1 with the current map fed in
    # place of the past -- not what it gave behind frame 0
    fresh = BEVDet4DRunner(model, torch.device("cuda"), graph=False).step(frames[1], *rigs[1])
    torch.cuda.synchronize()
    assert torch.equal(seen[3], fresh[5]) and not torch.equal(seen[3], seen[1])


def test_capture_guard_and_refusals():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVSTEREO_R50, BEVDet4DRunner, BEVDET_R50, BEVDEPTH4D_R50
    from bevformer_tensorrt_amd.functions import pack_bev_align_meta
    model = _build(1, "hip", torch.float16)
    rig = _drive(model.view, 1)[0]
    calib = model.view.calibration_matrices(*rig).cuda()
    meta = pack_bev_align_meta(torch.zeros(1, 1, 2, 3), [1], [0], 0).cuda()
    hist = model.new_history(1, "cuda", torch.float16)
    img = torch.zeros(1, 6, 3, 256, 704, device="cuda", dtype=torch.float16)
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            model.forward_temporal(img, calib, hist, meta)
    del graph
    with pytest.raises(NotImplementedError, match="stride-4"):
        BEVDet(dict(BEVSTEREO_R50, temporal=dict(num_adj=1, pre_process=True)))
    with pytest.raises(NotImplementedError, match="temporal"):
        Q.build_int8_bevdet(model, torch.device("cuda"), [])
    with pytest.raises(ValueError, match="temporal"):
        BEVDet4DRunner(BEVDet(BEVDET_R50), torch.device("cuda"))
    assert BEVDEPTH4D_R50["view_transformer"] == "bevdepth" and BEVDEPTH4D_R50["temporal"]["num_adj"] == 1
