"""BEVDet with an occupancy head (FLASHOCC_R50 reduced: 256 x 704 cameras, a 48 x 48 BEV grid, hidden 128, Dz 4): the fast
path's occ against the fp32 plain path wherever the plain top-two gap exceeds the model tests' 3e-2 bar, the head launch
against its own statement on the tensors the forward fed it, BEVDetRunner replay against eager at batch 1 and 2, the
launch count, the refusals, and BEVDet()'s six maps bit for bit against the parent commit's."""
import types

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from util_occ_head import bound, decided, statement

pytestmark = pytest.mark.gpu
BAR = 3e-2
LAST_SCALE = 8.0       # the predictor's last layer of the synthetic weights, scaled so that <= 10 % of the gaps lie under BAR


def _cfg():
    from bevformer_tensorrt_amd.bevdet import FLASHOCC_R50
    grid = dict(FLASHOCC_R50["grid_config"], x=[-9.6, 9.6, 0.4], y=[-9.6, 9.6, 0.4])
    return dict(FLASHOCC_R50, grid_config=grid, occ_head=dict(Dz=4, num_classes=18, hidden=128))


class _Probe:
    """The package's operator set with occ_head_nhwc recorded: (y, packed, out) of every call."""

    def __init__(self):
        from bevformer_tensorrt_amd import functions
        self.__dict__.update(vars(functions))
        self.calls = []
        real = functions.occ_head_nhwc

        def occ_head_nhwc(y, packed, logits=False, out=None):
            got = real(y, packed, logits, out)
            self.calls.append((y.clone(), packed, out.clone()))
            return got
        self.occ_head_nhwc = occ_head_nhwc


@pytest.fixture(scope="module")
def setup():
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    probe = _Probe()
    hip = BEVDet(_cfg(), ops=probe, seed=0, bev_half="hip").cuda().half()
    with torch.no_grad():
        hip.predicter[2].weight.mul_(LAST_SCALE)
        hip.predicter[2].bias.mul_(LAST_SCALE)
    ref = BEVDet(_cfg(), seed=0, bev_half="torch").cuda().float()
    ref.load_state_dict({k: v.float() for k, v in hip.state_dict().items()})
    rigs = [jittered_rig(hip.view, k) for k in (1, 2)]
    imgs = torch.randn(2, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda()
    return types.SimpleNamespace(hip=hip, ref=ref, rigs=rigs, imgs=imgs, probe=probe)


class _Aten(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
        self.names.append(str(func))
        return func(*args, **(kwargs or {}))


def test_fast_path_against_the_fp32_plain_path(setup):
    from bevformer_tensorrt_amd.functions import occ_head_plain
    s, w = setup, setup.ref._occ_weights()
    calib = s.hip.view.calibration_matrices(*s.rigs[0]).cuda()
    del s.probe.calls[:]
    occ = s.hip.forward_calibrated(s.imgs[:1].half(), calib)
    want = s.ref.forward_calibrated(s.imgs[:1], calib)
    assert occ.dtype == torch.uint8 and tuple(occ.shape) == tuple(want.shape) == (1, 48, 48, 4) and len(s.probe.calls) == 1
    # the plain path once more, by hand, for its logits: occ[b, x, y] is pixel (row y, column x) of the map
    with torch.no_grad():
        feat = s.ref.bev_encoder(s.ref.view.view_transform_calibrated(s.ref.image_features(s.imgs[0]), calib))
        y32 = torch.relu(torch.nn.functional.conv2d(feat, s.ref.final_conv.weight, s.ref.final_conv.bias, 1, 1))
        o32, lg = occ_head_plain(y32, *w, logits=True)
    assert torch.equal(o32.permute(0, 2, 1, 3), want)
    top = lg.view(1, 48, 48, 4, 18).topk(2, -1).values
    sure = ((top[..., 0] - top[..., 1]) > BAR).permute(0, 2, 1, 3)
    left = 1.0 - float(sure.float().mean())
    wrong = int((occ[sure] != want[sure]).sum())
    print(f"flashocc reduced: left out {left:.4f}, {wrong} of {int(sure.sum())} decided voxels differ, "
          f"classes seen {want.unique().numel()}, logit spread {float(lg.std()):.3f}")
    assert left <= 0.10 and want.unique().numel() > 2
    assert wrong == 0
    # the launch inside the forward against its own statement on the tensors it was fed
    y, packed, out = s.probe.calls[0]
    rows = y.permute(0, 2, 3, 1).reshape(-1, 256)
    ops = (rows, *w[:4])
    so, slg, _, sh = statement(*ops, 4, 18)
    ok = decided(slg, bound(*ops, slg, sh), 4, 18)
    got = out.reshape(-1, 4).cpu().long()
    print(f"head launch against its statement: decided {float(ok.float().mean()):.4f}, {int((got[ok] != so[ok]).sum())} differ")
    assert float(ok.float().mean()) > 0.9 and torch.equal(got[ok], so[ok])
    assert torch.equal(out, occ.permute(0, 2, 1, 3))


def test_one_launch_and_no_library_work_behind_the_neck(setup):
    s = setup
    feat = torch.randn(1, 256, 48, 48, device="cuda").half().contiguous(memory_format=torch.channels_last)
    s.hip._occ(feat)                                   # (operands packed)
    del s.probe.calls[:]
    with _Aten() as seen:
        s.hip._occ(feat)
    assert len(s.probe.calls) == 1
    heavy = [n for n in seen.names if any(k in n for k in ("mm", "convolution", "cat", "argmax", "softplus", "linear", "amax"))]
    assert not heavy, heavy


@pytest.mark.parametrize("batch", [1, 2])
def test_runner_replay_equals_eager(setup, batch):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    s = setup
    rig = tuple(torch.cat([s.rigs[k][i] for k in range(batch)], 0) for i in range(6))
    img = s.imgs[:batch].half()
    runner = BEVDetRunner(s.hip, torch.device("cuda"), graph=True, batch=batch)
    eager = BEVDetRunner(s.hip, torch.device("cuda"), graph=False, batch=batch)
    want = eager.step(img, *rig).clone()
    for _ in range(2):
        got = runner.step(img, *rig)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (batch, 48, 48, 4) and torch.equal(got, want)
    if batch == 2:                                     # a sample's occ does not depend on its neighbour
        one = BEVDetRunner(s.hip, torch.device("cuda"), graph=False).step(img[1:], *(t[1:] for t in rig))
        assert torch.equal(one[0], want[1])
    raw = torch.randint(0, 256, (batch, 6, 900, 1600, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    r_graph = BEVDetRunner(s.hip, torch.device("cuda"), graph=True, batch=batch, raw_size=(900, 1600))
    r_eager = BEVDetRunner(s.hip, torch.device("cuda"), graph=False, batch=batch, raw_size=(900, 1600))
    args = (raw if batch > 1 else raw[0], rig[0], rig[1], rig[2], rig[5])
    want_raw = r_eager.step_raw(*args).clone()
    assert torch.equal(r_graph.step_raw(*args), want_raw) and torch.equal(r_graph.step_raw(*args), want_raw)


def test_refusals(setup):
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDetRunner, FLASHOCC_R50
    s = setup
    occ = torch.zeros(1, 48, 48, 4, dtype=torch.uint8, device="cuda")
    for fn in (s.hip.get_bboxes, s.hip.get_candidates):
        with pytest.raises(RuntimeError, match="occupancy"):
            fn(occ)
    with pytest.raises(ValueError, match="occupancy"):
        BEVDetRunner(s.hip, torch.device("cuda"), post="bboxes")
    with pytest.raises(NotImplementedError, match="occupancy"):
        Q.build_int8_bevdet(s.hip, torch.device("cuda"), [])
    with pytest.raises(NotImplementedError, match="FlashOcc4D"):
        BEVDet(dict(_cfg(), temporal=dict(num_adj=1, pre_process=True)))
    assert not hasattr(s.hip, "shared_conv") and len(s.hip.heads) == 0
    with torch.no_grad():
        s.hip.predicter[2].bias.add_(0.0)              # a touched weight: the pack is stale, and never rebuilt in a capture
    calib, scratch = s.hip.view.calibration_matrices(*s.rigs[0]).cuda(), torch.zeros(8, device="cuda")
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            s.hip.forward_calibrated(s.imgs[:1].half(), calib)
    assert FLASHOCC_R50["occ_head"] == dict(Dz=16, num_classes=18, hidden=512)


@pytest.mark.parametrize("bev_half,want", [("hip", "3e4ebac5b4c92436"), ("torch", "406989d149b5f3de")])
def test_the_default_model_keeps_the_parent_commits_bits(bev_half, want):
    """BEVDet(seed=0) in fp16 on a fixed frame: sha256 over the six maps of forward_calibrated (dispatch by rule) and of a
    BEVDetRunner replay, against the digests the commit before this head gave (recorded twice there, on an MI355X)."""
    import hashlib
    from bevformer_tensorrt_amd import bevdet as D

    def digest(outs):
        h = hashlib.sha256()
        for t in outs:
            h.update(t.contiguous().cpu().numpy().tobytes())
        return h.hexdigest()[:16]
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(1)).cuda().half()
    m = D.BEVDet(seed=0, bev_half=bev_half).cuda().half()
    assert len(list(m.parameters())) == 178 and hasattr(m, "shared_conv") and not hasattr(m, "predicter")
    rig = D.jittered_rig(m.view, 1)
    with D._rule_dispatch():
        assert digest(m.forward_calibrated(img, m.view.calibration_matrices(*rig).cuda())) == want
        if bev_half == "hip":
            runner = D.BEVDetRunner(m, torch.device("cuda"), graph=True)
            runner.step(img, *rig)
            assert digest(runner.step(img, *rig)) == want
