"""BEVDet(BEVDET_OCC_R50) shrunk (64 x 176 cameras, a 16 x 16 x 16 grid of 0.4 m cells, synthetic weights): the 3-D BEV half on
bevops_conv3d_slice_f16 against the fp32 plain path, gated at 1.25 x the error of the plain fp16 library path; occ where the
fp32 top-two gap exceeds the two logits' summed bar (2 x 3e-2, the model tests' per-output bar, which the logits are held
to as well); every conv3d launch of the forward against its float64 statement within tests/test_conv3d_gpu.py's derived
bound; BEVDetRunner replay against eager; the refusals; a default BEVDet() never imports the 3-D module."""
import contextlib
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_conv3d_gpu import bound64, conv64, ref64

pytestmark = pytest.mark.gpu
BAR, GATE, LAUNCHES = 3e-2, 1.25, 18       # 18 = blocks (2) + (3 + 2) + (3 + 2 * 3) convolutions, fpn conv, final_conv
# synthetic weights: the default initialisation leaves a pooled volume of rms 4e-4 and bias-only logits (one class).  The
# pooled features, the 3-D convolutions and the predicter's last layer are scaled so that the levels are of order 1 and
# the classes spread; chosen on the fp32 plain path: 8 classes seen, 2.8 % of the voxels under the gap
FEAT_SCALE, CONV_SCALE, LAST_SCALE = 256.0, 3.0, 8.0


def _cfg():
    from bevformer_tensorrt_amd.bevdet import BEVDET_OCC_R50
    grid = dict(BEVDET_OCC_R50["grid_config"], x=[-3.2, 3.2, 0.4], y=[-3.2, 3.2, 0.4])
    return dict(BEVDET_OCC_R50, input_size=(64, 176), grid_config=grid)


@pytest.fixture(scope="module")
def setup():
    from bevformer_tensorrt_amd import functions
    from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig
    probe, calls = types.SimpleNamespace(**vars(functions)), []

    def conv3d_taps(x, w, bias=None, act="relu", residual=None, stride=1, out=None):
        got = functions.conv3d_taps(x, w, bias, act, residual, stride, out)
        calls.append((x.clone(), w, bias, act, None if residual is None else residual.clone(), stride, got.clone()))
        return got
    probe.conv3d_taps = conv3d_taps
    hip = BEVDet(_cfg(), ops=probe, seed=0, bev_half="hip").cuda().half()
    with torch.no_grad():
        D = hip.view.D
        hip.view.depth_net.weight[D:].mul_(FEAT_SCALE)
        hip.view.depth_net.bias[D:].mul_(FEAT_SCALE)
        for conv in hip.bev3d.convs():
            conv.weight.mul_(CONV_SCALE)
        hip.bev3d.predicter[2].weight.mul_(LAST_SCALE)
    models = {"hip": hip}
    for name, dtype in (("f16", torch.float16), ("f32", torch.float32)):       # the library path, fp16 and fp32
        models[name] = BEVDet(_cfg(), seed=0, bev_half="torch").cuda().to(dtype)
        models[name].load_state_dict({k: v.to(dtype) for k, v in hip.state_dict().items()})
    rig = jittered_rig(hip.view, 1)
    img = torch.randn(1, 6, 3, 64, 176, generator=torch.Generator().manual_seed(1)).cuda()
    calib = hip.view.calibration_matrices(*rig).cuda()
    return types.SimpleNamespace(calls=calls, rig=rig, img=img, calib=calib, **models)


def _by_hand(m, img, calib):
    """forward_calibrated's steps with the three backbone levels and the logits kept -> (occ, [levels..., logits])."""
    from bevformer_tensorrt_amd.bevdet import _rule_dispatch
    # (the hip route takes the image half's convolutions by rule, as forward_calibrated does)
    with torch.no_grad(), _rule_dispatch() if m.bev_half == "hip" else contextlib.nullcontext():
        pooled = m.view.view_transform_calibrated(m.image_features(img[0].to(next(m.parameters()).dtype)), calib)
        hip = m._bev_half_ready(pooled) and pooled.is_contiguous(memory_format=torch.channels_last)
        kept = []
        y = m.bev3d.encode(pooled, m.ops, hip, kept)
        occ, lg = m.bev3d.head(y, m.ops, m._head_operands() if m._occ_fast(y) else None, logits=True)
    return hip, occ, [t.float() for t in kept + [lg]]


def test_error_gate_and_occ(setup):
    s = setup
    del s.calls[:]
    hip_on, occ, got = _by_hand(s.hip, s.img, s.calib)
    assert hip_on and len(s.calls) == LAUNCHES
    _, _, lib = _by_hand(s.f16, s.img, s.calib)
    on32, occ32, want = _by_hand(s.f32, s.img, s.calib)
    assert not on32 and occ.dtype == torch.uint8 and tuple(occ.shape) == tuple(occ32.shape) == (1, 16, 16, 16)
    assert torch.equal(occ, s.hip.forward_calibrated(s.img.half(), s.calib))
    rms = lambda a, b: float((a - b).pow(2).mean().sqrt())
    for name, g, l, w in zip(("level0", "level1", "level2", "logits"), got, lib, want):
        e_hip, e_lib = rms(g, w), rms(l, w)
        print(f"{name}: rms error hip {e_hip:.3e}, library fp16 {e_lib:.3e}, ratio {e_hip / e_lib:.3f}, rms value {rms(w, 0 * w):.3f}")
        assert e_hip <= GATE * e_lib
    lg = want[3]
    print(f"logits: max error hip {float((got[3] - lg).abs().max()):.3e} (bar {BAR})")
    assert float((got[3] - lg).abs().max()) <= BAR
    top = lg.topk(2, -1).values
    sure = ((top[..., 0] - top[..., 1]) > 2 * BAR).permute(0, 3, 2, 1)            # [B, Dz, Dy, Dx] -> occ's [B, Dx, Dy, Dz]
    left = 1.0 - float(sure.float().mean())
    print(f"occ: left out {left:.4f}, classes seen {occ32.unique().numel()}, {int((occ[sure] != occ32[sure]).sum())} differ")
    assert left < 0.05 and occ32.unique().numel() > 2 and torch.equal(occ[sure], occ32[sure])


def test_every_launch_against_its_statement(setup):
    s = setup
    if not s.calls:
        s.hip.forward_calibrated(s.img.half(), s.calib)
    assert len(s.calls) >= LAUNCHES
    t = lambda a: np.float64(a.permute(0, 2, 3, 4, 1).cpu().numpy())
    for x, w, bias, act, res, stride, out in s.calls[:LAUNCHES]:
        x64, w64, b64 = t(x), np.float64(w.cpu().numpy()), np.float64(bias.detach().cpu().numpy())
        r64 = None if res is None else t(res)
        ref = ref64(x64, w64, b64, r64, stride, act == "relu")
        S = conv64(np.abs(x64), np.abs(w64), stride) + np.abs(b64) + (0.0 if res is None else np.abs(r64))
        assert (np.abs(t(out) - ref) <= bound64(ref, S, w64[0].size)).all(), (tuple(x.shape), tuple(w.shape), stride)


def test_runner_replay_equals_eager(setup):
    from bevformer_tensorrt_amd.bevdet import BEVDetRunner
    s = setup
    want = BEVDetRunner(s.hip, torch.device("cuda"), graph=False).step(s.img.half(), *s.rig).clone()
    runner = BEVDetRunner(s.hip, torch.device("cuda"), graph=True)
    for _ in range(3):
        got = runner.step(s.img.half(), *s.rig)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (1, 16, 16, 16) and torch.equal(got, want)


def test_refusals(setup):
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.bevdet import BEVDet
    with pytest.raises(RuntimeError, match="get_bboxes: an occupancy model"):
        setup.hip.get_bboxes(torch.zeros(1, 16, 16, 16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(NotImplementedError, match="build_int8_bevdet: an occupancy model"):
        Q.build_int8_bevdet(setup.hip, torch.device("cuda"), [])
    with pytest.raises(NotImplementedError, match="BEVDet-Occ 4D"):
        BEVDet(dict(_cfg(), temporal=dict(num_adj=1, pre_process=True)))


def test_default_model_never_imports_the_3d_half():
    code = ("import sys, torch; from bevformer_tensorrt_amd.bevdet import BEVDet, jittered_rig; "
            "m = BEVDet(bev_half='hip').cuda().half(); calib = m.view.calibration_matrices(*jittered_rig(m.view, 1)).cuda(); "
            "out = m.forward_calibrated(torch.zeros(1, 6, 3, 256, 704, device='cuda').half(), calib); torch.cuda.synchronize(); "
            "assert len(out) == 6 and 'bevformer_tensorrt_amd.bevdet_occ3d' not in sys.modules; print('clean')")
    done = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "clean" in done.stdout, done.stderr[-2000:]
