"""bevops_lss_depth_head_f16 (csrc/depth_head.hip) through functions.lss_depth_head in the guarded arena of
tests/util_arena.py, against the float64 statement of tests/util_depth_head.py: the derived bounds on Gaussian operands
(design/depth_head.md), pads and extremes, column routing with one-hot rows, containment, and the D = 88 model."""
import numpy as np
import pytest
import torch

from util_arena import POISONS, Arena
from util_depth_head import CASES, operands, statement

pytestmark = pytest.mark.gpu
F16 = torch.float16


def launch(x, W, b, D, C, n, pitched=False):
    """One call per poison in a fresh arena (pitched: x is columns 8 .. of a buffer 40 wider) -> (depth [rows, D], feat)."""
    from bevformer_tensorrt_amd.functions.depth_head import lss_depth_head, pack_depth_head_tensors
    rows, Cin = x.shape
    got = []
    for poison in POISONS:
        A = Arena(8 << 20, poison)
        p = pack_depth_head_tensors(W, b, D, C)
        p = p._replace(w=A.place(p.w, 16, "w"), bias=A.place(p.bias, 16, "bias"))
        xb = A.empty((rows, Cin + (40 if pitched else 0)), F16, 16, "x")
        xs = xb[:, 8:8 + Cin] if pitched else xb
        xs.copy_(x)
        out = (A.empty((n, D, rows // n), F16, 2, "depth"), A.empty((n, rows // n, C), F16, 16, "feat"))
        lss_depth_head(xs, p, n, out=out)
        A.check()
        got.append((out[0].permute(0, 2, 1).reshape(rows, D).cpu(), out[1].reshape(rows, C).cpu()))
    assert all(torch.equal(a.view(torch.int16), c.view(torch.int16)) for a, c in zip(*got))
    return got[0]


def within(got, x, W, b, D, C):
    f, p, ef, ed = statement(x, W, b, D, C)
    depth, feat = (t.double().numpy() for t in got)
    rf, rd = np.abs(feat - f) / ef, np.abs(depth - p) / ed
    print(f"feat err / bound {rf.max():.3f}, depth err / bound {rd.max():.3f}, max |sum - 1| {np.abs(depth.sum(1) - 1).max():.2e}")
    assert np.isfinite(depth).all() and np.isfinite(feat).all()
    assert rf.max() <= 1 and rd.max() <= 1
    assert np.abs(depth.sum(1) - 1).max() <= D * 2.0 ** -11


@pytest.mark.parametrize("case,n,hw,pitched", [(c, n, hw, False) for c in CASES for n, hw in ((1, 1), (2, 45), (1, 129))]
                         + [(CASES[2], 2, 45, True)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gaussian_operands_within_the_derived_bound(case, n, hw, pitched):
    (Cin, C, D), (x, W, b) = case, operands(*case, n * hw)
    got = launch(x, W, b, D, C, n, pitched)
    within(got, x, W, b, D, C)
    assert D > 1 or bool((got[0] == 1.0).all())


@pytest.mark.parametrize("shift", [-30.0, 30000.0])
def test_pads_and_extremes(shift):
    """Depth biases at -30: a padded column (logit 0) that joined the maximum or the sum would take the whole mass;
    at +30000: exp overflows without the maximum subtraction."""
    (Cin, C, D), (x, W, b) = CASES[1], operands(*CASES[1], 90)
    b = torch.cat([(b[:D].float() + shift).half(), b[D:]])
    within(launch(x, W, b, D, C, 2), x, W, b, D, C)


def test_one_hot_rows_route_every_column():
    """x = I (row k selects input channel k), dyadic weights: v[k, j] = W[j, k] + b[j] exactly.  Depth row k % D of
    column k carries + 4, so pixel k's largest plane is k % D."""
    Cin, C, D, n = 256, 64, 88, 2
    j, k = torch.arange(D + C)[:, None], torch.arange(Cin)[None, :]
    W = ((j * 7 + k * 3) % 16 - 8).double() / 8
    W[:D] += 4.0 * (torch.arange(D)[:, None] == k % D)
    b = (torch.arange(D + C) % 5 - 2).double() / 4
    depth, feat = launch(torch.eye(Cin).half(), W.half(), b.half(), D, C, n)
    want = (W[D:].t() + b[D:]).half()
    assert torch.equal(feat.view(torch.int16), want.view(torch.int16))
    assert torch.equal(depth.argmax(1), torch.arange(Cin) % D)


def test_a_nan_stays_in_its_pixel():
    (Cin, C, D), (x, W, b) = CASES[2], operands(*CASES[2], 90)
    clean = launch(x, W, b, D, C, 2)
    x[50, 5] = float("nan")
    got = launch(x, W, b, D, C, 2)
    keep = torch.arange(90) != 50
    for a, c in zip(got, clean):
        assert not torch.isfinite(a[50]).any()
        assert torch.equal(a[keep].view(torch.int16), c[keep].view(torch.int16))


def test_the_d88_model_runs_the_fused_front():
    import bevformer_tensorrt_amd.functions as Fn
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDetRunner, jittered_rig
    cfg = dict(grid_config=dict(x=[-6.4, 6.4, 0.8], y=[-6.4, 6.4, 0.8], z=[-5, 3, 8], depth=[1.0, 45.0, 0.5]),
               input_size=(64, 176), downsample=16, in_channels=256, out_channels=64,
               occ_head=dict(Dz=4, num_classes=18, hidden=128))
    hip = BEVDet(cfg, seed=0, bev_half="hip").cuda().half()
    ref = BEVDet(cfg, seed=0, bev_half="torch").cuda().float()
    ref.load_state_dict({k: v.float() for k, v in hip.state_dict().items()})
    assert hip.prepare_bev_half() is hip and hip.view.D == 88
    g = torch.Generator().manual_seed(2)
    x = torch.randn(6, 256, 4, 11, generator=g).cuda().half().contiguous(memory_format=torch.channels_last)
    depth, feat = hip.view._depth_feat_hip(x)
    packed = Fn.pack_depth_head(hip.view.depth_net.weight, hip.view.depth_net.bias, 88, 64)
    d2, f2 = Fn.lss_depth_head(x.permute(0, 2, 3, 1).reshape(-1, 256), packed, 6, spatial=(4, 11))
    assert tuple(depth.shape) == (6, 88, 4, 11) and tuple(feat.shape) == (6, 4, 11, 64)
    assert torch.equal(depth.view(torch.int16), d2.view(torch.int16)) and torch.equal(feat.view(torch.int16), f2.view(torch.int16))
    rig = jittered_rig(hip.view, 1)
    calib = hip.view.calibration_matrices(*rig).cuda()
    got, want = hip.view.view_transform_calibrated(x, calib), ref.view.view_transform_calibrated(x.float(), calib)
    err, bar = float((got.float() - want).abs().max()), 3e-2 * max(1.0, float(want.abs().max()))
    print(f"BEV map: hip vs fp32 torch statements {err:.3e} (bar {bar:.3e})")
    assert got.shape == want.shape and err <= bar
    img = torch.randn(1, 6, 3, 64, 176, generator=g).cuda().half()
    want_occ = BEVDetRunner(hip, torch.device("cuda"), graph=False).step(img, *rig).clone()
    runner = BEVDetRunner(hip, torch.device("cuda"), graph=True)
    for _ in range(3):
        assert torch.equal(runner.step(img, *rig), want_occ)
    with torch.no_grad():
        hip.view.depth_net.bias.add_(0.0)                # a touched weight: the pack is stale, never rebuilt in a capture
    scratch = torch.zeros(8, device="cuda")
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="prepare_bev_half"):
            hip.forward_calibrated(img, calib)
