#!/usr/bin/env python3
"""Fixture of BEVStereo's DepthNet (bevformer_tensorrt_amd/bevdepth.py, functions/stereo.py): tests/golden/bevstereo.npz.
Build container only (needs the reference tree):

    python tests/golden/make_bevstereo_golden.py

The classes ASPP, _ASPPModule, Mlp, SELayer and DepthNet (with gen_grid, calculate_cost_volumn and forward) and the
method LSSViewTransformerBEVDepth.get_mlp_input are lifted from the reference's third_party/bev_mmdet3d/models/necks/
view_transformer.py by AST and EXECUTED on the CPU in fp32, in a child interpreter under tests/conftest.py's
PINNED_CPU_ENV.  No reference text is stored: the fixture holds the inputs, the state dict, the outputs, the key list.

mmdet's BasicBlock is not installed here: the script supplies conv1-bn1-relu-conv2-bn2-(downsample)-add-relu itself,
with mmdet's attribute names.  Parity with mmdet's own class is therefore NOT pinned by this fixture.

Sizes: 2 cameras of `jittered_rig` on a 32 x 48 image, a stride-4 stereo map of 8 x 12 with C = 8 post-ReLU-like features
(non-negative, about half exact zeros: gate == 0 fires inside the image too), D = 6 (depth 1 .. 6 m), mid = 32, a 2 x 3
stride-16 map.  k2s_sensor: a small ego motion for camera 0; camera 1 yawed by 35 degrees and moved back by 1.5 m (a
pure yaw cannot put one 60-degree volume partly inside the image AND partly behind the camera), so part of its volume
falls outside the image and part behind the z < 1e-3 plane.  bias 5 and 0, and the first frame (cv_feat_list[0] is None).

The reference's first-frame branch reads `self.depth_channels`, which its __init__ never sets: the script sets the
attribute before it runs that branch.

Also stored: the reference's own fp32 error.  `grid_err` = max |gen_grid fp32 - gen_grid float64| (the lifted method run on
float64 operands) over the positions whose float64 z is not within 1e-4 of the 1e-3 plane (asserted: at most 1 % are
left out); `cv_err` = max |calculate_cost_volumn fp32 - float64| with the float64 run fed the SAME fp32 grid."""
import ast
import math
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]

PATH = "third_party/bev_mmdet3d/models/necks/view_transformer.py"
PREFIX = "img_view_transformer.depth_net."
IMAGE, DEPTH, CV_DOWN, DOWN = (32, 48), [1.0, 7.0, 1.0], 4, 16
C_STEREO, MID, CONTEXT = 8, 32, 16


class BasicBlock(nn.Module):
    """mmdet's BasicBlock restated (stride 1): relu(bn2(conv2(relu(bn1(conv1(x))))) + (downsample(x) or x))."""

    def __init__(self, inplanes, planes, downsample=None):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(out)) + identity)


def lift_classes(names):
    import make_wrapper_golden as W
    tree = ast.parse(open(os.path.join(W.REF, PATH)).read())
    ns = {"torch": torch, "nn": nn, "F": torch.nn.functional, "BasicBlock": BasicBlock}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in names:
            exec(compile(ast.unparse(node), PATH, "exec"), ns)
            print(f"  lifted class {node.name} at {PATH}:{node.lineno}-{node.end_lineno}")
    return ns


def yaw_motion(deg, t):
    """A key-to-sweep sensor transform: rotation about the camera's y (down) axis and a translation."""
    a = math.radians(deg)
    m = torch.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    m[:3, 3] = torch.tensor(t)
    return m


def z_float64(metas):
    """The float64 z every frustum point has in front of the z < 1e-3 test (a restatement, used for the mask only)."""
    d = {k: v.double() for k, v in metas.items() if torch.is_tensor(v)}
    B, N, _ = d["post_trans"].shape
    p = d["frustum"] - d["post_trans"].view(B, N, 1, 1, 1, 3)
    p = torch.inverse(d["post_rots"]).view(B, N, 1, 1, 1, 3, 3).matmul(p.unsqueeze(-1))
    p = torch.cat((p[..., :2, :] * p[..., 2:3, :], p[..., 2:3, :]), 5)
    comb = d["k2s_sensor"][:, :, :3, :3].matmul(torch.inverse(d["intrins"]))
    p = comb.view(B, N, 1, 1, 1, 3, 3).matmul(p) + d["k2s_sensor"][:, :, :3, 3].reshape(B, N, 1, 1, 1, 3, 1)
    return p[..., 2, 0].reshape(B * N, *d["frustum"].shape[:3])


def record():
    import make_wrapper_golden as W
    from bevformer_tensorrt_amd.bevdet import jittered_rig, LSSViewTransformer
    ns = lift_classes(("_ASPPModule", "ASPP", "Mlp", "SELayer", "DepthNet"))
    get_mlp_input = W.lift(PATH, "LSSViewTransformerBEVDepth", "get_mlp_input")
    g = torch.Generator().manual_seed(2025)
    grid_config = dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=DEPTH)
    view = LSSViewTransformer(grid_config=grid_config, input_size=IMAGE, downsample=DOWN, in_channels=MID,
                              out_channels=CONTEXT, ops=object())
    D = view.D
    cv_frustum = view.create_frustum(DEPTH, IMAGE, CV_DOWN)
    view.D = D
    assert D == 6 and cv_frustum.shape == (6, 8, 12, 3)
    net = ns["DepthNet"](MID, MID, CONTEXT, D, use_dcn=False, stereo=True, bias=5.0).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            parent = name.split(".")[-2]
            is_bn = "bn" in parent or (name.startswith("reduce_conv") and parent == "1") or \
                (name.startswith("cost_volumn_net") and parent in ("1", "3")) or \
                (".global_avg_pool." in name and parent == "2")
            if p.dim() > 1:
                fan = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / fan ** 0.5))
            elif is_bn:
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g) if name.endswith("weight")
                        else 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.5 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    s2e, e2g, K, post_rots, post_trans, bda = jittered_rig(view, 5, n_cams=2)
    mlp_input = get_mlp_input(W.Stub(), s2e, e2g, K, post_rots, post_trans, bda)
    post_trans[0, :, 0] *= IMAGE[1] / 704.0          # the rig's crop jitter is sized for 704-wide images
    k2s = torch.stack([yaw_motion(1.5, [0.3, 0.02, 0.1]), yaw_motion(35.0, [0.1, -0.03, -1.5])]).view(1, 2, 4, 4)
    relu_like = lambda *shape: torch.relu(torch.randn(*shape, generator=g)) * 1.2
    prev, curr = relu_like(2, C_STEREO, 8, 12), relu_like(2, C_STEREO, 8, 12)
    curr = (0.5 * curr + 0.5 * prev.roll(1, 3)) * (curr > 0)        # correlated with its neighbour, still half zeros
    metas = dict(cv_feat_list=[prev, curr], k2s_sensor=k2s, intrins=K, post_rots=post_rots, post_trans=post_trans,
                 frustum=cv_frustum, downsample=DOWN, cv_downsample=CV_DOWN)
    res = {}
    with torch.no_grad():
        v = mlp_input.reshape(-1, 27)
        net.bn.running_mean.copy_(v.mean(0) * (1.0 + 0.05 * torch.randn(27, generator=g)))
        net.bn.running_var.copy_((0.02 * v.abs().mean(0) + 0.05) ** 2)
        x = torch.randn(2, MID, IMAGE[0] // DOWN, IMAGE[1] // DOWN, generator=g)
        grid = net.gen_grid(metas, 1, 2, D, 8, 12, 32, 48).view(2, D, 8, 12, 2)
        m64 = {k: (t.double() if torch.is_tensor(t) else t) for k, t in metas.items() if k != "cv_feat_list"}
        grid64 = net.gen_grid(m64, 1, 2, D, 8, 12, 32, 48).view(2, D, 8, 12, 2)
        z64 = z_float64(m64)
        near = (z64 - 1e-3).abs() <= 1e-4
        assert near.float().mean().item() <= 0.01
        behind = z64 < 1e-3
        assert 0.02 < behind[1].float().mean().item() < 0.9 and not behind[0].any()
        inside = (grid.abs() <= 1).all(-1)
        print(f"  in-image positions: camera 0 {inside[0].float().mean().item():.3f}, camera 1 {inside[1].float().mean().item():.3f}; "
              f"behind the plane in camera 1: {behind[1].float().mean().item():.3f}")
        assert 0.1 < inside[1].float().mean().item() < 0.95 and inside[0].float().mean().item() > 0.5
        grid_err = (grid.double() - grid64)[~near].abs().max().item()
        for tag, bias in (("b5", 5.0), ("b0", 0.0)):
            net.bias = bias
            cv = net.calculate_cost_volumn(metas)
            # float64 on the SAME fp32 grid: gen_grid replaced by the recorded grid for this one call
            m64cv = dict(m64, cv_feat_list=[prev.double(), curr.double()])
            keep = net.gen_grid
            net.gen_grid = lambda *a, **k: grid.double().view(2, D * 8, 12, 2)
            try:
                cv64 = net.calculate_cost_volumn(m64cv)
            finally:
                net.gen_grid = keep
            res["cv_" + tag] = cv.numpy()
            res["cv_err_" + tag] = np.float64((cv.double() - cv64).abs().max().item())
            res["out_" + tag] = net(x, mlp_input, metas).numpy()
            print(f"  bias {bias}: cost volume max-prob mean {cv.max(1).values.mean().item():.3f}, fp32 error "
                  f"{res['cv_err_' + tag]:.3e}")
            assert cv.max(1).values.mean().item() < 0.9         # not one-hot: neighbouring depths differ by O(1) in cost
        net.bias = 5.0
        net.depth_channels = D          # the reference reads it in the first-frame branch and never sets it
        out_first = net(x, mlp_input, dict(metas, cv_feat_list=[None, curr]))
    with torch.no_grad():
        import torch.nn.functional as F
        wp = F.grid_sample(prev[:, C_STEREO - 4:C_STEREO - 3], grid.view(2, D * 8, 12, 2), align_corners=True,
                           padding_mode="zeros").view(2, D, 8, 12)
        gate_zero = ((wp == 0) & inside).float().sum().item() / inside.float().sum().item()
    print(f"  gate == 0 at {100 * gate_zero:.1f} % of the in-image positions; grid fp32 error {grid_err:.3e}")
    assert 0.05 < gate_zero < 0.95
    assert out_first.shape == (2, D + CONTEXT, 2, 3) and bool(torch.isfinite(out_first).all())
    res.update({"x": x.numpy(), "mlp_input": mlp_input.numpy(), "prev": prev.numpy(), "curr": curr.numpy(),
                "k2s_sensor": k2s.numpy(), "intrins": K.numpy(), "post_rots": post_rots.numpy(),
                "post_trans": post_trans.numpy(), "cv_frustum": cv_frustum.numpy(), "grid": grid.numpy(),
                "grid_err": np.float64(grid_err), "near_plane": near.numpy(), "out_first": out_first.numpy(),
                "downsample": np.int64(DOWN), "cv_downsample": np.int64(CV_DOWN)})
    keys = []
    for k, t in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        keys.append(PREFIX + k)
        res["sd." + PREFIX + k] = t.numpy()
    res["keys"] = np.array(sorted(keys))
    path = os.path.join(HERE, "bevstereo.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(keys)} tensors")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pinned":
        record()
        raise SystemExit(0)
    from conftest import PINNED_CPU_ENV
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "pinned"], env=dict(os.environ, **PINNED_CPU_ENV))
