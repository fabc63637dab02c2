#!/usr/bin/env python3
"""Fixture of BEVDepth's DepthNet (bevformer_tensorrt_amd/bevdepth.py): tests/golden/bevdepth.npz.
Build container only (needs the reference tree):

    python tests/golden/make_bevdepth_golden.py

The classes ASPP, _ASPPModule, Mlp, SELayer and DepthNet and the method LSSViewTransformerBEVDepth.get_mlp_input are
lifted from the reference's third_party/bev_mmdet3d/models/necks/view_transformer.py by AST and EXECUTED on the CPU in
fp32, in a child interpreter under tests/conftest.py's PINNED_CPU_ENV.  No reference text is stored: the fixture holds
the inputs, the reference module's state dict (under the names its classes spell), its outputs and the key list.

mmdet's BasicBlock is not installed here: the script supplies conv1-bn1-relu-conv2-bn2-add-relu itself, with mmdet's
attribute names (conv1, bn1, conv2, bn2).  Parity with mmdet's own class is therefore NOT pinned by this fixture.

Sizes: 2 cameras, 16 channels, a 6 x 10 map, D = 8, C = 16 -- dilation 12 and 18 larger than the map, dilation 6 inside
it.  BatchNorm statistics and every parameter are randomised; all modules in eval mode (Dropout = identity)."""
import ast
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


class BasicBlock(nn.Module):
    """mmdet's BasicBlock restated (stride 1, no downsample): relu(bn2(conv2(relu(bn1(conv1(x))))) + x)."""

    def __init__(self, inplanes, planes, downsample=None):
        super().__init__()
        assert downsample is None and inplanes == planes
        self.conv1, self.bn1 = nn.Conv2d(inplanes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(out)) + x)


def lift_classes(names):
    import make_wrapper_golden as W
    tree = ast.parse(open(os.path.join(W.REF, PATH)).read())
    ns = {"torch": torch, "nn": nn, "F": torch.nn.functional, "BasicBlock": BasicBlock}
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name in names:
            exec(compile(ast.unparse(node), PATH, "exec"), ns)
            print(f"  lifted class {node.name} at {PATH}:{node.lineno}-{node.end_lineno}")
    return ns


def record():
    import make_wrapper_golden as W
    from bevformer_tensorrt_amd.bevdet import jittered_rig, LSSViewTransformer, BEVDET_R50
    ns = lift_classes(("_ASPPModule", "ASPP", "Mlp", "SELayer", "DepthNet"))
    get_mlp_input = W.lift(PATH, "LSSViewTransformerBEVDepth", "get_mlp_input")
    g = torch.Generator().manual_seed(2024)
    net = ns["DepthNet"](16, 16, 16, 8, use_dcn=False).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() > 1:
                fan = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / fan ** 0.5))
            elif "bn" in name.split(".")[-2] or name.split(".")[-2] in ("1", "2"):     # BatchNorm weight / bias
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g) if name.endswith("weight")
                        else 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.5 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    view = LSSViewTransformer(**BEVDET_R50, ops=object())
    s2e, e2g, K, post_rots, post_trans, bda = jittered_rig(view, 3, n_cams=2)
    mlp_input = get_mlp_input(W.Stub(), s2e, e2g, K, post_rots, post_trans, bda)
    with torch.no_grad():
        # the BatchNorm1d of the camera inputs: statistics that fit focal lengths above 1000 next to entries below 1
        v = mlp_input.reshape(-1, 27)
        net.bn.running_mean.copy_(v.mean(0) * (1.0 + 0.05 * torch.randn(27, generator=g)))
        net.bn.running_var.copy_((0.02 * v.abs().mean(0) + 0.05) ** 2)
        x = torch.randn(2, 16, 6, 10, generator=g)
        out = net(x, mlp_input)
        aspp_in = torch.randn(2, 16, 6, 10, generator=g)
        aspp_out = net.depth_conv[3](aspp_in)
    assert out.shape == (2, 8 + 16, 6, 10) and bool(torch.isfinite(out).all())
    res = {"x": x.numpy(), "mlp_input": mlp_input.numpy(), "out": out.numpy(), "aspp_in": aspp_in.numpy(),
           "aspp_out": aspp_out.numpy(), "sensor2ego": s2e.numpy(), "cam2imgs": K.numpy(), "post_rots": post_rots.numpy(),
           "post_trans": post_trans.numpy(), "bda": bda.numpy()}
    keys = []
    for k, t in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        keys.append(PREFIX + k)
        res["sd." + PREFIX + k] = t.numpy()
    res["keys"] = np.array(sorted(keys))
    path = os.path.join(HERE, "bevdepth.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(keys)} tensors")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pinned":
        record()
        raise SystemExit(0)
    from conftest import PINNED_CPU_ENV
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "pinned"], env=dict(os.environ, **PINNED_CPU_ENV))
