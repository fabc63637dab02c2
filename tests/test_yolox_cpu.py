"""CPU-only: yolox.py's architecture against the numbers of the reference's config, the BN fold at eps 1e-3, mmdet's
YOLOX key map (checkpoint.py), the block-diagonal predictor merge and the plain path's output shapes."""
import pytest
import torch
import torch.nn as nn

from bevformer_tensorrt_amd import checkpoint as C
from bevformer_tensorrt_amd import yolox as Y


@pytest.fixture(scope="module")
def small():
    return Y.YOLOX(Y.YOLOX_S)


def test_yolox_x_block_counts_and_widths():
    m = Y.YOLOX(Y.YOLOX_X)
    bb = m.backbone
    assert bb.stem.conv.in_channels == 12 and bb.stem.conv.out_channels == 80
    assert [s[0].out_channels for s in bb.stages] == [160, 320, 640, 1280]
    assert [s[0].in_channels for s in bb.stages] == [80, 160, 320, 640]
    assert all(s[0].stride == (2, 2) and s[0].kernel_size == (3, 3) for s in bb.stages)
    assert [len(s[-1].blocks) for s in bb.stages] == [4, 12, 12, 4]
    assert [s[-1].mid for s in bb.stages] == [80, 160, 320, 640]
    assert [all(b.add_identity for b in s[-1].blocks) for s in bb.stages] == [True, True, True, False]
    assert [len(s) for s in bb.stages] == [2, 2, 2, 3] and isinstance(bb.stages[3][1], Y.SPPBottleneck)
    assert bb.stages[3][1].kernel_sizes == (5, 9, 13) and bb.stages[3][1].conv2.in_channels == 4 * 640
    n = m.neck
    assert [c.in_channels for c in n.reduce_layers] == [1280, 640] and [c.out_channels for c in n.reduce_layers] == [640, 320]
    assert [len(b.blocks) for b in list(n.top_down_blocks) + list(n.bottom_up_blocks)] == [4] * 4
    assert not any(b.add_identity for l in list(n.top_down_blocks) + list(n.bottom_up_blocks) for b in l.blocks)
    assert [c.out_channels for c in n.out_convs] == [320] * 3 and all(d.stride == (2, 2) for d in n.downsamples)
    h = m.bbox_head
    assert [c.out_channels for c in h.conv_cls] == [80] * 3 and h.conv_reg[0].out_channels == 4 and h.conv_obj[0].out_channels == 1
    assert all(len(t) == 2 and t[0].out_channels == 320 and t[0].kernel_size == (3, 3) for t in h.cls_convs)
    assert Y.YOLOX_X["test_cfg"] == dict(score_thr=0.01, nms=dict(iou_threshold=0.65)) and Y.YOLOX_X["strides"] == (8, 16, 32)
    # the launch list of one fast forward (design/yolox.md): a CSP layer of n blocks is 3 + 2 n convolutions
    csp = [s[-1] for s in bb.stages] + list(n.top_down_blocks) + list(n.bottom_up_blocks)
    convs = sum(1 for mod in m.modules() if isinstance(mod, nn.Conv2d))
    assert convs == 1 + 4 + 2 + sum(3 + 2 * len(c.blocks) for c in csp) + 2 + 2 + 3 + 3 * 7 == 155


def test_plain_path_output_shapes(small):
    outs = small(torch.randn((1, 3, 64, 64), generator=torch.Generator().manual_seed(1)))
    assert [tuple(o.shape) for o in outs] == [(1, 80, 8, 8), (1, 80, 4, 4), (1, 80, 2, 2), (1, 4, 8, 8), (1, 4, 4, 4),
                                              (1, 4, 2, 2), (1, 1, 8, 8), (1, 1, 4, 4), (1, 1, 2, 2)]
    assert all(torch.isfinite(o).all() and o.std() > 1e-2 for o in outs)
    with pytest.raises(ValueError):
        small(torch.zeros((1, 3, 60, 64)))
    with pytest.raises(ValueError, match="16 384|16384"):
        Y.YOLOXRunner(small, 1, 1280, 1280)


def test_bn_fold_eps_1e3_equals_the_unfolded_module():
    g = torch.Generator().manual_seed(2)
    conv = nn.Conv2d(6, 10, 3, 2, 1, bias=False).double()
    bn = nn.BatchNorm2d(10, eps=1e-3, momentum=0.03).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64))
        bn.weight.copy_(torch.rand(10, generator=g, dtype=torch.float64) + 0.5)
        bn.bias.copy_(torch.randn(10, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(10, generator=g, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(10, generator=g, dtype=torch.float64) * 1e-2)      # small: eps matters
        x = torch.randn((2, 6, 9, 7), generator=g, dtype=torch.float64)
        want = bn(conv(x))
        w, b = C.fold_conv_bn(conv.weight, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, eps=C.YOLOX_BN_EPS)
        got = torch.nn.functional.conv2d(x, w, b, 2, 1)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
        w5, b5 = C.fold_conv_bn(conv.weight, None, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        assert not torch.allclose(torch.nn.functional.conv2d(x, w5, b5, 2, 1), want, rtol=1e-3, atol=1e-3)
    assert C.YOLOX_BN_EPS == Y.BN_EPS == 1e-3


def test_key_map_names_every_parameter_once_and_loads(small):
    kmap = C.yolox_key_map(small)
    own = dict(small.named_parameters())
    assert set(kmap) == set(own)
    folded = {v for v in kmap.values() if isinstance(v, tuple)}
    copied = [v for v in kmap.values() if not isinstance(v, tuple)]
    assert len(copied) == len(set(copied)) == 2 * 3 * 3                          # the nine predictors' weights and biases
    assert 2 * len(folded) == len(kmap) - len(copied)                            # a folded layer: one source, weight + bias
    assert all(tag == "conv_bn_yolox" for tag, _, _ in folded)
    assert ("conv_bn_yolox", "backbone.stage4.2.blocks.0.conv1.conv", "backbone.stage4.2.blocks.0.conv1.bn") in folded
    assert kmap["bbox_head.conv_obj.2.bias"] == "bbox_head.multi_level_conv_obj.2.bias"
    # a synthetic mmdet state dict: conv without bias + BN per ConvModule, plain predictors
    g = torch.Generator().manual_seed(3)
    sd = {}
    for name, src in kmap.items():
        if isinstance(src, tuple) and name.endswith(".weight"):
            _, conv, bn = src
            co = own[name].shape[0]
            sd[conv + ".weight"] = torch.randn(own[name].shape, generator=g)
            sd[bn + ".weight"], sd[bn + ".bias"] = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
            sd[bn + ".running_mean"], sd[bn + ".running_var"] = torch.randn(co, generator=g), torch.rand(co, generator=g) * 1e-2
            sd[bn + ".num_batches_tracked"] = torch.tensor(1)
        elif not isinstance(src, tuple):
            sd[src] = torch.randn(own[name].shape, generator=g)
    m = Y.YOLOX(Y.YOLOX_S, seed=1)
    missing, unexpected = C.load_yolox_state_dict(m, sd)
    assert not missing and not unexpected
    conv, bn = "neck.out_convs.1.conv", "neck.out_convs.1.bn"
    w, b = C.fold_conv_bn(sd[conv + ".weight"], None, sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"],
                          sd[bn + ".running_var"], eps=1e-3)
    assert torch.equal(m.neck.out_convs[1].weight, w.float()) and torch.equal(m.neck.out_convs[1].bias, b.float())
    assert torch.equal(m.bbox_head.conv_reg[0].weight, sd["bbox_head.multi_level_conv_reg.0.weight"])
    with pytest.raises(KeyError):
        C.load_yolox_state_dict(m, {k: v for k, v in sd.items() if k != conv + ".weight"})


def test_block_diagonal_predictor_merge():
    g = torch.Generator().manual_seed(4)
    feat = 32
    cls = (torch.randn((80, feat, 1, 1), generator=g), torch.randn(80, generator=g))
    reg = (torch.randn((4, feat, 1, 1), generator=g), torch.randn(4, generator=g))
    obj = (torch.randn((1, feat, 1, 1), generator=g), None)
    w, b, slices = Y.merge_yolox_predictors(cls, reg, obj)
    assert w.shape == (88, 2 * feat, 1, 1) and b.shape == (88,) and slices == [(0, 80), (80, 84), (84, 85)]
    assert torch.equal(w[:80, :feat], cls[0]) and not w[:80, feat:].any()
    assert torch.equal(w[80:84, feat:], reg[0]) and torch.equal(w[84:85, feat:], obj[0]) and not w[80:85, :feat].any()
    assert not w[85:].any() and not b[84:].any() and torch.equal(b[:80], cls[1]) and torch.equal(b[80:84], reg[1])
    cf, rf = torch.randn((2, feat, 3, 5), generator=g).double(), torch.randn((2, feat, 3, 5), generator=g).double()
    packed = torch.nn.functional.conv2d(torch.cat([cf, rf], 1), w.double(), b.double())
    for (a, e), (wi, bi), x in zip(slices, (cls, reg, obj), (cf, rf, rf)):
        want = torch.nn.functional.conv2d(x, wi.double(), None if bi is None else bi.double())
        assert torch.allclose(packed[:, a:e], want, rtol=1e-12, atol=1e-12)
    assert not packed[:, 85:].any()
    with pytest.raises(ValueError):
        Y.merge_yolox_predictors(cls, (torch.zeros((4, feat + 1, 1, 1)), None), obj)
