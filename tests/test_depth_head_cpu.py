"""CPU-only: pack_depth_head_tensors against include/bevops.h's indexing, bevops_lss_depth_head_f16's statuses in order,
lss_depth_head_plain against float64 with the measured fp32 softmax term of util_depth_head.py, FLASHOCC_R50_D88."""
import ctypes

import numpy as np
import pytest
import torch

from util_depth_head import CASES, T, operands, statement


@pytest.mark.parametrize("Cin,C,D", [(32, 8, 1), (64, 64, 59), (96, 80, 118)])
def test_pack_places_every_column_and_k(Cin, C, D):
    from bevformer_tensorrt_amd.functions.depth_head import pack_depth_head_tensors
    W = (1 + torch.arange((D + C) * Cin).view(D + C, Cin) % 2039).half()         # non-zero, exact in fp16
    b = (1 + torch.arange(D + C)).float()
    p = pack_depth_head_tensors(W.view(D + C, Cin, 1, 1), b, D, C)
    nt = (C + D + 31) // 32
    assert (p.nt, p.Cin, p.C, p.D) == (nt, Cin, C, D) and tuple(p.w.shape) == (nt, Cin // 16, 64, 8)
    assert p.w.dtype == torch.float16 and p.bias.dtype == torch.float32 and tuple(p.bias.shape) == (32 * nt,)
    t, s, l, e = torch.meshgrid(torch.arange(nt), torch.arange(Cin // 16), torch.arange(64), torch.arange(8), indexing="ij")
    col, k = 32 * t + (l & 31), 16 * s + 8 * (l >> 5) + e
    src = torch.where(col < C, col + D, col - C)                                  # features behind the D depth rows
    want = torch.where(col < C + D, W[src.clamp_max(D + C - 1), k], torch.zeros((), dtype=torch.float16))
    assert torch.equal(p.w, want)
    assert torch.equal(p.bias, torch.cat([b[D:], b[:D], torch.zeros(32 * nt - C - D)]))


def call(lib, **kw):
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    a = dict(x=p, x_pitch=256, w=p, bias=p, depth=p, feat=p, n=0, hw=4, Cin=256, C=64, D=88)
    for k, v in kw.items():
        a[k] = p + v if k in ("x", "w", "bias", "depth", "feat") and isinstance(v, int) else v
    return lib.bevops_lss_depth_head_f16(a["x"], a["x_pitch"], a["w"], a["bias"], a["depth"], a["feat"], a["n"], a["hw"],
                                         a["Cin"], a["C"], a["D"], None)


BAD = [dict(x=None), dict(w=None), dict(bias=None), dict(depth=None), dict(feat=None), dict(n=-1), dict(hw=-1), dict(Cin=0),
       dict(C=0), dict(D=0), dict(x_pitch=248), dict(x_pitch=260), dict(x=8), dict(w=4), dict(bias=4), dict(feat=8),
       dict(depth=1)]
UNSUPPORTED = [dict(Cin=48, x_pitch=48), dict(Cin=544, x_pitch=544), dict(C=4), dict(C=136), dict(C=128, D=129),
               dict(n=1 << 16, hw=1 << 15)]


@pytest.mark.parametrize("kw", BAD, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_bad_param_comes_first(kw):
    from bevformer_tensorrt_amd.utils import load_library
    assert call(load_library(), **kw) == 2
    assert call(load_library(), **dict(kw, D=kw.get("D", 250))) == 2              # in front of NOT_SUPPORTED


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_not_supported_then_the_empty_call(kw):
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    assert call(lib, **kw) == 3 and call(lib) == 0 and call(lib, n=3, hw=0) == 0  # no rows: success without a launch


@pytest.mark.parametrize("case", CASES[:4], ids=lambda c: "x".join(map(str, c)))
def test_plain_statement_and_the_measured_fp32_softmax_term(case):
    """lss_depth_head_plain in float64 is the statement; exp / sum / divide in numpy float32 on the fp32-rounded logits
    stays within T / 4 (relative) of float64 on those same logits (the factor: design/depth_head.md, "Error bound")."""
    from bevformer_tensorrt_amd.functions import lss_depth_head_plain
    (Cin, C, D), (x, W, b) = case, operands(*case, 90)
    f, p, _, _ = statement(x, W, b, D, C)
    depth, feat = lss_depth_head_plain(x.double(), W.view(D + C, Cin, 1, 1), b, D, C, 2, spatial=(5, 9))
    assert tuple(depth.shape) == (2, D, 5, 9) and tuple(feat.shape) == (2, 5, 9, C)
    assert np.abs(depth.permute(0, 2, 3, 1).reshape(90, D).numpy() - p).max() <= 1e-14
    assert np.abs(feat.reshape(90, C).numpy() - f).max() <= 1e-12
    z = (x.double() @ W.double().t() + b.double())[:, :D].numpy().astype(np.float32)
    e32 = np.exp(z - z.max(1, keepdims=True))
    p32 = e32 / e32.sum(1, keepdims=True, dtype=np.float32)
    z64 = z.astype(np.float64)
    e64 = np.exp(z64 - z64.max(1, keepdims=True))
    rel = np.abs(p32 / (e64 / e64.sum(1, keepdims=True)) - 1).max()
    print(f"{case}: fp32 softmax term {rel:.3e}, T = {T:.3e}, logit range {z.min():.2f} .. {z.max():.2f}")
    assert p32.dtype == np.float32 and 4 * rel <= T


def test_the_d88_constant_builds():
    from bevformer_tensorrt_amd.bevdet import BEVDet, FLASHOCC_R50, FLASHOCC_R50_D88
    assert FLASHOCC_R50["grid_config"]["depth"] == [1.0, 60.0, 1.0] and FLASHOCC_R50_D88["occ_head"] == FLASHOCC_R50["occ_head"]
    m = BEVDet(FLASHOCC_R50_D88)
    assert m.view.D == 88 and m.view._depth_head_fused() and m.view.depth_net.out_channels == 88 + 64
