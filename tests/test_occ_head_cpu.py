"""CPU-only: the statuses of bevops_occ_head_f16 in their documented order, pack_occ_head_tensors against float64 indexing,
functions.occ_head_plain against a hand-written loop, and the premises of tests/test_occ_head_gpu.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

from util_occ_head import (EXACT_CASES, GENERAL_CASES, SOFTPLUS_ERR, exact_operands, general_operands, plain64,
                           softplus_f32)

LL = ctypes.c_longlong


def call(lib, **kw):
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15
    a = dict(y=p, y_pitch=256, w1=p, b1=p, w2=p, b2=p, occ=p, s_img=0, s_line=0, s_px=16, logits=None, B=0, H=1, W=1,
             C=256, Hd=512, Dz=16, Ncls=18)
    for k, v in kw.items():
        a[k] = p + v if k in ("y", "w1", "b1", "w2", "b2", "occ", "logits") and isinstance(v, int) else v
    return lib.bevops_occ_head_f16(a["y"], a["y_pitch"], a["w1"], a["b1"], a["w2"], a["b2"], a["occ"], LL(a["s_img"]),
                                   LL(a["s_line"]), LL(a["s_px"]), a["logits"], a["B"], a["H"], a["W"], a["C"], a["Hd"],
                                   a["Dz"], a["Ncls"], None)


BAD = [dict(y=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(occ=None), dict(B=-1), dict(H=0),
       dict(W=0), dict(C=0), dict(Hd=0), dict(Dz=0), dict(Ncls=0), dict(y_pitch=248), dict(y_pitch=260), dict(s_px=15),
       dict(s_line=-1), dict(y=8), dict(w1=2), dict(b1=8), dict(w2=4), dict(b2=8), dict(logits=1)]
UNSUPPORTED = [dict(C=48, y_pitch=48), dict(C=288, y_pitch=288), dict(Hd=96), dict(Hd=1088), dict(Dz=17, s_px=17),
               dict(Ncls=33), dict(Dz=16, Ncls=21), dict(H=1 << 16, W=1 << 16)]


@pytest.mark.parametrize("kw", BAD, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_bad_param_comes_first(kw):
    from bevformer_tensorrt_amd.utils import load_library
    assert call(load_library(), **kw) == 2
    assert call(load_library(), **dict(kw, Hd=96 if "Hd" not in kw else kw["Hd"])) == 2      # in front of NOT_SUPPORTED


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_not_supported_then_the_empty_call(kw):
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    assert call(lib, **kw) == 3 and call(lib) == 0                      # B == 0: success without a launch
    assert lib.bevops_occ_head_blocks(16, 18) == 9 and lib.bevops_occ_head_blocks(11, 29) == 11
    assert lib.bevops_occ_head_blocks(16, 21) == 0 and lib.bevops_occ_head_blocks(1, 2) == 1


@pytest.mark.parametrize("Dz,Ncls", [(1, 2), (3, 18), (16, 18), (11, 29), (15, 21), (16, 20)])
def test_pack_round_trip(Dz, Ncls):
    """Every (z, cls, hidden unit) is found where include/bevops.h says, every other packed element is zero."""
    from bevformer_tensorrt_amd.functions import occ_head as Fn
    Hd, C, N = 128, 32, Dz * Ncls
    W2 = (1 + torch.arange(N * Hd).view(N, Hd) % 2039).half()            # non-zero, exact in fp16
    b2 = (1 + torch.arange(N)).half()
    p = Fn.pack_occ_head_tensors(torch.zeros(Hd, C), torch.zeros(Hd), W2, b2, Dz, Ncls)
    nb = Fn.occ_head_blocks(Dz, Ncls)
    assert nb == math.ceil(math.ceil(Dz / 2) * Ncls / 16) and tuple(p.w2.shape) == (Hd // 64, 32 * nb, 64)
    seen = torch.zeros_like(p.w2, dtype=torch.bool)
    for z in range(Dz):
        for cls in range(Ncls):
            t, hb = (z // 2) * Ncls + cls, z % 2
            P = 32 * (t // 16) + 8 * (t % 16 // 4) + 4 * hb + t % 4
            assert float(p.b2[P]) == float(b2[z * Ncls + cls])
            for u in range(Hd):
                s, r = divmod(u, 64)
                i, pp, q, h, c = r // 32, r // 16 % 2, r // 8 % 2, r // 4 % 2, r % 4
                j = 32 * i + 16 * pp + 8 * h + 4 * q + c
                assert float(p.w2[s, P, j]) == float(W2[z * Ncls + cls, u])
                seen[s, P, j] = True
    assert int(seen.sum()) == N * Hd and float(p.w2[~seen].abs().sum()) == 0 and int((p.b2 != 0).sum()) == N


def test_plain_statement_by_hand():
    """occ_head_plain on a [2, 4, 2, 3] map against a scalar loop: softplus, class-fastest columns, ties to the lowest
    class; occ[b, h, w] follows the input's own axes (the model permutes)."""
    from bevformer_tensorrt_amd.functions import occ_head_plain
    g = torch.Generator().manual_seed(5)
    B, C, H, W, Hd, Dz, Ncls = 2, 4, 2, 3, 5, 2, 3
    y, W1, b1 = torch.randn(B, C, H, W, generator=g).double(), torch.randn(Hd, C, generator=g).double(), torch.randn(Hd).double()
    W2, b2 = torch.randn(Dz * Ncls, Hd, generator=g).double(), torch.randn(Dz * Ncls, generator=g).double()
    W2[4], b2[4] = W2[3], b2[3]                                      # voxel 1: classes 0 and 1 always tie
    W2[5], b2[5] = W2[3], b2[3] - 1.0
    occ, lg = occ_head_plain(y, W1, b1, W2, b2, Dz, Ncls, logits=True)
    assert occ.dtype == torch.uint8 and tuple(occ.shape) == (B, H, W, Dz) and tuple(lg.shape) == (B, H, W, Dz * Ncls)
    for b in range(B):
        for h in range(H):
            for w in range(W):
                hid = [math.log1p(math.exp(sum(float(W1[j, c] * y[b, c, h, w]) for c in range(C)) + float(b1[j])))
                       for j in range(Hd)]
                logit = [sum(float(W2[n, j]) * hid[j] for j in range(Hd)) + float(b2[n]) for n in range(Dz * Ncls)]
                assert np.allclose(lg[b, h, w].numpy(), logit, rtol=1e-12, atol=1e-12)
                assert int(occ[b, h, w, 0]) == int(np.argmax(logit[:3])) and int(occ[b, h, w, 1]) == 0
    big = torch.full((1, C, 1, 1), 50.0).double()                     # above the threshold: v itself
    assert float(occ_head_plain(big, torch.ones(Hd, C).double(), b1 * 0, W2, b2, Dz, Ncls, logits=True)[1][0, 0, 0, 0]) == \
        float((W2[0] * 200.0).sum() + b2[0])


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_chain_premises(case):
    ops, (occ, lg, v, h) = exact_operands(*case)
    assert torch.equal(v, v.round()) and float(v.min()) > 20 and float(v.max()) <= 2048 and torch.equal(h, v)
    assert torch.equal(lg, lg.round()) and float(lg.abs().max()) < 2048
    vox = lg.view(-1, *case[2:])
    tied = ((vox == vox.amax(-1, keepdim=True)).sum(-1) > 1).float().mean()
    assert float(tied) >= 0.25, f"ties in {float(tied):.2f} of the voxels"
    o, l = plain64(*ops, *case[2:])
    assert torch.equal(o.long(), occ) and torch.equal(l, lg)
    assert len(occ.unique()) > 1 or case[3] == 2


@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_general_premises(case):
    ops, (occ, lg, v, h), eps, sure = general_operands(*case)
    assert float((v < -1).float().mean()) > 0.1 and float((v > 1).float().mean()) > 0.1 and float(v.max()) < 20     # the knee
    for rows in (129, 300):
        left = 1.0 - float(sure[:rows].float().mean())
        print(f"{case} rows {rows}: left out {left:.4f}, median eps {float(eps.median()):.3e}")
        assert left <= 0.10
    # the float32 statement on the CPU (the kernel's Softplus formula, one fp16 rounding of h) lies inside half the bound
    y, W1, b1, W2, b2 = (t.float() for t in ops)
    h32 = torch.from_numpy(softplus_f32((y @ W1.t() + b1).numpy())).half().float()
    assert bool((((h32 @ W2.t() + b2).half().double() - lg).abs() <= 0.5 * eps).all())


def test_softplus_term_is_measured():
    v = np.linspace(-40.0, 20.0, 600001)
    ref = np.log1p(np.exp(v.astype(np.float32).astype(np.float64)))
    err = np.abs(softplus_f32(v).astype(np.float64) - ref) / np.maximum(1.0, ref)
    print(f"softplus fp32 formula: max err / max(1, softplus) = {err.max():.3e}; the bound uses {SOFTPLUS_ERR:.3e}")
    assert err.max() <= SOFTPLUS_ERR / 4
    assert softplus_f32(np.float32(20.5)) == np.float32(20.5) and softplus_f32(np.float32(2047.0)) == np.float32(2047.0)


def test_checkpoint_keys_fill_the_head():
    """occ_head_key_map names exactly the head's parameters, and load_reference_state_dict fills them from those keys."""
    from bevformer_tensorrt_amd.bevdet import BEVDet, FLASHOCC_R50
    from bevformer_tensorrt_amd.checkpoint import load_reference_state_dict, occ_head_key_map
    m = BEVDet(dict(FLASHOCC_R50, occ_head=dict(Dz=2, num_classes=3, hidden=64)))
    kmap = occ_head_key_map(m)
    own = {n: p for n, p in m.named_parameters() if n.startswith(("final_conv.", "predicter."))}
    assert sorted(kmap) == sorted(own) and len(own) == 6 and occ_head_key_map(object()) == {}
    assert set(kmap.values()) == {f"occ_head.{k}.{n}" for k in ("final_conv.conv", "predicter.0", "predicter.2")
                                  for n in ("weight", "bias")}
    sd = {src: torch.full_like(own[n], 1.0 + i) for i, (n, src) in enumerate(sorted(kmap.items()))}
    missing, unexpected = load_reference_state_dict(m, sd, strict=False, key_map=kmap)
    assert not unexpected and not any(n in own for n in missing)
    assert all(float(own[n].mean()) == 1.0 + i for i, n in enumerate(sorted(kmap)))
