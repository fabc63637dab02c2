"""CPU-only: the pre-launch status contract of bevops_dwsep_conv_s8 (csrc/dwsep_conv_s8.hip) in its documented order,
functions.yolox_ops.quantize_dwsep_weights against a float64 statement, the INT8 plan of YOLOX-Nano
(yolox_int8.build_plan: 30 depthwise-separable steps, one site each beside the scale groups; the dense plan unchanged) and
the `depthwise` keyword of quantization.build_int8_yolox."""
import ctypes

import numpy as np
import pytest
import torch

SUCCESS, BAD_PARAM, NOT_SUPPORTED = 0, 2, 3
F16, I8 = 1, 2


def test_status_codes_in_the_documented_order():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    buf = (ctypes.c_char * 16384)()
    p = (ctypes.addressof(buf) + 255) & ~255              # aligned host address: never dereferenced
    res = p + 8192

    def call(x=p, xp=32, sx=0.5, wd=p + 512, sd=p + 1024, bd=p + 2048, st=0.5, wp=p + 3072, sp=p + 4096, sw=1.0, bp=p + 5120,
             r=None, rp=0, sr=1.0, od=I8, o=p + 6144, op=16, so=0.25, B=1, H=4, W=4, Cin=32, Cout=16, s=1, a1=2, a2=2):
        return lib.bevops_dwsep_conv_s8(x, xp, sx, wd, sd, bd, st, wp, sp, sw, bp, r, rp, sr, od, o, op, so, B, H, W, Cin,
                                        Cout, s, a1, a2, None)

    for k in ("x", "wd", "sd", "wp", "o"):
        assert call(**{k: None}) == BAD_PARAM, k
    for k in ("H", "W", "Cin", "Cout", "s"):
        assert call(**{k: 0}) == BAD_PARAM, k
    assert call(B=-1) == BAD_PARAM
    assert call(od=0) == NOT_SUPPORTED and call(od=0, xp=16) == NOT_SUPPORTED and call(od=0, H=0) == BAD_PARAM
    assert call(xp=16) == BAD_PARAM and call(op=0) == BAD_PARAM and call(r=res, rp=0) == BAD_PARAM       # pitch < channels
    assert call(xp=40) == BAD_PARAM and call(op=24) == BAD_PARAM and call(r=res, rp=24) == BAD_PARAM     # pitch % 16
    assert call(od=F16, Cout=8, op=12) == BAD_PARAM and call(od=F16, Cout=8, op=8, B=0) == SUCCESS           # fp16 out: % 8
    for k, v in (("x", p + 8), ("wd", p + 520), ("wp", p + 3080), ("o", p + 6152), ("sd", p + 1028), ("bd", p + 2052),
                 ("sp", p + 4098), ("bp", p + 5122)):
        assert call(**{k: v}) == BAD_PARAM, k
    assert call(r=res + 8, rp=16) == BAD_PARAM and call(sp=p + 4100, bp=p + 5124, B=0) == SUCCESS        # 4-byte operands
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        for k in ("sx", "st", "sw", "so"):
            assert call(**{k: bad}) == BAD_PARAM, (k, bad)
        assert call(r=res, rp=16, sr=bad) == BAD_PARAM and call(B=0, sr=bad) == SUCCESS
        assert call(B=0, od=F16, so=bad) == SUCCESS and call(sx=bad, Cin=48, xp=48) == BAD_PARAM         # before the widths
    assert call(s=3) == NOT_SUPPORTED and call(a1=3) == NOT_SUPPORTED and call(a2=-1) == NOT_SUPPORTED
    assert call(Cin=48, xp=48) == NOT_SUPPORTED and call(Cin=16, xp=16) == NOT_SUPPORTED
    assert call(Cout=24, op=32) == NOT_SUPPORTED and call(Cout=12, op=16, od=F16) == NOT_SUPPORTED
    assert call(B=1 << 20, H=1 << 6, W=1 << 6, xp=32) == NOT_SUPPORTED                                   # 32-bit offsets
    assert call(B=0) == SUCCESS and call(B=0, bd=None, sp=None, bp=None) == SUCCESS
    for cin in (32, 96, 160):
        assert call(B=0, Cin=cin, xp=cin + 16, r=res, rp=48, op=48, s=2) == SUCCESS


def test_quantize_dwsep_weights_against_float64():
    from bevformer_tensorrt_amd.functions import quantize_dwsep_weights
    g = torch.Generator().manual_seed(2)
    C, Co = 24, 40
    wd, bd = torch.randn((C, 1, 3, 3), generator=g), torch.randn((C,), generator=g)
    wp, bp = torch.randn((Co, C, 1, 1), generator=g), torch.randn((Co,), generator=g)
    wd[5] = 0                                             # a real channel of zeros: scale 1 as a pad channel's
    qd, sd, b1, qp, sp, b2 = quantize_dwsep_weights(wd, bd, wp, bp, 32, 64)
    assert qd.shape == (3, 3, 32) and qp.shape == (64, 32) and qd.dtype == qp.dtype == torch.int8
    for q, s, b, w, bias, n in ((qd.permute(2, 0, 1).reshape(32, 9), sd, b1, wd.reshape(C, 9), bd, C),
                                (qp, sp, b2, torch.cat([wp[:, :, 0, 0], torch.zeros(Co, 8)], 1), bp, Co)):
        amax = w.abs().amax(1)
        want_s = np.where(amax.numpy() > 0, (amax / 127.0).numpy(), np.float32(1)).astype(np.float32)
        assert np.array_equal(s[:n].numpy(), want_s) and bool((s[n:] == 1).all()) and s.dtype == torch.float32
        ratio = w.double().numpy() / want_s.astype(np.float64)[:, None]
        want_q = np.clip(np.rint(ratio), -127, 127)
        near_tie = np.abs(np.abs(ratio - np.floor(ratio)) - 0.5) < 1e-5       # the quotient is formed in fp32
        assert np.array_equal(q[:n].numpy()[~near_tie], want_q[~near_tie]) and near_tie.mean() < 0.01
        assert not q[n:].any() and torch.equal(b[:n], bias) and not b[n:].any()
        assert int(q.abs().max()) == 127


def test_plans_keyword_and_the_unquantised_emulation():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd import yolox as Y
    from bevformer_tensorrt_amd import yolox_int8 as YI
    nano = Y.YOLOX(Y.YOLOX_NANO)
    plan = YI.build_plan(nano)
    n_groups = plan.groups()[1]
    sites = YI.plan_sites(plan)
    assert plan.num_dwsep == 30 == sum(isinstance(m, Y.DWSepConvAct) for m in nano.modules())
    assert [s.dw for s in plan.steps if s.op == "dwsep"] == list(range(30))
    assert len(sites) == n_groups + 30 == len(set(sites)) and sites[:n_groups] == [YI.group_site(g) for g in range(n_groups)]
    for l in range(3):                                    # the head's first tower convolutions: two halves of one buffer
        a, r = (next(s for s in plan.steps if s.key is c[l][0]) for c in (nano.bbox_head.cls_convs, nano.bbox_head.reg_convs))
        assert a.dst.buf == r.dst.buf and (a.dst.c0, r.dst.c0) == (0, 64) and a.src.buf == r.src.buf
    dense = YI.build_plan(Y.YOLOX(Y.YOLOX_S))             # the dense plan and its sites are what they were
    assert dense.num_dwsep == 0 and len(dense.bufs) == 62 and sum(s.op == "conv" for s in dense.steps) == 74
    assert YI.plan_sites(dense) == [YI.group_site(g) for g in range(57)]
    with pytest.raises(NotImplementedError, match="use_depthwise"):
        Q.build_int8_yolox(nano, "cpu", iter(()))
    with pytest.raises(ValueError, match="depthwise"):
        Q.build_int8_yolox(nano, "cpu", iter(()), depthwise="fp16")
    with pytest.raises(ValueError, match="30 depthwise-separable layers"):
        YI.Int8YOLOX(nano, [1.0] * n_groups)
    # mode "emulate" without scales on the fp32 weights themselves is the plain model, for the dense plan too: the
    # tolerance of tests/test_yolox_int8_cpu.py
    image = torch.randn((2, 3, 64, 96), generator=torch.Generator().manual_seed(5))
    for fp in (nano, Y.YOLOX(Y.YOLOX_S)):
        fl = YI.float_operands(fp)
        for a, b in zip(YI.split_outputs(YI.run_plan(YI.build_plan(fp), image, "emulate", None, fl), fl["slices"]), fp(image)):
            assert tuple(a.shape) == tuple(b.shape) and float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
