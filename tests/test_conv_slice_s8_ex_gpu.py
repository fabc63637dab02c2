"""bevops_conv_slice_s8_ex (csrc/conv_slice_s8.hip): the identity IN FRONT of the activation (res_first), through the C
ABI in the guarded arena of tests/util_arena.py under both poisons, every byte of the output buffer outside the output
slice compared.

* res_first = 0 is bevops_conv_slice_s8 bit for bit on the lattice cases of tests/test_conv_slice_s8_gpu.py.
* res_first = 1 with ReLU and with none, int8 and fp16 out, layouts dense / slice / inplace, on the cases of
  tests/util_conv_slice_s8_ex.py (3 x 3 at 64 -> 64, 1 x 1 at 96 -> 48; maps 7 x 9 and 12 x 11): tolerance 0 against the
  float64 statement, whose two orders differ on at least 10 % of the outputs with ReLU (asserted on the statement, here
  and in tests/test_deconv_s8_cpu.py): a kernel that ignores the flag cannot pass.
* the Python wrapper's res_first keyword."""
import numpy as np
import pytest
import torch

import test_conv_slice_s8_gpu as T
import util_conv_slice_s8_ex as E
import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20


def c_call_ex(arena, x, w, ws, bias, res, act, stride, layout, out, res_first, scale_a=E.S_A, scale_w=1.0, scale_res=E.S_RES,
              scale_out=1.0):
    """tests/test_conv_slice_s8_gpu.py's c_call on the _ex entry (layouts 'dense', 'slice', 'inplace')."""
    L, h, st = T._lib()
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = X.conv_out_hw(H, W, k, stride)
    odt = torch.int8 if out == "int8" else torch.float16
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    wsd = None if ws is None else arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 4, "w_scales")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 4, "bias")
    xp, xc0 = (Cin, 0) if layout == "dense" else (Cin + 48, 16)
    op, oc0 = (Cout, 0) if layout == "dense" else ((Cout + 32, 16) if out == "int8" else (Cout + 24, 8))
    _, xv = T._place_slice(arena, x, xp, xc0, "x")
    if layout == "inplace":
        assert out == "int8" and res is not None
        obuf, _ = T._place_slice(arena, res, op, oc0, "identity|out")
    else:
        obuf = arena.empty((B, Ho, Wo, op), odt, 16, "out")
    ov = obuf[..., oc0:oc0 + Cout]
    rv, rp = None, 0
    if res is not None:
        if layout == "inplace":
            rv, rp = ov, op
        else:
            rp = (Cout if layout == "dense" else Cout + 16) + 15 & ~15
            _, rv = T._place_slice(arena, res, rp, 0, "identity")
    before = obuf.cpu().numpy().view(np.uint8).copy()
    rc = h.bevops_conv_slice_s8_ex(xv.data_ptr(), xp, scale_a, wd.data_ptr(), None if wsd is None else wsd.data_ptr(),
                                   scale_w, None if bd is None else bd.data_ptr(), None if rv is None else rv.data_ptr(), rp,
                                   scale_res, L.I8 if out == "int8" else L.F16, ov.data_ptr(), op, scale_out, B, H, W, Cin,
                                   Cout, k, stride, act, int(res_first), st)
    assert rc == L.SUCCESS
    arena.check()
    after = obuf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[..., oc0:oc0 + Cout] = True
    mask8 = np.repeat(mask, after.itemsize, axis=-1)
    assert np.array_equal(after.view(np.uint8)[~mask8], before[~mask8]), "bytes of the output buffer outside the slice were written"
    return after[..., oc0:oc0 + Cout].copy()


def run_both_poisons(*args, **kw):
    got = [c_call_ex(Arena(CAPACITY, poison), *args, **kw) for poison in POISONS]
    assert np.array_equal(got[0].view(np.uint8), got[1].view(np.uint8)), "results differ between the two poisons"
    return got[0]


# ---------------------------------------------------------------------------------------------- res_first = 0
@pytest.mark.parametrize("act", [T.NONE, T.RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("case", [c for c in T.CASES if c[7] != "same"], ids=lambda c: "x".join(map(str, c)))
def test_res_first_0_is_conv_slice_s8_bit_for_bit(case, act):
    x, w, ws, bias, res, acc = T.lattice_case(case)
    layout, out = case[7], case[8]
    want, s_out, _ = T.lattice_statement(case, True, act)
    ref = T.c_call(Arena(CAPACITY, POISONS[0]), x, w, ws, bias, res, act, case[6], layout, out, scale_out=s_out)
    got = run_both_poisons(x, w, ws, bias, res, act, case[6], layout, out, 0, scale_out=s_out)
    T._assert_equal(got, ref)
    T._assert_equal(got, want)


# ---------------------------------------------------------------------------------------------- res_first = 1
@pytest.mark.parametrize("layout,out", [("dense", "int8"), ("slice", "int8"), ("inplace", "int8"), ("dense", "fp16"),
                                        ("slice", "fp16")])
@pytest.mark.parametrize("act", [E.NONE, E.RELU], ids=["linear", "relu"])
@pytest.mark.parametrize("case", E.CASES, ids=lambda c: "x".join(map(str, c)))
def test_res_first_1_equals_the_statement(case, act, layout, out):
    x, w, ws, bias, res, acc = E.operands(case)
    front, behind, s_out = E.statements(case, act, out)
    share = E.differing_share(front, behind)
    print(f"{share:.2%} of the outputs differ between the two orders")
    assert share >= 0.10 if act == E.RELU else share == 0.0
    T._assert_equal(E.order_statement(case, act, out, s_out), front)        # the fp32 operation order gives the same bits
    got = run_both_poisons(x, w, ws, bias, res, act, 1, layout, out, 1, scale_out=s_out)
    T._assert_equal(got, front)
    assert front.any() and (out == "fp16" or ((front == 127).any() and (front == 0).any()))


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrapper_keyword_res_first():
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    from bevformer_tensorrt_amd.utils import lib as L
    case = E.CASES[1]
    x, w, ws, bias, res, acc = E.operands(case)
    front, behind, s_out = E.statements(case, E.RELU, "int8")
    dev = torch.device("cuda")
    xd, rd = (torch.from_numpy(a.copy()).to(dev).permute(0, 3, 1, 2) for a in (x, res))
    wd, wsd, bd = (torch.from_numpy(a.copy()).to(dev) for a in (w, ws, bias))
    y1 = Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, bd, "relu", rd, E.S_RES, 1, None, s_out, torch.int8, res_first=True)
    y0 = Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, bd, "relu", rd, E.S_RES, 1, None, s_out, torch.int8)
    T._assert_equal(y1.permute(0, 2, 3, 1).cpu().numpy(), front)
    T._assert_equal(y0.permute(0, 2, 3, 1).cpu().numpy(), behind)
    for kw in (dict(act="silu", residual_q=rd), dict(act="relu", residual_q=None)):
        with pytest.raises(L.BevopsError) as e:
            Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, bd, kw["act"], kw["residual_q"], E.S_RES, 1, None, s_out, torch.int8,
                                res_first=True)
        assert e.value.status == L.NOT_SUPPORTED
