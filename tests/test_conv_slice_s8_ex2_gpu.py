"""bevops_conv_slice_s8_ex2 (csrc/conv_slice_s8.hip): dilation and the per-image bias, through the C ABI in the guarded
arena of tests/util_arena.py under both poisons, every byte of the output buffer outside the output slice compared.

* exact bytes on the power-of-two lattice against the float64 statement of tests/util_conv_slice_s8_ex2.py, int8 and fp16
  out, shared and per-image bias, at the cases listed there (tolerance 0);
* one-hot taps at dilation 2 and 6; the per-image bias alone (zero sums); res_first with dilation; SiLU with general
  scales inside the derived interval of tests/util_conv_slice_s8.py; a NaN bias row spoils its own image only;
  (dilation 1, no image bias) is bevops_conv_slice_s8_ex bit for bit; the Python wrapper's keywords, also under capture."""
import numpy as np
import pytest
import torch

import test_conv_slice_s8_gpu as T
import util_conv_slice_s8 as S
import util_conv_slice_s8_ex2 as E
import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 16 << 20


def run_both_poisons(*args, **kw):
    got = [E.c_call_ex2(Arena(CAPACITY, poison), *args, **kw) for poison in POISONS]
    assert np.array_equal(got[0].view(np.uint8), got[1].view(np.uint8)), "results differ between the two poisons"
    return got[0]


# ---------------------------------------------------------------------------------------------- tolerance 0
@pytest.mark.parametrize("out", ["int8", "fp16"])
@pytest.mark.parametrize("epi", ["bias", "image"])
@pytest.mark.parametrize("case", E.LATTICE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_lattice_bits(case, epi, out):
    x, w, ws, bias, ibias, res, acc = E.operands(case)
    d, layout = case[5], case[6]
    act = E.RELU if epi == "image" else E.NONE            # (ASPP's layers are ReLU layers; the linear form keeps both signs)
    want, s_out, t = E.lattice_statement(case, epi, act, out)
    shared, per_image = (bias, None) if epi == "bias" else (None, ibias)
    T._assert_equal(E.order_statement(acc, E.S_A, ws, shared, per_image, act, None, 1.0, False, s_out, out), want)
    if t is not None:
        ties, beyond = X.int8_shares(t)
        print(f"scale_out 2^{int(np.log2(s_out))}: {ties:.3%} exact ties, {beyond:.3%} beyond +-127")
        assert ties > 0 and beyond > 0
    got = run_both_poisons(x, w, ws, shared, None, act, layout, out, 0, d, per_image, scale_out=s_out)
    T._assert_equal(got, want)
    assert want.any()


def test_the_statement_needs_the_dilation_and_the_image_of_every_row():
    """What a kernel that ignores either value would produce differs from the statement on most outputs."""
    case = E.LATTICE_CASES[1]
    x, w, ws, bias, ibias, res, acc = E.operands(case)
    assert (acc != S.sums(x, w, 3, 1)).mean() > 0.5
    want, _, _ = E.lattice_statement(case, "image", E.NONE, "fp16")
    for b in range(case[0]):
        first = E.order_statement(acc, E.S_A, ws, None, np.broadcast_to(ibias[b], ibias.shape), E.NONE, None, 1.0, False,
                                  1.0, "fp16")
        same = [bool(np.array_equal(first[i], want[i])) for i in range(case[0])]
        assert same == [i == b for i in range(case[0])]


# ---------------------------------------------------------------------------------------------- one-hot taps
@pytest.mark.parametrize("cin", [32, 96])
@pytest.mark.parametrize("d", [2, 6])
def test_one_hot_taps_land_on_their_own_pixel(cin, d):
    """ONE non-zero pixel (1, 6, 6) on a 13 x 13 map and ONE non-zero weight per output channel at its own (ky, kx, ci):
    output channel co is non-zero at exactly pixel (1, 6 - (ky - 1) d, 6 - (kx - 1) d) and nowhere else."""
    B, H, W, Cout = 2, 13, 13, 48
    K = 9 * cin
    must = sorted({0, 15, 16, K - 1, K - 16, K - 17, K - 33} | {t * cin for t in range(9)} | {t * cin + cin - 1 for t in range(9)})
    ks = (must + [v for v in sorted({int(v) for v in np.linspace(0, K - 1, 97)}) if v not in must])[:Cout]
    assert len(ks) == Cout == len(set(ks)) and {kk // cin for kk in ks} == set(range(9))
    w = np.zeros((Cout, K), np.int8)
    for co, kk in enumerate(ks):
        w[co, kk] = 1 + co % 3
    w = w.reshape(Cout, 3, 3, cin)
    x = np.zeros((B, H, W, cin), np.int8)
    x[1, 6, 6] = 1 + np.arange(cin) % 100
    want = np.zeros((B, H, W, Cout), np.int64)
    for co, kk in enumerate(ks):
        tap, ci = divmod(kk, cin)
        want[1, 6 - (tap // 3 - 1) * d, 6 - (tap % 3 - 1) * d, co] = (1 + co % 3) * (1 + ci % 100)
    assert np.array_equal(E.sums_dilated(x, w, d), want) and all(np.count_nonzero(want[..., co]) == 1 for co in range(Cout))
    got = E.c_call_ex2(Arena(CAPACITY, POISONS[0]), x, w, None, None, None, E.NONE, "slice", "fp16", 0, d, None, scale_a=1.0)
    T._assert_equal(got, want.astype(np.float16))


# ---------------------------------------------------------------------------------------------- the per-image bias alone
@pytest.mark.parametrize("out", ["fp16", "int8"])
@pytest.mark.parametrize("shape", [(3, 5, 7, 32, 48, 1), (2, 16, 44, 64, 144, 3)], ids=lambda s: "x".join(map(str, s)))
def test_exactly_one_row_of_the_bias_table_reaches_each_output_row(shape, out):
    """Zero weights: the output IS the bias.  Entry (b, co) = b * 40 + co % 37 - 18 identifies its image and (modulo 37)
    its channel; the pad columns of the table hold the arena's poison."""
    B, H, W, Cin, Cout, k = shape
    x = X.gen_int8(X._rng("ex2 image bias", shape), (B, H, W, Cin))
    w = np.zeros((Cout, k, k, Cin), np.int8)
    table = (np.arange(B)[:, None] * 40 + np.arange(Cout)[None, :] % 37 - 18).astype(np.float16)
    assert np.abs(table).max() <= 127 and len(np.unique(table[:, :37])) == B * 37
    got = run_both_poisons(x, w, None, None, None, E.NONE, "slice", out, 0, 1, table, scale_a=1.0, scale_out=1.0)
    want = np.broadcast_to(table[:, None, None, :], (B, H, W, Cout))
    T._assert_equal(got, want.astype(np.int8 if out == "int8" else np.float16))


# ---------------------------------------------------------------------------------------------- res_first with dilation
@pytest.mark.parametrize("out", ["int8", "fp16"])
def test_res_first_with_dilation(out):
    case = (2, 12, 11, 64, 64, 2, "slice")
    x, w, ws, bias, ibias, res, acc = E.operands(case)
    front, s_out, _ = E.lattice_statement(case, "bias", E.RELU, out, res_first=True, with_res=True)
    behind, _, _ = E.lattice_statement(case, "bias", E.RELU, out, res_first=False, with_res=True)
    assert (T._bits(front) != T._bits(behind)).mean() >= 0.10          # a kernel that ignores the flag cannot pass
    T._assert_equal(E.order_statement(acc, E.S_A, ws, bias, None, E.RELU, res, E.S_RES, True, s_out, out), front)
    got = run_both_poisons(x, w, ws, bias, res, E.RELU, "slice", out, 1, 2, None, scale_out=s_out)
    T._assert_equal(got, front)


# ---------------------------------------------------------------------------------------------- SiLU, general scales
# (B, H, W, Cin, Cout, dilation, layout)
GENERAL_CASES = ((3, 5, 7, 96, 48, 2, "slice"), (2, 16, 44, 64, 144, 6, "slice4"))


def general_case(case):
    B, H, W, Cin, Cout, d, _ = case
    r = X._rng("conv_slice_s8_ex2 general", case)
    x = np.clip(np.rint(r.normal(0, 40, (B, H, W, Cin))), -127, 127).astype(np.int8)
    w = np.clip(np.rint(r.normal(0, 40, (Cout, 3, 3, Cin))), -127, 127).astype(np.int8)
    scale_a, scale_res = np.float32(0.0371), np.float32(0.0433)
    ws = (r.uniform(0.5, 2.0, Cout) * 3.0 / (40.0 * 40.0 * np.sqrt(9 * Cin) * float(scale_a))).astype(np.float32)
    ibias = r.normal(0, 1, (B, Cout)).astype(np.float16)
    res = np.clip(np.rint(r.normal(0, 40, (B, H, W, Cout))), -127, 127).astype(np.int8)
    return x, w, ws, ibias, res, E.sums_dilated(x, w, d), scale_a, scale_res


@pytest.mark.parametrize("identity", [False, True], ids=["plain", "identity"])
@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_general_scales_within_the_derived_interval(case, identity):
    """SiLU, general scales, dilation and the per-image bias: the interval of tests/util_conv_slice_s8.py's
    silu_interval (the bias enters it as an exact fp32 number, which an fp16 value is).  Every output is checked."""
    x, w, ws, ibias, res, acc, scale_a, scale_res = general_case(case)
    r = res if identity else None
    b = ibias.astype(np.float32)[:, None, None, :]
    t0, _, _, _ = S.silu_interval(acc, scale_a, 1.0, ws, b, r, scale_res, 1.0)
    scale_out = np.float32(t0.std() / 47.3)
    t, delta, lo, hi = S.silu_interval(acc, scale_a, 1.0, ws, b, r, scale_res, scale_out)
    assert t.shape == acc.shape and (np.abs(t) > 127.5).any() and delta.max() < 0.01
    runs = [run_both_poisons(x, w, ws, None, r, E.SILU, case[6], "int8", 0, case[5], ibias, scale_a=float(scale_a),
                             scale_res=float(scale_res), scale_out=float(scale_out)) for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    share = S.check_interval(runs[0], lo, hi)
    print(f"delta max {delta.max():.2e} steps; {share:.4%} of the outputs within delta of a half-integer")


# ---------------------------------------------------------------------------------------------- non-finite containment
@pytest.mark.parametrize("out", ["int8", "fp16"])
def test_a_nan_bias_row_spoils_its_own_image_only(out):
    case = GENERAL_CASES[0]
    x, w, ws, ibias, res, acc, scale_a, scale_res = general_case(case)
    args = dict(scale_a=float(scale_a), scale_res=float(scale_res), scale_out=0.11)
    clean = E.c_call_ex2(Arena(CAPACITY, POISONS[0]), x, w, ws, None, res, E.NONE, "slice", out, 0, case[5], ibias, **args)
    bad = ibias.copy()
    bad[1] = np.nan
    got = E.c_call_ex2(Arena(CAPACITY, POISONS[0]), x, w, ws, None, res, E.NONE, "slice", out, 0, case[5], bad, **args)
    assert np.array_equal(T._bits(got[[0, 2]]), T._bits(clean[[0, 2]]))
    assert (got[1] == -127).all() if out == "int8" else np.isnan(got[1]).all()


# ---------------------------------------------------------------------------------------------- (1, NULL, 0) is _ex
@pytest.mark.parametrize("which", ["identity+relu", "fp16", "silu"])
def test_dilation_1_without_image_bias_is_conv_slice_s8_ex_bit_for_bit(which):
    if which == "silu":
        x, w, ws, bias, res, acc, scale_a, scale_res = T.silu_case(T.SILU_CASES[0])
        args = dict(act=E.SILU, out="int8", scale_a=float(scale_a), scale_res=float(scale_res), scale_out=0.11)
    else:
        case = T.CASES[9] if which == "identity+relu" else T.CASES[6]
        x, w, ws, bias, res, acc = T.lattice_case(case)
        _, s_out, _ = T.lattice_statement(case, True, T.RELU)
        args = dict(act=E.RELU, out=case[8], scale_out=s_out)
    act, out = args.pop("act"), args.pop("out")
    got = {e: E.c_call_ex2(Arena(CAPACITY, POISONS[1]), x, w, ws, bias, res, act, "slice", out, 0, 1, None, entry=e, **args)
           for e in ("ex", "ex2")}
    T._assert_equal(got["ex2"], got["ex"])
    assert got["ex"].any()


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrapper_keywords_eager_and_under_capture():
    """conv_slice_q_taps(dilation=, image_bias=) gives the statement's bits, eagerly and from a captured graph (the
    wrapper allocates nothing when `out` is given and synchronises nowhere); what the entry refuses raises."""
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    from bevformer_tensorrt_amd.utils import lib as L
    case = E.LATTICE_CASES[1]
    x, w, ws, bias, ibias, res, acc = E.operands(case)
    want, s_out, _ = E.lattice_statement(case, "image", E.RELU, "int8")
    dev = torch.device("cuda")
    xd = torch.from_numpy(x.copy()).to(dev).permute(0, 3, 1, 2)
    wd, wsd, bd, ibd = (torch.from_numpy(a.copy()).to(dev) for a in (w, ws, bias, ibias))
    y = Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, None, "relu", None, 1.0, 1, None, s_out, torch.int8, dilation=case[5],
                            image_bias=ibd)
    T._assert_equal(y.permute(0, 2, 3, 1).cpu().numpy(), want)
    out = torch.zeros_like(y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, None, "relu", None, 1.0, 1, out, s_out, torch.int8, dilation=case[5],
                                image_bias=ibd)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    T._assert_equal(out.permute(0, 2, 3, 1).cpu().numpy(), want)
    with pytest.raises(ValueError):
        Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, bd, "relu", image_bias=ibd, scale_out=s_out)
    with pytest.raises(ValueError):
        Y.conv_slice_q_taps(xd, E.S_A, wd, wsd, None, "relu", dilation=0, scale_out=s_out)
    with pytest.raises(L.BevopsError) as e:
        Y.conv_slice_q_taps(xd, E.S_A, wd[:, 1:2, 1:2].contiguous(), wsd, None, "relu", dilation=2, scale_out=s_out)
    assert e.value.status == L.NOT_SUPPORTED
