"""The float64 DCNv2 reference of util_dcn.py (CPU): it agrees with the C oracle and with the library's plain
convolution, and the lattice inputs satisfy the premise the GPU tests' bit-exact expectations rest on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import util_dcn as U
from test_mdconv_gpu import CASES, make

# the seven shapes of test_mdconv_gpu.CASES; the three large ones cut down in H x W (same channels, groups and deform
# groups) so that each takes seconds on the CPU
SMALL = {"ref_test_like": dict(H=10, W=11), "r101_stage3": dict(H=9, W=13), "r101_stage4": dict(H=7, W=10)}


def _oracle(oracle_mod, x, off, mask, w, b, stride, pad, dil, g, dg):
    return oracle_mod.mdconv(x.numpy(), off.numpy(), mask.numpy(), w.numpy(), None if b is None else b.numpy(),
                             (stride,) * 2, (pad,) * 2, (dil,) * 2, g, dg)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("with_bias", [True, False])
def test_dcn_ref_matches_the_c_oracle(oracle_mod, name, with_bias):
    """Two independent statements of DCNv2 (float64 torch from the definition, fp32 C): 1e-5 of the output scale."""
    c = dict(CASES[name], **SMALL.get(name, {}))
    x, off, mask, w, b = make(**c, off_std=2.0)
    b = b if with_bias else None
    K = c["K"]
    got = U.dcn_ref(x, off, mask, w, b, c["stride"], c["pad"], c["dil"], c["g"], c["dg"]).numpy()
    want = _oracle(oracle_mod, x, off, mask, w, b, c["stride"], c["pad"], c["dil"], c["g"], c["dg"])
    assert got.shape == want.shape and K in (1, 3)
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= 1e-5 * scale, (err, scale)


def _lattice_cases():
    for (cin, cout) in U.LATTICE_CHANNELS:
        for geom in U.LATTICE_GEOM:
            yield cin, cout, geom, 1, 1
    yield 128, 8, (1, 1, 1), 2, 2
    yield 6, 10, (1, 1, 1), 1, 3


LATTICE_IDS = [f"cin{c}-cout{o}-s{g[0]}p{g[1]}d{g[2]}-g{gr}dg{dg}" for c, o, g, gr, dg in _lattice_cases()]


@pytest.mark.parametrize("cin,cout,geom,groups,dg", list(_lattice_cases()), ids=LATTICE_IDS)
def test_dcn_ref_matches_the_c_oracle_on_the_lattice(oracle_mod, cin, cout, geom, groups, dg):
    """Taps exactly on -1, 0, H - 1, H (and far outside): the oracle and dcn_ref draw the image rim alike."""
    s, p, d = geom
    lat = U.lattice(U.LATTICE_B, cin, cout, U.LATTICE_H, U.LATTICE_W, s, p, d, groups, dg)
    got = U.dcn_ref(lat["x"], lat["offset"], lat["mask"], lat["weight"], lat["bias"], s, p, d, groups, dg).numpy()
    want = _oracle(oracle_mod, lat["x"], lat["offset"], lat["mask"], lat["weight"], lat["bias"], s, p, d, groups, dg)
    scale = max(1.0, float(np.abs(want).max()))
    assert float(np.abs(got - want).max()) <= 1e-5 * scale
    if dg == 1:     # the channels-last operand unpacks to the same offsets and to masks {0, 1/2, 1} up to 1e-8
        off, m = U.unpack_offset_mask(lat["om32"].half())
        assert torch.equal(off, lat["offset"].double())
        assert torch.equal(U.unpack_offset_mask(lat["om28"].half())[0], off)
        assert (torch.minimum((m - 0.5).abs(), torch.minimum(m, 1 - m)) < 1e-8).all()
        for v in (0.0, 0.5, 1.0):
            assert ((m - v).abs() < 1e-8).any()


@pytest.mark.parametrize("cfg", [dict(Cin=8, Cout=6, g=1, stride=1, pad=1, dil=1), dict(Cin=8, Cout=6, g=2, stride=2, pad=1, dil=1),
                                 dict(Cin=12, Cout=8, g=4, stride=1, pad=2, dil=2), dict(Cin=4, Cout=4, g=1, stride=2, pad=2, dil=2)])
def test_dcn_ref_with_zero_offsets_is_conv2d(cfg):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, cfg["Cin"], 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(cfg["Cout"], cfg["Cin"] // cfg["g"], 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cfg["Cout"], generator=g, dtype=torch.float64)
    Ho, Wo = (U.out_size(n, cfg["stride"], cfg["pad"], cfg["dil"]) for n in (9, 11))
    for dg in (1, 2):
        off = torch.zeros(2, dg * 18, Ho, Wo)
        mask = torch.ones(2, dg * 9, Ho, Wo)
        for relu in (False, True):
            got = U.dcn_ref(x, off, mask, w, b, cfg["stride"], cfg["pad"], cfg["dil"], cfg["g"], dg, relu=relu)
            want = F.conv2d(x, w, b, cfg["stride"], cfg["pad"], cfg["dil"], cfg["g"])
            want = torch.relu(want) if relu else want
            assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("cin,cout,geom,groups,dg", list(_lattice_cases()), ids=LATTICE_IDS)
def test_lattice_inputs_make_a_correct_kernel_exact(cin, cout, geom, groups, dg):
    """The premise of every torch.equal in test_mdconv_nhwc_gpu.py, shown on the inputs and the float64 reference
    alone: every tap class pair occurs, every column element is an fp16 number, every output before its final
    rounding is a multiple of 2^-10 below 2^14 -- so fp16 blends and fp32 sums of a correct kernel round nowhere."""
    s, p, d = geom
    lat = U.lattice(U.LATTICE_B, cin, cout, U.LATTICE_H, U.LATTICE_W, s, p, d, groups, dg)
    pairs = set(zip(lat["cls_h"].flatten().tolist(), lat["cls_w"].flatten().tolist()))
    assert {(a, b) for a in range(11) for b in range(11)} <= pairs
    assert any(a == -1 for a, _ in pairs) and any(b == -1 for _, b in pairs)
    for far in U.FAR:
        assert (lat["offset"] == far).any()
    assert set(lat["mask"].unique().tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    assert lat["x"].abs().max() <= 4 and lat["weight"].abs().max() <= 1
    variants = [(lat["offset"], lat["mask"])]
    if dg == 1:
        assert (lat["om32"][:, 27:] != 0).all() and (lat["om28"][:, 27:] != 0).all()
        off, m = U.unpack_offset_mask(lat["om32"].half())
        m16 = m.half().double()                              # the sigmoid rounded to fp16: what the kernel multiplies by
        assert set(m16.unique().tolist()) == {0.0, 0.5, 1.0}
        variants.append((off, m16))
    for off, mask in variants:
        for bias in (lat["bias"], None):
            out, col = U.dcn_ref(lat["x"], off, mask, lat["weight"], bias, s, p, d, groups, dg, return_col=True)
            assert torch.equal(col.half().double(), col)
            assert torch.equal(col * 128, torch.round(col * 128)) and col.abs().max() <= 4
            assert torch.equal(out * 1024, torch.round(out * 1024)) and out.abs().max() < 2 ** 14
            assert torch.equal(out.float().double(), out)
            assert col.abs().sum() > 0 and (out.half().double() != out).any()    # non-trivial, and the store does round


def test_int8_oracle_on_the_lattice_needs_no_allowance(oracle_mod):
    """test_mdconv_int8_vs_oracle allows +-1 LSB on 1 % of outputs for the fp32 rounding of sampling coordinates.
    With int8 offsets at scale 1/2 every coordinate is a multiple of 1/2 -- exact in fp32 and in float64 alike --
    so on these inputs that allowance has no cause: the oracle's coordinates equal the exact ones, and the oracle
    repeats itself bit for bit (OpenMP thread count does not enter)."""
    lat = U.lattice(U.LATTICE_B, 128, 260, U.LATTICE_H, U.LATTICE_W, 1, 1, 1)
    q = U.lattice_int8(lat)
    coord32 = (q["offset"].float() * np.float32(q["s_o"]))
    assert torch.equal(coord32.double(), q["offset"].double() * 0.5)
    near = lat["offset"].abs() <= 63.5
    assert torch.equal(coord32[near], lat["offset"][near])           # the same tap targets as the fp16 lattice
    assert (coord32[~near].abs() == 63.5).all()
    args = (q["x"].numpy(), q["s_x"], q["offset"].numpy(), q["s_o"], q["mask"].numpy(), q["s_m"], q["weight"].numpy(),
            q["s_w"], q["bias"].numpy(), 4.0, (1, 1), (1, 1), (1, 1), 1, 1)
    a = oracle_mod.mdconv_s8(*args)
    b = oracle_mod.mdconv_s8(*args)
    assert np.array_equal(a, b) and np.abs(a.astype(np.int32)).max() > 8
