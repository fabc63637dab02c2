"""The lattice operands and the float64 reference of tests/util_exact_msda.py, checked without a GPU: the reference
against a naive loop and, bit for bit, against the C oracle; the budget of every case test_msda_exact_gpu.py runs;
the class-pair coverage; how much of the output a tolerance-0 comparison actually pins (non-binary16 values, ties,
exact zeros); the tier-2 budget terms against a direct evaluation."""
import functools

import numpy as np
import pytest

import util_exact_msda as X


@functools.lru_cache(maxsize=None)
def ops(cid):
    return X.make_ops(X.CASES[cid])


@functools.lru_cache(maxsize=None)
def ref(cid):
    return X.reference(X.CASES[cid], ops(cid))


def _items(c, n=40):
    r = np.random.default_rng(7)
    return [(int(r.integers(c["bs"])), int(r.integers(c["nq"])), int(r.integers(c["heads"]))) for _ in range(n)]


@pytest.mark.parametrize("cid", ["small-17-t1", "tsa-t1", "ragged-full-t1", "sca-staged-t1", "staged-narrow-t2"])
def test_reference_equals_a_naive_loop(cid):
    c, o, r = X.CASES[cid], ops(cid), ref(cid)
    items = _items(c)
    want = X.naive(c, o, items)
    got = np.stack([r["out"][b, q, h] for b, q, h in items])
    if c["tier"] == 1:
        assert np.array_equal(got, want)
    else:
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cid", X.TIER1)
def test_budget_holds_and_oracle_agrees_bit_for_bit(oracle_mod, cid):
    """reference() raises BudgetError unless every intermediate is exact; the C oracle's fp32 arithmetic
    (oracle/msda_ref.c) is then exact on the lattice too and must give the same bits."""
    c, o, r = X.CASES[cid], ops(cid), ref(cid)
    want = X.expected(r, "fp32")
    bs = c["bs"]
    off = np.broadcast_to(o["off"], (bs,) + o["off"].shape[1:])
    lg = np.broadcast_to(o["logit"], (bs,) + o["logit"].shape[1:])
    got = oracle_mod.msda_f32(o["value"], o["shapes"], o["ref"], off, lg)
    assert np.array_equal(got, want)
    # every operand is a binary16 number: the fp16 kernels see the same problem
    for k in ("value", "ref", "off", "logit"):
        X.f16_exact(o[k], k)
    if c["shared"]:
        assert X.expected_sca(c, o, r).shape == (1, c["nq"], 256)


def test_budget_error_is_raised_outside_the_budget():
    c = dict(X.CASES["staged-narrow-t1"])
    c["amps"] = (256,) * 4                      # full amplitude on levels whose blend is packed fp16
    with pytest.raises(X.BudgetError):
        X.reference(c, X.make_ops(c))
    c = X.CASES["small-17-t1"]
    o = dict(ops("small-17-t1"))
    o["off"] = o["off"] + 2.0 ** -13            # a location off the lattice: a product that is no multiple of 2^-7
    with pytest.raises(X.BudgetError):
        X.reference(c, o)


@pytest.mark.parametrize("cid", ["tsa-t1", "ragged-full-t1", "staged-full-t1", "sca-ragged-t1", "sca-staged-t1"])
def test_every_class_pair_occurs_on_every_level(cid):
    c, o = X.CASES[cid], ops(cid)
    cnt = X.coverage(c, o)
    assert cnt.shape == (c["L"], X.N_CLASS, X.N_CLASS)
    assert cnt.min() >= 1, (cid, int(cnt.min()))
    # cold samples take every class pair too (weight 0 must contribute exactly 0)
    cold = ~o["hot"]
    for l in range(c["L"]):
        seen = np.zeros((X.N_CLASS, X.N_CLASS), dtype=bool)
        seen[o["cx"][:, :, :, l][cold[:, :, :, l]], o["cy"][:, :, :, l][cold[:, :, :, l]]] = True
        assert seen.all()
    # every (level, point) slot is hot for some item, and every hot count occurs
    assert o["hot"].reshape(-1, c["LP"]).any(0).all()
    assert set(np.unique(o["hot"].reshape(-1, c["LP"]).sum(-1))) == {k for k in (1, 2, 4, 8) if k <= c["LP"]}


def test_small_cases_cover_every_class_per_axis():
    o = ops("small-65-t1")
    for l in range(2):
        for key in ("cx", "cy"):
            assert set(np.unique(o[key][:, :, :, l][o["hot"][:, :, :, l]])) == set(range(X.N_CLASS))


def test_sixteenth_grid_is_present_and_needs_more_than_binary16():
    c, o = X.CASES["ragged-full-t1"], ops("ragged-full-t1")
    assert o["jit"][:, :, :, 0].sum() > 1000 and not o["jit"][:, :, :, 1:].any()
    # the locations of those samples are not binary16 numbers
    W = c["levels"][0][1]
    g = np.arange(c["P"]) % c["ppg"]
    x = o["ref"][:, :, 0, 2 * g][:, :, None, :] * W + o["off"].reshape(c["bs"], c["nq"], 8, 4, 8, 2)[:, :, :, 0, :, 0] - 0.5
    j = o["jit"][:, :, :, 0]
    assert (x[j].astype(np.float16).astype(np.float64) != x[j]).all()
    assert (x[~j].astype(np.float16).astype(np.float64) == x[~j]).all()


@pytest.mark.parametrize("cid", X.TIER1)
def test_shares_of_outputs_a_tolerance_zero_comparison_pins(cid):
    """A truncating or doubly rounding store is only visible on outputs that are not binary16 numbers."""
    c, r = X.CASES[cid], ref(cid)
    inexact, tie, zero = X.fp16_shares(r["out"])
    print(f"{cid}: non-fp16 {inexact:.3f}  ties {tie:.3f}  zeros {zero:.3f}")
    dead = (np.abs(r["out"]).max(-1) == 0).mean()
    assert dead > 0.01 or c["nq"] < 17                 # items all of whose hot samples fail the gate: exactly 0
    if c["nq"] >= 17:
        # (amplitude 16 on every level leaves few 12-bit results: the all-staged narrow cases pin the LDS blend and its
        # addresses; the store rounding of those kernels is pinned by the ragged cases and the one-level cases)
        all_blend = len(c["blend"]) == c["L"]
        assert inexact > (0.001 if all_blend else 0.10), inexact
        assert tie > (0.001 if all_blend else 0.005), tie


@pytest.mark.parametrize("cid", ["tsa-t2", "ragged-narrow-t2", "staged-narrow-t2"])
def test_tier2_budget_terms_against_a_direct_evaluation(cid):
    c, o, r = X.CASES[cid], ops(cid), ref(cid)
    for (b, q, h) in _items(c, 12):
        lg = o["logit"][b, q, h]
        sm = np.exp(lg - lg.max())
        sm /= sm.sum()
        A = np.zeros(c["C"])
        base = 0
        for l, (H, W) in enumerate(c["levels"]):
            for p in range(c["P"]):
                j, g = l * c["P"] + p, p % c["ppg"]
                x = o["ref"][b, q, 0, 2 * g] * W + o["off"][b, q, h, 2 * j] - 0.5
                y = o["ref"][b, q, 0, 2 * g + 1] * H + o["off"][b, q, h, 2 * j + 1] - 0.5
                if not (y > -1 and x > -1 and y < H and x < W):
                    continue
                x0, y0 = int(np.floor(x)), int(np.floor(y))
                lx, ly = x - x0, y - y0
                for yy, xx, w in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                                  (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                    if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                        t = sm[j] * w * np.abs(o["value"][b, base + yy * W + xx, h])
                        A += t
            base += H * W
        assert np.allclose(r["A"][b, q, h], A, rtol=1e-12, atol=1e-15)
    bar = X.tier2_bar(r)
    assert np.array_equal(bar, 3 * 2.0 ** -11 * r["A"]) and (np.abs(r["out"]) <= r["A"] * (1 + 1e-12)).all()
    # the bar is relative to each output's own magnitude: 0.15 % of A, against the parity tests' 1e-2 absolute on a
    # signal of standard deviation 0.15 (7 %)
    print(f"{cid}: signal std {r['out'].std():.1f}, median bar {np.median(bar):.3e}, median bar / std "
          f"{np.median(bar) / r['out'].std():.2e}")
    assert np.median(bar) < 0.01 * r["out"].std()


def test_projection_operands_reproduce_the_lattice_values():
    c, o = X.CASES["sca-ragged-t1"], ops("sca-ragged-t1")
    feats, weight, bias = X.projection_operands(c, o)
    assert (np.abs(weight).sum(0) == 16).all() and (np.abs(weight).sum(1) == 16).all()
    X.f16_exact(weight, "weight")
    X.f16_exact(bias, "bias")
