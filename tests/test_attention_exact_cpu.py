"""CPU-only proof of the construction of util_exact_attention.py, for every (dtype, shape, E) that
test_attention_exact_gpu.py runs: the partition meets its conditions, the plan mirror agrees with the library and its
boundaries with a brute-force walk, the float64 softmax of the constructed operands IS the class means, the off-class
logit gap leaves exp2 no choice but 0, and an fp32 emulation of the kernels' online softmax (running maximum, alpha,
fp32 row sums per lane half, fp16 probabilities for the fp16 variant, flushed exp2) gives the expected bits in the
kernels' own tile / wave / split order and in a shuffled one.  Exact equality is therefore a fair demand of any correct
implementation; nothing here runs a kernel."""
import numpy as np
import pytest

import util_exact_attention as X

QKV_CASES = [(dt, B, Lq, Lkv, E, "qkv") for dt in X.QKV_DTYPES for (B, Lq, Lkv) in X.QKV_SHAPES for E in X.QKV_DIMS]
SELF_CASES = [("float16", h, n, n, X.SELF_ATTN_DIM, "self_attention") for n in X.SELF_ATTN_N for h in X.SELF_ATTN_HEADS]
CASES = QKV_CASES + SELF_CASES
IDS = ["%s-%s-%dx%dx%dx%d" % (c[5], c[0], *c[1:5]) for c in CASES]
F32 = np.float32


def _scale_log2e(E, kernel):
    if kernel == "self_attention":                         # float(hd ** -0.5) -> float, * 1.4426950408889634f
        return F32(F32(E ** -0.5) * X.LOG2E32)
    return F32(X.LOG2E32 / np.sqrt(F32(E)))                # 1.4426950408889634f / sqrtf((float)E)


def _np_dtype(dtype):
    return np.float16 if X.is_half(dtype) else np.float32


def test_plan_mirror_matches_the_issue_and_the_library():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    B, Lq, Lkv = X.QKV_SPLIT_SHAPE
    for dt in X.QKV_DTYPES:
        for E in X.QKV_DIMS:
            pl = X.plan(dt, B, Lq, Lkv, E)
            assert pl["nsplit"] == (3 if pl["NW"] == 8 else 6) and pl["NW"] == (8 if dt == "float16" and E <= 64 else 4)
    for (dt, B, Lq, Lkv, E, _) in QKV_CASES:                # the workspace is a pure function of the plan
        pl = X.plan(dt, B, Lq, Lkv, E)
        want = pl["nsplit"] * B * Lq * (E + 2) * 4 if pl["nsplit"] > 1 else 0
        assert lib.bevops_qkv_workspace_size(1 if X.is_half(dt) else 0, B, Lq, Lkv, E) == want, (dt, B, Lq, Lkv, E)
    pl = X.plan("float16", 1, 70, 70, 32)                   # 3 tiles, 8 waves: five waves own no key
    assert pl["NW"] == 8 and sorted(set(pl["wave"])) == [0, 1, 2]
    pl = X.plan("float16", 3, 900, 900, 32, "self_attention")
    assert pl["wave"] == [t // 4 for t in range(29)] and pl["nsplit"] == 1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_partition_and_boundaries(case):
    dt, B, Lq, Lkv, E, kernel = case
    d = X.cached_inputs(*case)
    pl = d["plan"]
    # brute force: walk the keys, note where the (split, wave, tile) that owns a key changes; and the last key
    if kernel == "qkv":
        NW, tps = X.qkv_waves(dt, E), pl["tiles_per_split"]

        def owner(j):
            t_begin = j // 32 // tps * tps
            return t_begin // tps, (j // 32 - t_begin) % NW, j // 32
    else:
        per = -(-((Lkv + 31) // 32) // 8)

        def owner(j):
            return 0, next(w for w in range(8) if w * per <= j // 32 < (w + 1) * per), j // 32
    walk = {j for j in range(1, Lkv) if owner(j) != owner(j - 1)} | ({Lkv - 1} if Lkv > 1 else set())
    assert d["bounds"] == sorted(walk)
    assert [pl["wave"][t] for t in range(pl["ntiles"])] == [owner(32 * t)[1] for t in range(pl["ntiles"])]
    assert [pl["split"][t] for t in range(pl["ntiles"])] == [owner(32 * t)[0] for t in range(pl["ntiles"])]
    assert len(d["classes"]) == B
    for classes in d["classes"]:
        X.check_classes(classes, Lkv, d["bounds"], pl)
        assert len(classes) <= Lq                            # every class is aimed at
    if B > 1 and Lkv > 1:                                    # a batch / head mix-up shows (one key: through v alone)
        assert d["classes"][0] != d["classes"][1] and not np.array_equal(d["want"][0], d["want"][1])
    if B > 1:
        assert not np.array_equal(d["v"][0], d["v"][1])
    # the operands are what the docstring says: binary16 numbers, codes on nb channels, small integers
    for name in ("q", "k", "v"):
        assert np.array_equal(d[name].astype(np.float16).astype(F32), d[name])
    assert set(np.unique(np.abs(d["k"]))) <= {0.0, X.AMP} and (np.abs(d["k"]) == X.AMP).sum(-1).max() == d["nb"] <= 16
    assert np.abs(d["v"]).max() <= X.VMAX and np.array_equal(d["v"], np.round(d["v"]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_softmax_is_the_class_means_and_the_gap_is_wide(case):
    dt, B, Lq, Lkv, E, kernel = case
    d = X.cached_inputs(*case)
    q, k, v = (d[n].astype(np.float64) for n in "qkv")
    s = q @ k.transpose(0, 2, 1) / np.sqrt(E)
    w = np.exp(s - s.max(-1, keepdims=True))
    got = (w / w.sum(-1, keepdims=True)) @ v
    npdt = _np_dtype(dt)
    assert np.array_equal(got.astype(npdt), d["want"].astype(npdt))
    assert np.array_equal(d["want"].astype(npdt).astype(np.float64), d["want"])      # the cast rounds nothing
    # fp32 scores (exact integers) times the kernel's fp32 scale: on-class ties are bit-identical, everything else
    # is at least 150 below in log2 units (2^-150 < half the smallest fp32 subnormal)
    s32 = (d["q"] @ d["k"].transpose(0, 2, 1)).astype(F32)
    assert np.array_equal(s32.astype(np.float64), q @ k.transpose(0, 2, 1))
    t = s32 * _scale_log2e(E, kernel)
    assert t.dtype == F32
    top = t.max(-1, keepdims=True)
    off = np.where(t == top, -np.inf, t)
    for b, classes in enumerate(d["classes"]):
        sizes = np.array([len(c) for c in classes])
        target = (np.arange(Lq) + 3 * b + 1) % len(classes)
        assert np.array_equal((t[b] == top[b]).sum(-1), sizes[target])               # the ties are the class, exactly
    if np.isfinite(off).any():
        assert (top - off).min() >= 150.0


def _exp2(x):
    """v_exp_f32 on an fp32 argument <= 0, results below the normal range flushed to 0."""
    with np.errstate(under="ignore"):
        y = np.exp2(x.astype(F32)).astype(F32)
    y[y < 2.0 ** -126] = 0.0
    return y


def _wave(q, k, v, tiles, Lkv, scale, half):
    """One wave's state after its key tiles, for every query of a batch: (m [Lq], l [Lq, 2 lane halves], acc)."""
    Lq, E = q.shape
    m, l, acc = np.full(Lq, -np.inf, F32), np.zeros((Lq, 2), F32), np.zeros((Lq, E), F32)
    for t in tiles:
        keys = np.arange(32 * t, min(32 * t + 32, Lkv))     # (keys past Lkv are -inf: weight 0)
        s = (q @ k[keys].T).astype(F32) * scale
        m_new = np.maximum(m, s.max(1))
        alpha = _exp2(m - m_new)
        m = m_new
        p = _exp2(s - m_new[:, None])
        hi = (keys & 4) != 0                                  # key (r & 3) + 8 (r >> 2) + 4 hi: the partner lane's
        l[:, 0] = l[:, 0] * alpha + p[:, ~hi].sum(1, dtype=F32)
        l[:, 1] = l[:, 1] * alpha + p[:, hi].sum(1, dtype=F32)
        pv = p.astype(np.float16).astype(F32) if half else p
        acc = acc * alpha[:, None] + (pv @ v[keys]).astype(F32)
    return m, l, acc


def _merge(states, order):
    """(maximum, sum, accumulator) of several partial states, added in `order`."""
    m_all = np.max([s[0] for s in states], 0)
    l_tot, o = np.zeros_like(m_all), np.zeros_like(states[0][2])
    for i in order:
        m, l, acc = states[i]
        f = _exp2(m - m_all)
        l_tot = l_tot + (l[:, 0] + l[:, 1]) * f
        o = o + acc * f[:, None]
    return m_all, np.stack([l_tot, np.zeros_like(l_tot)], 1), o


def _emulate(d, dt, E, kernel, groups, rng=None):
    """groups: [split][wave] -> list of tiles.  rng: shuffle the merge orders too."""
    half = X.is_half(dt)
    B, Lq, _ = d["q"].shape
    Lkv = d["k"].shape[1]
    scale = _scale_log2e(E, kernel)
    out = np.empty((B, Lq, E), F32)
    order = (lambda n: rng.permutation(n)) if rng is not None else range
    for b in range(B):
        parts = []
        for waves in groups:
            states = [_wave(d["q"][b], d["k"][b], d["v"][b], tiles, Lkv, scale, half) for tiles in waves]
            parts.append(_merge(states, order(len(states))))
        m, l, o = _merge(parts, order(len(parts))) if len(parts) > 1 else parts[0]
        out[b] = o * (F32(1.0) / (l[:, 0] + l[:, 1]))[:, None]
    return out.astype(_np_dtype(dt))


@pytest.mark.parametrize("heads", X.SELF_ATTN_HEADS)
@pytest.mark.parametrize("n", X.SELF_ATTN_TIE_N)
def test_all_keys_tie_is_exact_too(n, heads):
    d = X.tie_inputs(heads, n, X.SELF_ATTN_DIM)
    want = d["want"].astype(np.float16)
    assert np.array_equal(want.astype(np.float64), d["want"])                         # a binary16 number
    assert np.array_equal(_emulate(d, "float16", X.SELF_ATTN_DIM, "self_attention", [[[0]] + [[]] * 7]), want)
    assert np.array_equal(_emulate(d, "float16", X.SELF_ATTN_DIM, "qkv", [[[0]] + [[]] * 7]), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_online_softmax_gives_the_expected_bits_in_any_order(case):
    dt, B, Lq, Lkv, E, kernel = case
    d = X.cached_inputs(*case)
    pl = d["plan"]
    want = d["want"].astype(_np_dtype(dt))
    # the kernel's order: split by split, wave w owns its tiles in ascending order, waves and splits merge ascending
    groups = [[[t for t in range(pl["ntiles"]) if pl["split"][t] == s and pl["wave"][t] == w]
               for w in range(pl["NW"])] for s in range(pl["nsplit"])]
    assert sorted(t for waves in groups for tiles in waves for t in tiles) == list(range(pl["ntiles"]))
    assert np.array_equal(_emulate(d, dt, E, kernel, groups), want)
    # any other order: tiles dealt at random to a random number of waves and splits (some of them without keys)
    rng = np.random.default_rng([Lq, Lkv, E, B])
    tiles = rng.permutation(pl["ntiles"])
    nsplit = int(rng.integers(1, min(4, pl["ntiles"]) + 1))
    groups = []
    for part in np.array_split(tiles, nsplit):               # every split holds a key, as in the kernel
        nw = int(rng.integers(1, 9))
        waves = [[] for _ in range(nw)]
        for t in part:
            waves[int(rng.integers(0, nw))].append(int(t))
        groups.append(waves)
    assert np.array_equal(_emulate(d, dt, E, kernel, groups, rng), want)
