"""Operands on which the attention kernels (csrc/qkv.hip: qkv / qkv2, fp32 and fp16; csrc/attention.hip:
self_attention_qkv) make NO rounding at all, so that the result is "the mean of these named V rows", bit for bit,
whatever order key tiles, lane halves, waves and key splits are merged in.  Plain numpy; shares no code with the
package.  Used by test_attention_exact_cpu.py (which proves the construction without a GPU) and
test_attention_exact_gpu.py (torch.equal, no tolerance).

The construction.
  * The keys of a batch (or head) are partitioned into classes of 1, 2 or 4 keys.  Class c is written in
    nb = max(1, ceil(log2(#classes))) bits; nb channels are picked by a seeded permutation of range(E).  A key of class
    c holds +32 / -32 on those channels according to the bits of c and 0 elsewhere; a query aimed at class t holds the
    code of t by the same rule.  Everything is a binary16 number.
  * A dot product is 1024 * (agreeing bits - disagreeing bits): an integer multiple of 1024 of magnitude <= 16 * 1024,
    exact in any fp32 accumulation order.  Keys of one class have identical rows, hence bit-identical scores: ties.
    Another class differs in at least one bit and scores lower by >= 2 * 1024 * log2(e) / sqrt(E) in log2 units: 261 at
    E = 128, 522 at E = 32, 737 at E = 16.  exp2 of -261 is below 2^-149: 0 in fp32, flushed or not.
  * On-class weights are exp2(0) = 1, the row sum is n in {1, 2, 4}, 1.f / n is exact.  V holds integers in [-8, 8]:
    sums of <= 4 rows and their quarter are exact in binary16 and fp32.
  * Expected: out[b, i, :] = mean of v[b, j, :] over the class query i aims at, in float64.

Where the partition puts its classes is what makes a routing or counting mistake show (make_classes): a pair across
every key index at which the owner of a key changes (tile, wave, split) and across the last key, a quad over three
tiles of two waves, classes across key splits, the last key (the one a clamped load duplicates) tied to tile 0.
"""
import functools
import math

import numpy as np

AMP = 32.0                  # |q|, |k| on the code channels
VMAX = 8                    # |v| <= VMAX, integers
CUS = 256                   # kQkvCUs
SELF_ATTN_WAVES = 8         # kAtWaves
SELF_ATTN_DIM = 32          # kAtD
LOG2E32 = np.float32(1.4426950408889634)


def is_half(dtype):
    return "16" in str(dtype)


def qkv_waves(dtype, E):
    return 8 if is_half(dtype) and E <= 64 else 4


def plan(dtype, B, Lq, Lkv, E, kernel="qkv"):
    """Mirror of qkv_waves / qkv_plan (csrc/qkv.hip) or, kernel="self_attention", of the key ranges of
    csrc/attention.hip.  wave[t] / split[t]: the wave and the grid.z split that own key tile t."""
    ntiles = (Lkv + 31) // 32
    if kernel == "self_attention":
        NW = SELF_ATTN_WAVES
        per = (ntiles + NW - 1) // NW                      # contiguous ranges of `per` key blocks
        return dict(kernel=kernel, NW=NW, ntiles=ntiles, nsplit=1, tiles_per_split=ntiles,
                    wave=[t // per for t in range(ntiles)], split=[0] * ntiles)
    assert kernel == "qkv"
    NW = qkv_waves(dtype, E)
    blocks = B * ((Lq + 31) // 32)
    ns = 1
    if blocks < 3 * CUS // 4:
        want = (2 * CUS + blocks - 1) // blocks
        most = ntiles // (2 * NW)
        ns = max(1, min(want, most))
    tps = (ntiles + ns - 1) // ns
    nsplit = (ntiles + tps - 1) // tps
    return dict(kernel=kernel, NW=NW, ntiles=ntiles, nsplit=nsplit, tiles_per_split=tps,
                wave=[(t % tps) % NW for t in range(ntiles)],      # (tile - t_begin) % NW
                split=[t // tps for t in range(ntiles)])


def boundaries(pl, Lkv):
    """Key indices b (1 <= b < Lkv) at which key b has another owner than key b - 1 -- every multiple of 32, every
    change of the owning wave, every split start -- and the last key Lkv - 1."""
    out = {32 * t for t in range(1, pl["ntiles"])}                # a new tile
    out |= {32 * t for t in range(1, pl["ntiles"]) if pl["wave"][t] != pl["wave"][t - 1]}
    out |= {32 * s * pl["tiles_per_split"] for s in range(1, pl["nsplit"])}
    out.add(Lkv - 1)
    return sorted(b for b in out if 1 <= b < Lkv)


def straddles(cls, b):
    return len(cls) == 2 and cls[0] < b <= cls[1]


def make_classes(Lkv, bounds, seed, pl, max_classes=None):
    """Partition range(Lkv) into classes (sorted tuples) of 1, 2 or 4 keys; see the module docstring and
    check_classes() for what it guarantees.  max_classes: the number of queries that will observe them."""
    rng = np.random.default_rng([int(seed), Lkv, 77])
    free = np.ones(Lkv, bool)
    classes = []

    def take(members):
        members = tuple(sorted(int(m) for m in members))
        assert len(set(members)) == len(members) and all(free[m] for m in members), members
        free[list(members)] = False
        classes.append(members)

    # the last key -- the one the clamped loads of a partial tile duplicate -- with a key of tile 0
    if Lkv > 32:
        take((31 if Lkv == 33 else int(rng.integers(0, 31)), Lkv - 1))
    # a pair across every boundary: {b - 1, b}, else the nearest free keys on both sides, else one that is there
    for b in bounds:
        if free[b - 1] and free[b]:
            take((b - 1, b))
            continue
        if (b - 1, b) in classes:
            continue
        lo = next((j for j in range(b - 1, max(b - 9, -1), -1) if free[j]), None)
        hi = next((j for j in range(b, min(b + 8, Lkv)) if free[j]), None)
        if lo is not None and hi is not None:
            take((lo, hi))
        else:
            assert any(straddles(c, b) for c in classes), b
    # a quad over the first two, a middle and the last tile with a free key: three or more tiles, two or more waves,
    # and with a key split the first and the last split
    if pl["ntiles"] >= 3:
        members = []
        for t in (0, 1, pl["ntiles"] // 2, pl["ntiles"] - 1):
            while True:
                cand = [j for j in range(32 * t, min(32 * t + 32, Lkv)) if free[j] and j not in members]
                if cand:
                    break
                t -= 1
            members.append(cand[int(rng.integers(0, len(cand)))])
        take(members)
    # the rest: quads and distant pairs by a seeded permutation, and singles -- at least a quarter of all classes,
    # and as many quads as it takes for the queries to observe every class
    rest = rng.permutation(np.flatnonzero(free))
    F, R = len(classes), len(rest)
    f = R // 16
    while True:
        rem = R - 4 * f
        s = -(-(2 * F + rem + 2 * f) // 7)                 # 3 s >= F + p + f with p = (rem - s) / 2
        s += (rem - s) % 2
        s = min(s + 2, rem)
        p = (rem - s) // 2
        assert s >= 0 and s + 2 * p + 4 * f == R
        if max_classes is None or F + f + p + s <= max_classes or rem < 4:
            break
        f += 1
    for i in range(f):
        take(rest[4 * i:4 * i + 4])
    for i in range(p):
        take(rest[4 * f + 2 * i:4 * f + 2 * i + 2])
    for j in rest[4 * f + 2 * p:]:
        take((j,))
    assert not free.any()
    return [classes[i] for i in rng.permutation(len(classes))]


def check_classes(classes, Lkv, bounds, pl):
    """The conditions a partition must meet (AssertionError otherwise)."""
    flat = sorted(j for c in classes for j in c)
    assert flat == list(range(Lkv)), "every key in exactly one class"
    assert all(len(c) in (1, 2, 4) and tuple(sorted(c)) == tuple(c) for c in classes)
    for b in bounds:
        assert any(straddles(c, b) for c in classes), ("no pair across boundary", b)
        if b != Lkv - 1:                                   # (the last key's partner is in tile 0)
            near = [c for c in classes if straddles(c, b) and c[1] - c[0] <= 16]
            assert near, ("no nearby pair across boundary", b)
    tiles = lambda c: {j // 32 for j in c}                                   # noqa: E731
    waves = lambda c: {(pl["split"][j // 32], pl["wave"][j // 32]) for j in c}   # noqa: E731
    splits = lambda c: {pl["split"][j // 32] for j in c}                     # noqa: E731
    if pl["ntiles"] >= 3:
        assert any(len(c) == 4 and len(tiles(c)) >= 3 and len(waves(c)) >= 2 for c in classes)
    if pl["nsplit"] > 1:
        assert any(len(c) == 2 and len(splits(c)) == 2 for c in classes)
        assert any(len(c) == 4 and len(splits(c)) >= 2 for c in classes)
    if Lkv > 32:
        last = next(c for c in classes if Lkv - 1 in c)
        assert any(j < 32 for j in last), "the last key shares a class with a key of tile 0"
    assert 4 * sum(len(c) == 1 for c in classes) >= len(classes), "a quarter of the classes are singles"


def _codes(n, nb):
    """[n, nb] of +-AMP: bit i of the class number -> +AMP (set) or -AMP."""
    bits = (np.arange(n)[:, None] >> np.arange(nb)[None, :]) & 1
    return np.where(bits == 1, AMP, -AMP).astype(np.float32)


def make_inputs(dtype, B, Lq, Lkv, E, kernel="qkv", seed=0):
    """q [B, Lq, E], k, v [B, Lkv, E] (float32 arrays of binary16 numbers), want [B, Lq, E] float64, and the plan,
    the boundaries and the per-batch classes.  kernel="self_attention": B is the number of heads, Lq == Lkv."""
    pl = plan(dtype, B, Lq, Lkv, E, kernel)
    bounds = boundaries(pl, Lkv)
    parts = [make_classes(Lkv, bounds, 1000 * seed + b, pl, max_classes=Lq) for b in range(B)]
    ncls = max(len(p) for p in parts)
    nb = max(1, math.ceil(math.log2(ncls)))
    assert nb <= min(16, E), (nb, E)
    rng = np.random.default_rng([int(seed), B, Lq, Lkv, E])
    chan = rng.permutation(E)[:nb]                         # the same code for every batch
    code = _codes(ncls, nb)
    q = np.zeros((B, Lq, E), np.float32)
    k = np.zeros((B, Lkv, E), np.float32)
    v = rng.integers(-VMAX, VMAX + 1, size=(B, Lkv, E)).astype(np.float32)
    want = np.zeros((B, Lq, E), np.float64)
    for b, classes in enumerate(parts):
        n = len(classes)
        assert Lq >= n, f"{n} classes but only {Lq} queries: a class would go unobserved"
        cls_of_key = np.empty(Lkv, np.int64)
        mean = np.empty((n, E), np.float64)
        for c, members in enumerate(classes):
            cls_of_key[list(members)] = c
            mean[c] = v[b, list(members)].astype(np.float64).mean(0)
        target = (np.arange(Lq) + 3 * b + 1) % n
        k[b][:, chan] = code[cls_of_key]
        q[b][:, chan] = code[target]
        want[b] = mean[target]
    return dict(q=q, k=k, v=v, want=want, plan=pl, bounds=bounds, classes=parts, chan=chan, nb=nb)


@functools.lru_cache(maxsize=None)
def cached_inputs(dtype, B, Lq, Lkv, E, kernel="qkv"):
    """make_inputs once per case, shared by the tests of a session; the arrays are read-only."""
    d = make_inputs(dtype, B, Lq, Lkv, E, kernel)
    for name in ("q", "k", "v", "want"):
        d[name].setflags(write=False)
    return d


def pack_self_attention(d):
    """make_inputs(kernel="self_attention") -> qkv [n, 3, heads, 32] float32, want [n, heads * 32] float64."""
    qkv = np.stack([d["q"], d["k"], d["v"]], 0).transpose(2, 0, 1, 3)          # [3, heads, n, 32] -> [n, 3, heads, 32]
    want = d["want"].transpose(1, 0, 2).reshape(d["want"].shape[1], -1)
    return qkv.copy(), want.copy()


def uniform_inputs(B, Lq, Lkv, E):
    """q = 0 (every key weighs 1 / Lkv), v[j, ch] = (j % E == ch): out[.., ch] = count_ch / Lkv, in float64."""
    q = np.zeros((B, Lq, E), np.float32)
    k = np.random.default_rng([Lkv, E]).integers(-VMAX, VMAX + 1, size=(B, Lkv, E)).astype(np.float32)
    v = np.zeros((B, Lkv, E), np.float32)
    v[:, np.arange(Lkv), np.arange(Lkv) % E] = 1.0
    count = np.bincount(np.arange(Lkv) % E, minlength=E).astype(np.float64)
    want = np.broadcast_to(count / Lkv, (B, Lq, E)).copy()
    return q, k, v, want, count


def tie_inputs(B, L, E, seed=0):
    """q = 0, L a power of two <= 16: every key weighs exactly 1 / L and out = the mean of all V rows (integers in
    [-8, 8]: the sum is below 2^7 and its 1 / L a multiple of 2^-4, a binary16 number).  A kernel that stages zero K
    rows past L (attention.hip) ties them with the real keys: only its `key < n` mask keeps them out of the sum, which
    the class codes cannot show (a zero row scores below every aimed-at class)."""
    assert L in (1, 2, 4, 8, 16)
    rng = np.random.default_rng([int(seed), B, L, E, 5])
    q = np.zeros((B, L, E), np.float32)
    k = rng.integers(-VMAX, VMAX + 1, size=(B, L, E)).astype(np.float32)
    v = rng.integers(-VMAX, VMAX + 1, size=(B, L, E)).astype(np.float32)
    want = np.broadcast_to(v.astype(np.float64).mean(1, keepdims=True), (B, L, E)).copy()
    return dict(q=q, k=k, v=v, want=want)


def ulp(x, dtype):
    """Spacing of the format at |x| (x a float64 array; 0 where x == 0): 2^(floor(log2 |x|) - mantissa bits), not
    below the format's smallest subnormal step."""
    mant, emin = (10, -14) if is_half(dtype) else (23, -126)
    ax = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    return np.where(ax > 0, np.ldexp(1.0, (np.maximum(e, emin) - mant).astype(np.int64)), 0.0)


# the shapes of test_attention_exact_gpu.py (and of the CPU proof, which must cover the same ones)
QKV_DTYPES = ("float32", "float16")
QKV_DIMS = (16, 32, 48, 64, 80, 96, 112, 128)
QKV_SHAPES = ((2, 1, 1), (3, 37, 31), (1, 33, 32), (2, 40, 33), (1, 70, 70), (2, 300, 517), (1, 800, 1541))
QKV_SPLIT_SHAPE = (1, 800, 1541)
UNIFORM_LKV = (1, 33, 517, 1541)
UNIFORM_B, UNIFORM_LQ = 1, 33          # two blocks: the 1541 keys are split
SELF_ATTN_N = (1, 31, 32, 33, 257, 900, 1024)
SELF_ATTN_HEADS = (1, 3)
SELF_ATTN_TIE_N = (1, 2, 4, 8, 16)      # exact: powers of two inside one partial key block
SELF_ATTN_UNIFORM_N = (31, 33, 257)      # a key more or less moves a channel by >= 1 / 258 of its value; bar: 1 / 1024
