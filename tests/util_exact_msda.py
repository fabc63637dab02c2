"""Operands on which the fp32 / fp16 multi-scale deformable attention kernels (csrc/msda*.hip) and the fused SCA
entries make NO rounding before their final store, a float64 reference that predicts every output bit, and the tier-2
error budget for random logits.  Plain numpy; shares no code with oracle/ or the package.  Used by
test_msda_exact_cpu.py (which checks all of this without a GPU) and test_msda_exact_gpu.py (tolerance 0).

The lattice.
  * A sampling location x = ref_x * W + off_x - 0.5 (y likewise) sits on a 1/8 grid; on a level with W >= 160 half of
    the targets at x >= 128 are moved onto the 1/16 grid (x + 1/16 needs 12 significant bits: a kernel that forms
    locations in binary16 is wrong there).  ref is a multiple of 1/8 in [0, 1], off = target + 0.5 - ref * S is checked to
    be a binary16 number (where the 1/16 step would not survive, the target stays on the 1/8 grid).  ref * S, + off and
    - 0.5 are exact in fp32 (multiples of 1/16 below 2^9), fused or not.
  * Targets are drawn per (batch, query, head, level, point) from N_CLASS = 18 classes per axis (classes(S)): both
    sides of every border, integer coordinates, the centre.  -1, S and S + 0.5 fail the reference's strict gate.
  * Bilinear weights are products of multiples of 1/8 (1/16): multiples of 2^-6 (2^-7), exact in binary16 and fp32.
  * Tier 1 logits are k-hot: k in {1, 2, 4, 8} logits equal 0, the others -30000 (a binary16 number).  exp(0) = 1,
    exp(-30000) = 0, the normaliser is k: softmax weights are exactly 1/k or 0, and acc / k == acc * (1 / k).
  * Values are integers, |v| <= amp (256 by default), so every weight x value product is a multiple of 2^-7 below 2^9
    and the sum of the magnitudes of ALL terms of an output stays below 2^17 * 2^-7: every partial sum, in any order
    and with or without FMA contraction, is exact in fp32.  Channels 0-3 carry codes (x, y, 16 * level + batch, head),
    the others a hash of (batch, level, y, x, head, channel): a wrong address, level base, head or batch shows.
  * `blend16` levels (narrowing for the head-major kernels that keep small levels in LDS, design/msda.md): hm3 / hm4 / hm5
    blend the four corners of a sample from an LDS-resident level in PACKED BINARY16 (v * w00, then three fp16 FMAs)
    before the fp32 accumulation.  On those levels the value amplitude is 16, so that every product and partial sum of
    a blend is an integer multiple of 2^-6 of magnitude <= 16 = 1024 * 2^-6: a binary16 number.  The codes are taken
    modulo amp + 1 there.
The reference does not assume any of this: it checks every step and raises BudgetError otherwise.

Expected output: the float64 result cast (fp32: exact) or rounded once, RNE, to binary16.  The fused SCA entries
round each camera's row to binary16, form sum_cam mask * row in fp32 (exact: mask in {1, 1/2, 1/4}) and round again.

Tier 2 (random logits, same locations and values).  Only the softmax weights round.  Per output the reference returns
A = sum_j softmax_j * sum_corners c |v| and the bound is

    bar = 3 * 2^-11 * A

  * 2^-11 A: one binary16 rounding of each packed weight e * corner (hm2 - hm5 pack it; relative 2^-11);
  * 2^-11 A >= 2^-11 |out|: the rounding of the stored result;
  * 2^-11 A: __expf, the reciprocal and the fp32 accumulation, each some 2^-20 relative (a generous 2^-11 in all).
The packed-fp16 blend of the staging kernels adds up to four more roundings on the samples of blend16 levels, and a
packed weight below 2^-14 is a binary16 subnormal with an absolute error; neither needed its own term: the largest
err / A measured on the device is 2.15 * 2^-11 (hm3, every level staged; profiles/msda_exact/gpu_tests.log).
"""
import zlib

import numpy as np

HEADS, C = 8, 32
COLD = -30000.0
N_CLASS = 18
BLEND_AMP = 16

RAGGED = ((90, 161), (45, 81), (23, 41), (1, 21))     # two big levels (W >= 160: the 1/16 grid), two LDS-resident ones
STAGED = ((24, 41), (12, 21), (6, 11), (1, 5))        # every level LDS-resident from 2 048 queries on
SMALL = ((9, 11), (4, 5))
TSA = ((50, 50),)
NQ_SCA = 2083                                          # just above the 2 048-query staging threshold, odd
MASK_WEIGHTS = (0.0, 1.0, 0.5, 0.25)


class BudgetError(AssertionError):
    """An intermediate of the reference is not exactly representable: the operands are outside the budget."""


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def classes(S):
    """The 18 target coordinates of an axis of size S."""
    return np.array([-1, -0.875, -0.5, -0.125, 0, 0.125, 0.5, 1, S - 2, S - 1.125, S - 1, S - 0.875, S - 0.5, S - 0.125,
                     S, S + 0.5, S / 2, S // 2 + 0.375], dtype=np.float64)


def f32_exact(v, what):
    v = np.asarray(v, dtype=np.float64)
    if not np.array_equal(v.astype(np.float32).astype(np.float64), v):
        raise BudgetError(f"{what}: not fp32 numbers")
    return v


def f16_exact(v, what):
    v = np.asarray(v, dtype=np.float64)
    if not np.array_equal(v.astype(np.float16).astype(np.float64), v):
        raise BudgetError(f"{what}: not binary16 numbers")
    return v


def to_f16(v):
    """float64 -> binary16, ONE rounding (RNE)."""
    return np.asarray(v, dtype=np.float64).astype(np.float16)


# ------------------------------------------------------------------------------------------------------- cases
def _case(name, levels, bs, nq, P, ppg, shared=False, blend=(), tier=1):
    L = len(levels)
    amps = tuple(BLEND_AMP if l in blend else 256 for l in range(L))
    return dict(id=f"{name}-t{tier}", name=name, levels=tuple(levels), bs=bs, nq=nq, P=P, ppg=ppg, shared=shared,
                blend=tuple(blend), amps=amps, tier=tier, heads=HEADS, C=C, L=L, LP=L * P,
                nk=sum(h * w for h, w in levels), geom=(tuple(levels), bs, nq, P, ppg, shared))


def cases():
    """name -> case.  `*-narrow`: the blend16 narrowing for hm3 / hm4 / hm5 (same locations and logits as `*-full`)."""
    out = {}
    for tier in (1, 2):
        cs = [_case("tsa", TSA, 2, 2500, 4, 1, tier=tier),
              _case("ragged-full", RAGGED, 3, NQ_SCA, 8, 4, tier=tier),
              _case("ragged-narrow", RAGGED, 3, NQ_SCA, 8, 4, blend=(2, 3), tier=tier),
              _case("staged-full", STAGED, 2, NQ_SCA, 8, 4, tier=tier),
              _case("staged-narrow", STAGED, 2, NQ_SCA, 8, 4, blend=(0, 1, 2, 3), tier=tier)]
        if tier == 1:
            cs += [_case(f"small-{nq}", SMALL, 2, nq, 4, 2) for nq in (1, 17, 65)]
            cs += [_case("sca-ragged", RAGGED, 3, NQ_SCA, 8, 4, shared=True, blend=(2, 3)),
                   _case("sca-staged", STAGED, 3, NQ_SCA, 8, 4, shared=True, blend=(0, 1, 2, 3))]
        for c in cs:
            out[c["id"]] = c
    return out


CASES = cases()
TIER1 = [k for k, c in CASES.items() if c["tier"] == 1]


# ---------------------------------------------------------------------------------------------------- operands
def make_values(c):
    """[bs, nk, heads, C] float64 integers, |v| <= amps[level]."""
    bs, heads, ch = c["bs"], c["heads"], c["C"]
    parts = []
    for l, (H, W) in enumerate(c["levels"]):
        amp = c["amps"][l]
        b = np.arange(bs, dtype=np.uint64).reshape(bs, 1, 1, 1, 1)
        y = np.arange(H, dtype=np.uint64).reshape(1, H, 1, 1, 1)
        x = np.arange(W, dtype=np.uint64).reshape(1, 1, W, 1, 1)
        h = np.arange(heads, dtype=np.uint64).reshape(1, 1, 1, heads, 1)
        k = np.arange(ch, dtype=np.uint64).reshape(1, 1, 1, 1, ch)
        with np.errstate(over="ignore"):
            z = (b * np.uint64(0x9E3779B97F4A7C15) + np.uint64(l + 1) * np.uint64(0xC2B2AE3D27D4EB4F)
                 + y * np.uint64(0x165667B19E3779F9) + x * np.uint64(0xD6E8FEB86659FD93)
                 + h * np.uint64(0xA0761D6478BD642F) + k * np.uint64(0xE7037ED1A0B428DB))
            z ^= z >> np.uint64(31)
            z *= np.uint64(0xBF58476D1CE4E5B9)
            z ^= z >> np.uint64(29)
            z *= np.uint64(0x94D049BB133111EB)
            z ^= z >> np.uint64(32)
        v = (z % np.uint64(2 * amp + 1)).astype(np.int64) - amp
        mod = amp + 1
        shape = v.shape[:4]
        v[..., 0] = np.broadcast_to(x[..., 0].astype(np.int64) % mod, shape)
        v[..., 1] = np.broadcast_to(y[..., 0].astype(np.int64) % mod, shape)
        v[..., 2] = np.broadcast_to((16 * l + b[..., 0].astype(np.int64)) % mod, shape)
        v[..., 3] = np.broadcast_to(h[..., 0].astype(np.int64) % mod, shape)
        parts.append(v.reshape(bs, H * W, heads, ch))
    return np.concatenate(parts, axis=1).astype(np.float64)


def make_ops(c):
    """Operands of a case as float64 numpy arrays: value [bs, nk, heads, C], shapes int32 [L, 2], ref [bs, nq, 1, 2 ppg],
    off [B, nq, heads, LP * 2], logit [B, nq, heads, LP] (B = 1 when the offsets / logits are camera-shared, else bs),
    and the bookkeeping of the coverage statistics: cx / cy class indices [B, nq, heads, L, P], jit (moved onto the 1/16
    grid), hot (logit == 0), same [bs, nq] (the camera's reference points are the ones the classes were drawn for),
    mask [bs, nq] (shared cases: the bev_mask weights)."""
    levels, bs, nq, P, ppg, heads, L = c["levels"], c["bs"], c["nq"], c["P"], c["ppg"], c["heads"], c["L"]
    B = 1 if c["shared"] else bs
    r = _rng("loc", c["geom"])
    ref0 = r.integers(0, 9, size=(B, nq, ppg, 2)) / 8.0
    cx = r.integers(0, N_CLASS, size=(B, nq, heads, L, P))
    cy = r.integers(0, N_CLASS, size=(B, nq, heads, L, P))
    g = np.arange(P) % ppg
    off = np.empty((B, nq, heads, L, P, 2))
    jit = np.zeros((B, nq, heads, L, P), dtype=bool)
    for l, (H, W) in enumerate(levels):
        tx, ty = classes(W)[cx[:, :, :, l]], classes(H)[cy[:, :, :, l]]
        rx = ref0[:, :, g, 0][:, :, None, :] * W           # [B, nq, 1, P]
        ry = ref0[:, :, g, 1][:, :, None, :] * H
        if W >= 160:
            j = (tx >= 128) & (r.random(tx.shape) < 0.5)
            ox = tx + j / 16.0 + 0.5 - rx
            j &= ox.astype(np.float16).astype(np.float64) == ox      # the 1/16 step must survive binary16
            jit[:, :, :, l] = j
            tx = tx + j / 16.0
        off[:, :, :, l, :, 0] = tx + 0.5 - rx
        off[:, :, :, l, :, 1] = ty + 0.5 - ry
    f16_exact(off, "sampling offsets")
    if np.abs(off[jit][:, 0]).max(initial=0) >= 128:
        raise BudgetError("an offset on the 1/16 grid is not below 128")
    # reference points per batch entry / camera
    if c["shared"]:
        same = r.random((bs, nq)) < 0.5
        same[0] = True
        other = r.integers(0, 9, size=(bs, nq, ppg, 2)) / 8.0
        ref = np.where(same[:, :, None, None], ref0, other)
        kind = r.integers(0, 5, size=nq)      # 0: no camera, 1: one camera with weight 1, 2: all, 3: one with 1/2, 4: two
        w = np.array(MASK_WEIGHTS)[r.integers(1, 4, size=(bs, nq))]
        cam = r.integers(0, bs, size=nq)
        cam2 = (cam + 1 + r.integers(0, bs - 1, size=nq)) % bs
        one = np.arange(bs)[:, None] == cam[None, :]
        two = one | (np.arange(bs)[:, None] == cam2[None, :])
        mask = np.where(kind == 0, 0.0, np.where(kind == 1, one * 1.0, np.where(kind == 2, w, np.where(
            kind == 3, one * 0.5, two * w))))
    else:
        same, ref, mask = np.ones((bs, nq), dtype=bool), ref0, None
    # logits
    LP = c["LP"]
    rl = _rng("logit", c["geom"], c["tier"])
    if c["tier"] == 1:
        ks = np.array([k for k in (1, 2, 4, 8) if k <= LP])
        k = ks[rl.integers(0, len(ks), size=(B, nq, heads))]
        rank = np.argsort(np.argsort(rl.random((B, nq, heads, LP)), axis=-1), axis=-1)
        hot = rank < k[..., None]
        logit = np.where(hot, 0.0, COLD)
    else:
        logit = rl.standard_normal((B, nq, heads, LP)).astype(np.float16).astype(np.float64)
        hot = np.ones((B, nq, heads, LP), dtype=bool)
    return dict(value=make_values(c), shapes=np.array(levels, dtype=np.int32), ref=ref.reshape(bs, nq, 1, 2 * ppg),
                off=off.reshape(B, nq, heads, LP * 2), logit=logit, cx=cx, cy=cy, jit=jit,
                hot=hot.reshape(B, nq, heads, L, P), same=same, mask=mask)


# --------------------------------------------------------------------------------------------------- reference
def _numerators(c, o):
    """softmax numerators e [B, nq, heads, LP] and their sum: exactly 1 / 0 and k in tier 1."""
    lg = o["logit"]
    if c["tier"] == 1:
        if not np.isin(lg, (0.0, COLD)).all() or not (lg.max(-1) == 0).all():
            raise BudgetError("tier-1 logits are not k-hot")
        e = (lg == 0).astype(np.float64)
        s = e.sum(-1)
        if not np.isin(s, (1, 2, 4, 8)).all():
            raise BudgetError("the normaliser is not a power of two")
    else:
        e = np.exp(lg - lg.max(-1, keepdims=True))
        s = e.sum(-1)
    return e, s


def reference(c, o):
    """float64 MSDA with the reference's rules (strict range gate, per-corner bounds, acc / sum) on the operands of
    make_ops.  Returns dict(out, A), both [bs, nq, heads, C] float64; A = sum_j softmax_j sum_corners c |v| is the tier-2
    scale.  Tier 1: raises BudgetError unless every intermediate is exact in the kernels' formats."""
    bs, nq, heads, ch, P, ppg = c["bs"], c["nq"], c["heads"], c["C"], c["P"], c["ppg"]
    exact = c["tier"] == 1
    e, s = _numerators(c, o)
    B = e.shape[0]
    value, ref, off = o["value"], o["ref"], o["off"]
    n_item = bs * nq * heads
    acc = np.zeros((n_item, ch))
    A = np.zeros((n_item, ch))
    item = np.arange(n_item).reshape(bs, nq, heads)
    bidx = np.broadcast_to(np.arange(bs).reshape(bs, 1, 1), (bs, nq, heads))
    hidx = np.broadcast_to(np.arange(heads).reshape(1, 1, heads), (bs, nq, heads))
    base = 0
    for l, (H, W) in enumerate(c["levels"]):
        blend = l in c["blend"]
        for p in range(P):
            j, g = l * P + p, p % ppg
            ej = np.broadcast_to(e[..., j], (bs, nq, heads)) if B == 1 else e[..., j]
            tx = ref[:, :, 0, 2 * g][:, :, None] * W
            ty = ref[:, :, 0, 2 * g + 1][:, :, None] * H
            ux, uy = tx + off[..., 2 * j], ty + off[..., 2 * j + 1]
            x, y = ux - 0.5, uy - 0.5
            if exact:
                for v, what in ((tx, "ref * W"), (ty, "ref * H"), (ux, "+ off"), (uy, "+ off"), (x, "- 0.5"), (y, "- 0.5")):
                    f32_exact(v, what)
            x, y = np.broadcast_to(x, (bs, nq, heads)), np.broadcast_to(y, (bs, nq, heads))
            live = (ej > 0) & (y > -1) & (x > -1) & (y < H) & (x < W)
            if not live.any():
                continue
            xs, ys, es, it, bb, hh = x[live], y[live], ej[live], item[live], bidx[live], hidx[live]
            x0, y0 = np.floor(xs), np.floor(ys)
            lx, ly = xs - x0, ys - y0
            x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
            tot = np.zeros((es.size, ch))
            mag = np.zeros((es.size, ch))
            for dy, dx, wy, wx in ((0, 0, 1 - ly, 1 - lx), (0, 1, 1 - ly, lx), (1, 0, ly, 1 - lx), (1, 1, ly, lx)):
                yy, xx = y0 + dy, x0 + dx
                ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
                cw = np.where(ok, wy * wx, 0.0)
                v = value[bb, base + np.clip(yy, 0, H - 1) * W + np.clip(xx, 0, W - 1), hh, :]
                w = es * cw
                term = w[:, None] * v
                if exact:
                    f32_exact(cw, "bilinear weight")
                    f16_exact(w, "softmax x bilinear weight")
                    unit = 2.0 ** -7
                    if not np.array_equal(np.rint(term / unit) * unit, term):
                        raise BudgetError("a weight x value product is not a multiple of 2^-7")
                tot += term
                mag += np.abs(term)
            if exact and blend:
                # the packed-fp16 blend of an LDS-resident level: products are multiples of 2^-6, magnitudes sum to <= 2^5
                if not np.array_equal(np.rint(mag * 64) / 64, mag) or mag.max() > 2048 / 64:
                    raise BudgetError(f"level {l}: a packed-fp16 blend is not exact (max sum of magnitudes {mag.max()})")
            acc[it] += tot          # (the items of one sample index are distinct)
            A[it] += mag
        base += H * W
    if exact and A.max() >= 2.0 ** 17:
        raise BudgetError("sum of the magnitudes of an output's terms is not below 2^24 units of 2^-7")
    sb = np.broadcast_to(s, (bs, nq, heads)).reshape(n_item, 1)
    out = acc / sb
    if exact:
        f32_exact(out, "acc / sum")
        if not np.array_equal(acc * (1.0 / sb), out):
            raise BudgetError("acc * (1 / sum) differs from acc / sum")
    shape = (bs, nq, heads, ch)
    return dict(out=out.reshape(shape), A=(A / sb).reshape(shape))


def tier2_bar(r):
    """Per-output bound of |kernel fp16 output - float64 reference| (module docstring)."""
    return 3 * 2.0 ** -11 * r["A"]


def expected(r, dtype):
    """The output bits of an MSDA call: 'fp32' (the float64 result is an fp32 number) or 'fp16' (one RNE rounding)."""
    if dtype == "fp32":
        return f32_exact(r["out"], "output").astype(np.float32)
    return to_f16(r["out"])


def expected_sca(c, o, r):
    """The fused SCA op on a shared case: every camera's row rounded to binary16 (the per-camera scratch rows, or the
    row the planned sampler stores directly when one camera alone sees the query with weight 1), the masked sum over
    the cameras in fp32 (ascending fma chain; exact, checked), rounded to binary16.  [1, nq, heads * C] float16."""
    rows = to_f16(r["out"]).astype(np.float64)                        # [cams, nq, heads, C]
    m = o["mask"]
    f16_exact(m, "bev_mask")
    acc = np.zeros(rows.shape[1:])
    for b in range(c["bs"]):
        acc = f32_exact(acc + m[b][:, None, None] * rows[b], "masked camera sum")
    return to_f16(acc).reshape(1, c["nq"], c["heads"] * c["C"])


def naive(c, o, items):
    """A per-sample loop in Python floats over the given (b, q, h) items: the reference of the reference."""
    P, ppg, ch = c["P"], c["ppg"], c["C"]
    out = np.zeros((len(items), ch))
    for n, (b, q, h) in enumerate(items):
        bi = 0 if c["shared"] else b
        lg = o["logit"][bi, q, h]
        m = max(lg)
        e = [float(np.exp(v - m)) for v in lg]
        acc = np.zeros(ch)
        base = 0
        for l, (H, W) in enumerate(c["levels"]):
            for p in range(P):
                j, g = l * P + p, p % ppg
                x = o["ref"][b, q, 0, 2 * g] * W + o["off"][bi, q, h, 2 * j] - 0.5
                y = o["ref"][b, q, 0, 2 * g + 1] * H + o["off"][bi, q, h, 2 * j + 1] - 0.5
                if not (y > -1 and x > -1 and y < H and x < W):
                    continue
                x0, y0 = int(np.floor(x)), int(np.floor(y))
                lx, ly = x - x0, y - y0
                smp = np.zeros(ch)
                for yy, xx, w in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                                  (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                    if 0 <= yy <= H - 1 and 0 <= xx <= W - 1:
                        smp += w * o["value"][b, base + yy * W + xx, h]
                acc += e[j] * smp
            base += H * W
        out[n] = acc / sum(e)
    return out


def coverage(c, o):
    """[L, N_CLASS, N_CLASS] counts of (x class, y class) among hot samples that sit exactly on their class (not moved
    onto the 1/16 grid) of a batch entry / camera whose reference points are the ones the classes were drawn for and,
    in a shared case, whose bev_mask weight is not 0."""
    bs, L = c["bs"], c["L"]
    cnt = np.zeros((L, N_CLASS, N_CLASS), dtype=np.int64)
    take = o["hot"] & ~o["jit"]
    if c["shared"]:
        use = (o["same"] & (o["mask"] != 0)).any(0)               # [nq]
        take = take & use[None, :, None, None, None]
    for l in range(L):
        t = take[:, :, :, l]
        np.add.at(cnt[l], (o["cx"][:, :, :, l][t], o["cy"][:, :, :, l][t]), 1)
    return cnt


def fp16_shares(v):
    """(share of float64 values that are not binary16 numbers, share that are exact rounding ties, share of zeros)."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    h16 = v.astype(np.float16)
    h = h16.astype(np.float64)
    inexact = h != v
    up = np.nextafter(h16, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h16, np.float16(-np.inf)).astype(np.float64)
    other = np.where(v > h, up, dn)
    tie = inexact & (np.abs(v - h) == np.abs(other - v))
    return float(inexact.mean()), float(tie.mean()), float((v == 0).mean())


# ------------------------------------------------------------------------- the projected form (value projection)
def projection_operands(c, o):
    """features [bs, nk, 256] (integers * 2^-4), weight [256, 256] (a signed permutation matrix * 2^4) and bias [256]
    (integers) in float64, such that features @ weight.T + bias is EXACTLY o['value'] viewed [bs, nk, 256]: one product
    per output column, exact in fp32 and a binary16 number."""
    E = c["heads"] * c["C"]
    r = _rng("proj", c["geom"])
    perm = r.permutation(E)
    sign = r.choice(np.array([-1.0, 1.0]), size=E)
    bias = r.integers(-4, 5, size=E).astype(np.float64)
    weight = np.zeros((E, E))
    weight[np.arange(E), perm] = sign * 16.0
    v = o["value"].reshape(c["bs"], c["nk"], E)
    feats = np.zeros_like(v)
    feats[:, :, perm] = (v - bias) * sign / 16.0
    f16_exact(feats, "features")
    if not np.array_equal(feats @ weight.T + bias, v):
        raise BudgetError("the projection does not reproduce the lattice values")
    return feats, weight, bias
