"""bevops_bev_align_stack_s8 (csrc/bev_align_s8.hip) through functions.bev_align_stack in the guarded arena of
tests/util_arena.py under both poisons, against `bev_align_stack_q_plain` (the float64 statement on the launch's own
fp32 positions) and, for the derived bound, the unrounded float64 blend of tests/util_bev_align.py.

A lane owns 16 channels: C = 16 is one pass with one vector per pixel, C = 80 two passes with V = 5 (no divisor of 64),
C = 272 the instance that re-reads curr (more than four passes).  The 9 x 11 map is one tile and a bit in y and a
partial second tile in x.  Every byte of the operands' buffers outside the written slices is compared."""
import functools
import itertools

import pytest
import torch

import util_bev_align as U
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

H, W = 9, 11
SHAPES = [(B, C, T) for C in (16, 80, 272) for T in (1, 2) for B in (1, 2)]
CASES = list(itertools.product(SHAPES, (False, True)))
IDS = [f"B{s[0]}-C{s[1]}-T{s[2]}" + ("-sliced" if sl else "") for s, sl in CASES]


def run(shape, sliced, curr, hist, meta):
    """One call per poison on arena buffers -> (out [B, (T + 1) C, H, W], hist after) int8 on the CPU; the bytes the call
    must not touch are checked, and both poisons must give the same bytes (an int8 kernel that reads what it should not
    shows it as a difference)."""
    from bevformer_tensorrt_amd.functions import bev_align_stack
    B, C, T = shape
    write_slot = int(meta[0])
    pad, off = (48, 16) if sliced else (0, 0)
    results = []
    for poison in POISONS:
        arena = Arena(8 << 20, poison)
        cbuf = arena.empty((B, C + pad, H, W), torch.int8, 16, "curr", channels_last=True)
        hbuf = arena.empty(((T + 1) * B, C + pad, H, W), torch.int8, 16, "hist", channels_last=True).unflatten(0, (T + 1, B))
        obuf = arena.empty((B, (T + 1) * C + pad, H, W), torch.int8, 16, "out", channels_last=True)
        cd, hd, od = cbuf[:, off:off + C], hbuf[:, :, off:off + C], obuf[:, off:off + (T + 1) * C]
        cd.copy_(curr)
        hd.copy_(hist)
        md = arena.place(meta, 16, "meta")
        before = [t.clone() for t in (cbuf, hbuf, obuf)]
        res = bev_align_stack(cd, hd, md, T, out=od)
        assert res.data_ptr() == od.data_ptr() and res.dtype == torch.int8
        arena.check()
        assert torch.equal(cbuf, before[0]), "curr was written"
        outside = torch.ones(C + pad, dtype=torch.bool)
        outside[off:off + C] = False
        assert torch.equal(hbuf[:, :, outside], before[1][:, :, outside]), "hist: bytes outside the slice were written"
        others = [s for s in range(T + 1) if s != write_slot]
        assert torch.equal(hbuf[others], before[1][others]), "a ring slot other than write_slot changed"
        outside = torch.ones((T + 1) * C + pad, dtype=torch.bool)
        outside[off:off + (T + 1) * C] = False
        assert torch.equal(obuf[:, outside], before[2][:, outside]), "out: bytes outside the slice were written"
        results.append((od.cpu().contiguous(), hd.cpu().contiguous()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), "the poison shows"
    return results[0]


@functools.lru_cache(maxsize=None)
def features(shape, lo=-128):
    B, C, T = shape
    g = torch.Generator().manual_seed(29 + sum(shape))
    return (torch.randint(lo, 128, (B, C, H, W), generator=g, dtype=torch.int8),
            torch.randint(lo, 128, (T + 1, B, C, H, W), generator=g, dtype=torch.int8))


def pack(shape, tf, slots, valid, write_slot):
    from bevformer_tensorrt_amd.functions import pack_bev_align_meta
    B, C, T = shape
    return pack_bev_align_meta(torch.tensor(tf, dtype=torch.float32).view(B, T, 2, 3), slots, valid, write_slot)


def statement(curr, hist, meta, T):
    from bevformer_tensorrt_amd.functions import bev_align_stack_q_plain
    ring = hist.clone()
    return bev_align_stack_q_plain(curr, ring, meta, T), ring


@pytest.mark.parametrize("shape,sliced", CASES, ids=IDS)
def test_exact_on_the_quarter_pixel_lattice(shape, sliced):
    """Arbitrary int8 values, lattice positions (whole cells, one row of corners outside, quarter pixels, a quarter turn,
    the whole map outside): weights are multiples of 1 / 16, every product and sum is exact in fp32, so the bytes are
    the statement's, ties to even in both signs included.  One slice of the first call is invalid: a copy."""
    B, C, T = shape
    curr, hist = features(shape)
    tfs = [U.shift(3, -2), U.shift(-1, -1), U.shift(0.25, -1.75), U.rot90(H, W), U.shift(0.5, 0.5), U.shift(W + 5, 0)]
    ties = torch.zeros(2, dtype=torch.long)
    for start in range(0, len(tfs), B * T):
        tf = [[tfs[(start + b * T + t) % len(tfs)] for t in range(T)] for b in range(B)]
        write_slot = start % (T + 1)
        slots = [[(write_slot + 1 + (t + b) % T) % (T + 1) for t in range(T)] for b in range(B)]
        valid = [[not (start == 0 and b == B - 1 and t == T - 1 and B * T > 1) for t in range(T)] for b in range(B)]
        meta = pack(shape, tf, slots, valid, write_slot)
        want, ring = statement(curr, hist, meta, T)
        got, hist_after = run(shape, sliced, curr, hist, meta)
        assert torch.equal(got, want), (got.int() - want.int()).abs().max().item()
        assert torch.equal(hist_after, ring) and torch.equal(got[:, :C], curr) and torch.equal(hist_after[write_slot], curr)
        exact, _ = U.ref_align(curr, hist, tf, slots, valid)
        tie = (exact[:, C:] - exact[:, C:].floor()) == 0.5
        ties += torch.stack(((tie & (exact[:, C:] > 0)).sum(), (tie & (exact[:, C:] < 0)).sum()))
    assert bool((ties > 0).all()), ties


@pytest.mark.parametrize("shape", [(1, 16, 1), (2, 80, 2)], ids=["B1-C16-T1", "B2-C80-T2"])
def test_one_hot_source_byte(shape):
    """One non-zero byte per channel in one pixel of the past maps under a generic rotation: exactly the output pixels
    whose footprint holds it are non-zero, with the statement's rounded weights."""
    B, C, T = shape
    curr, _ = features(shape)
    hist = torch.zeros(T + 1, B, C, H, W, dtype=torch.int8)
    hist[1:, :, :, H // 2 - 1, W // 2 + 1] = (torch.arange(C) % 2 * 2 - 1).mul(127 - torch.arange(C) % 64).to(torch.int8).view(C)
    tf = [[U.rotation(H, W, 0.3, 0.4, -0.3)] * T] * B
    slots, valid = [[t + 1 for t in range(T)]] * B, [[True] * T] * B
    meta = pack(shape, tf, slots, valid, 0)
    got, _ = run(shape, False, curr, hist, meta)
    want = statement(curr, hist, meta, T)[0]
    lit = (got[:, C:2 * C] != 0).any(1)
    assert torch.equal(got, want) and 2 <= int(lit[0].sum()) <= 6


@pytest.mark.parametrize("shape,sliced", CASES, ids=IDS)
def test_general_transforms_within_the_derived_bound(shape, sliced):
    """Every byte: |got - exact| <= 0.5 + 8 * 2^-24 * sum_k w_k |p_k| (design/bevdet4d_int8.md section 4: the final
    rounding to an integer, and design/bevdet4d.md section 4's count of fp32 roundings in front of it).  Values within
    +-127, the int8 convention, so the clamp does not act."""
    B, C, T = shape
    curr, hist = features(shape, -127)
    tf = [[U.rotation(H, W, 0.11 + 0.07 * (b * T + t), 0.3 - 0.45 * t, -0.2 + 0.35 * b) for t in range(T)] for b in range(B)]
    slots, valid = [[t + 1 for t in range(T)]] * B, [[True] * T] * B
    exact, mag = U.ref_align(curr, hist, tf, slots, valid)
    got, hist_after = run(shape, sliced, curr, hist, pack(shape, tf, slots, valid, 0))
    err, bound = (got.double() - exact).abs(), 0.5 + 8 * 2.0 ** -24 * mag
    print(f"{shape}: max error {err.max().item():.6f}, max (error - bound) {(err - bound).max().item():.3e}, "
          f"inside {(mag[:, C:] > 0).double().mean().item():.2f}")
    assert bool((err <= bound).all())
    assert (mag[:, C:] > 0).double().mean().item() > 0.5
    assert torch.equal(got[:, :C], curr) and torch.equal(hist_after[0], curr)


SPECIAL = {"nan-a00": (float("nan"), 0), "inf-a11": (float("inf"), 4), "huge-a02": (1e30, 2), "huge-a12": (-3e38, 5),
           "inf-a02": (float("-inf"), 2), "invalid": None, "outside-the-ring": None}


@pytest.mark.parametrize("shape", [(2, 80, 2), (1, 272, 2)], ids=["B2-C80-T2", "B1-C272-T2"])
@pytest.mark.parametrize("case", list(SPECIAL))
def test_special_entries_of_slice_1_of_sample_0(case, shape):
    """A non-finite or huge transform entry, or a slot outside the ring (with write_slot outside it too:
    pack_bev_align_meta refuses both, so the words are written here): zeros, nothing read out of bounds, nothing kept for
    write_slot outside.  valid == 0: a byte copy of curr.  Everything else is the statement's, the guards intact."""
    B, C, T = shape
    curr, hist = features(shape)
    tf = [[list(U.shift(0.25, 1)) for _ in range(T)] for _ in range(B)]
    if SPECIAL[case]:
        tf[0][0][SPECIAL[case][1]] = SPECIAL[case][0]
    meta = pack(shape, tf, [[1, 2]] * B, [[case != "invalid", True]] * B, 0)
    if case == "outside-the-ring":
        meta[0], meta[4] = T + 1, -1
    got, hist_after = run(shape, True, curr, hist, meta)
    want, ring = statement(curr, hist, meta, T)
    assert torch.equal(got, want) and torch.equal(hist_after, ring) and torch.equal(got[:, :C], curr)
    assert bool(got[0, C:2 * C].any()) == (case == "invalid") == torch.equal(got[0, C:2 * C], curr[0])
    assert bool(got[0, 2 * C:].any()) and torch.equal(hist_after, hist) == (case == "outside-the-ring")


def test_graph_replay_with_meta_rewritten():
    """Captured once; slot order, validity, transforms and write_slot change between replays through the static meta
    buffer: every replay equals the eager call on the same ring, bit for bit."""
    from bevformer_tensorrt_amd.functions import bev_align_stack
    from bevformer_tensorrt_amd.graph_runner import capture
    shape = (2, 80, 2)
    B, C, T = shape
    curr, hist = features(shape)
    rot = [[U.rotation(H, W, 0.5 + t + b, 0.25, -0.5) for t in range(T)] for b in range(B)]
    metas = [pack(shape, rot, [1, 2], [1, 1], 0), pack(shape, [r[::-1] for r in rot], [2, 0], [1, 0], 1),
             pack(shape, rot, [[1, 0], [0, 1]], [[1, 1], [0, 1]], 2)]
    order = [0, 1, 2, 1, 0]

    def buffers():
        c = curr.cuda().contiguous(memory_format=torch.channels_last)
        h = hist.cuda().permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        return c, h, metas[0].cuda()
    c, h, m = buffers()
    eager = []
    bev_align_stack(c, h, m, T)                     # (the capture's warm-up calls, with the first meta, do the same)
    for i in order:
        m.copy_(metas[i])
        eager.append((bev_align_stack(c, h, m, T).clone(), h.clone()))
    c, h, m = buffers()
    graph, out = capture(lambda: bev_align_stack(c, h, m, T))
    for i, (want_out, want_hist) in zip(order, eager):
        m.copy_(metas[i])
        graph.replay()
        assert torch.equal(out, want_out) and torch.equal(h, want_hist), i
    assert not torch.equal(eager[0][0], eager[1][0])
