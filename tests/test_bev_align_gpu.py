"""bevops_bev_align_stack_f16 (csrc/bev_align.hip) through functions.bev_align_stack in the guarded arena of
tests/util_arena.py, against the float64 statement of tests/util_bev_align.py on the SAME fp32 positions.  Every shape
runs with contiguous operands and with curr, hist and out as interior channel slices of wider buffers; every byte of
those buffers outside the slices, and every ring slot but write_slot, is compared with what it held before.

The kernel's pixel tile is 8 x 8 (a wave owns two tile rows) and a lane owns one 8-channel vector: (1, 5, 7, 8, 1) lies
inside one tile with one vector per pixel, (2, 16, 16, 80, 2) is four full tiles of ten vectors, (1, 9, 33, 88, 3) has
eleven vectors and ragged tiles on both axes; (1, 3, 9, 136, 1) takes the kernel that does not keep curr in registers
(more than four passes: C > 128)."""
import functools

import pytest
import torch

import util_bev_align as U
from util_arena import Arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7, 8, 1), (2, 16, 16, 80, 2), (1, 9, 33, 88, 3), (1, 3, 9, 136, 1)]      # (B, H, W, C, T)
CASES = [(s, sliced) for s in SHAPES for sliced in (False, True)]
IDS = ["x".join(map(str, s)) + ("-sliced" if sl else "") for s, sl in CASES]
CAPACITY = 16 << 20
POISON = 0x55


def run(shape, sliced, curr, hist, tf, slots, valid, write_slot, meta=None):
    """One call on arena buffers -> (out [B, (T + 1) C, H, W], hist after [S, B, C, H, W]) fp16 on the CPU, with the bytes
    the call must not touch checked."""
    from bevformer_tensorrt_amd.functions import bev_align_stack, pack_bev_align_meta
    B, H, W, C, T = shape
    pad, off = (24, 8) if sliced else (0, 0)
    arena = Arena(CAPACITY, POISON)
    cbuf = arena.empty((B, C + pad, H, W), torch.float16, 16, "curr", channels_last=True)
    hbuf = arena.empty(((T + 1) * B, C + pad, H, W), torch.float16, 16, "hist", channels_last=True).unflatten(0, (T + 1, B))
    obuf = arena.empty((B, (T + 1) * C + pad, H, W), torch.float16, 16, "out", channels_last=True)
    cd, hd, od = cbuf[:, off:off + C], hbuf[:, :, off:off + C], obuf[:, off:off + (T + 1) * C]
    cd.copy_(curr.half())
    hd.copy_(hist.half())
    if meta is None:
        meta = pack_bev_align_meta(torch.tensor(tf, dtype=torch.float32).view(B, T, 2, 3), slots, valid, write_slot)
    md = arena.place(meta, 16, "meta")
    before = [t.clone().view(torch.int16) for t in (cbuf, hbuf, obuf)]
    res = bev_align_stack(cd, hd, md, T, out=od)
    assert res.data_ptr() == od.data_ptr()
    arena.check()
    c1, h1, o1 = (t.view(torch.int16) for t in (cbuf, hbuf, obuf))
    assert torch.equal(c1, before[0]), "curr was written"
    outside = torch.ones(C + pad, dtype=torch.bool)
    outside[off:off + C] = False
    assert torch.equal(h1[:, :, outside], before[1][:, :, outside]), "hist: bytes outside the slice were written"
    others = [s for s in range(T + 1) if s != write_slot]
    assert torch.equal(h1[others], before[1][others]), "a ring slot other than write_slot changed"
    outside = torch.ones((T + 1) * C + pad, dtype=torch.bool)
    outside[off:off + (T + 1) * C] = False
    assert torch.equal(o1[:, outside], before[2][:, outside]), "out: bytes outside the slice were written"
    return od.cpu().contiguous(), hd.cpu().contiguous()


def bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def features(shape, kind):
    B, H, W, C, T = shape
    g = torch.Generator().manual_seed(17 + sum(shape))
    make = (lambda s: U.dyadic(s, g)) if kind == "dyadic" else (lambda s: torch.randn(s, generator=g).half().float())
    return make((B, C, H, W)), make((T + 1, B, C, H, W))


def exact_transforms(H, W):
    """The quarter-pixel lattice: identity; shifts by one pixel either way (positions exactly at -1, 0, W - 1 and W, the
    same in y); an integer and a quarter-pixel shift; a quarter turn about the centre; the whole map outside."""
    return [U.shift(0, 0), U.shift(-1, -1), U.shift(1, 1), U.shift(3, -2), U.shift(0.25, -1.75), U.rot90(H, W),
            U.shift(W + 5, 0)]


def check_exact(got, hist_after, curr, want, write_slot):
    C = curr.shape[1]
    assert torch.equal(bits(got), bits(want.half())), (got.float() - want.float()).abs().max().item()
    assert torch.equal(bits(got[:, :C]), bits(curr.half())) and torch.equal(bits(hist_after[write_slot]), bits(curr.half()))


@pytest.mark.parametrize("shape,sliced", CASES, ids=IDS)
def test_exact_on_the_quarter_pixel_lattice(shape, sliced):
    """Dyadic features, lattice positions: every product and sum is exact in fp32, so the output is the float64 result
    rounded once -- slice 0 and hist[write_slot] bit copies of curr; one slice of each call is invalid (a copy)."""
    B, H, W, C, T = shape
    curr, hist = features(shape, "dyadic")
    tfs = exact_transforms(H, W)
    for start in range(0, len(tfs), B * T):
        tf = [[tfs[(start + b * T + t) % len(tfs)] for t in range(T)] for b in range(B)]
        write_slot = start % (T + 1)
        slots = [[(write_slot + 1 + (t + b) % T) % (T + 1) for t in range(T)] for b in range(B)]
        valid = [[not (start == 0 and b == B - 1 and t == T - 1 and B * T > 1) for t in range(T)] for b in range(B)]
        want, _ = U.ref_align(curr, hist, tf, slots, valid)
        got, hist_after = run(shape, sliced, curr, hist, tf, slots, valid, write_slot)
        check_exact(got, hist_after, curr, want, write_slot)
        if not valid[B - 1][T - 1]:
            assert torch.equal(bits(got[B - 1, T * C:]), bits(curr[B - 1].half()))


@pytest.mark.parametrize("shape,sliced", CASES, ids=IDS)
def test_gaussian_features_generic_rotations(shape, sliced):
    B, H, W, C, T = shape
    curr, hist = features(shape, "gauss")
    tf = [[U.rotation(H, W, 0.37 + 0.9 * (b * T + t), 0.3 - 0.45 * t, -0.2 + 0.35 * b) for t in range(T)] for b in range(B)]
    slots = [[t + 1 for t in range(T)]] * B
    valid = [[True] * T] * B
    want, mag = U.ref_align(curr, hist, tf, slots, valid)
    got, hist_after = run(shape, sliced, curr, hist, tf, slots, valid, 0)
    err, bound = (got.double() - want).abs(), U.general_bound(want, mag)
    print(f"{shape}: max error {err.max().item():.3e}, max (error - bound) {(err - bound).max().item():.3e}, "
          f"inside {(mag[:, C:] > 0).double().mean().item():.2f}")
    assert bool((err <= bound).all())
    assert (mag[:, C:] > 0).double().mean().item() > 0.3              # the rotations keep a good part of the map inside
    assert torch.equal(bits(got[:, :C]), bits(curr.half())) and torch.equal(bits(hist_after[0]), bits(curr.half()))


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[0:6:2])
def test_one_hot_source_pixel(shape):
    """One non-zero source pixel under a generic rotation: exactly the output pixels whose footprint holds it are
    non-zero (the lattice points inside a turned 2 x 2 square: a handful), with the statement's weights -- a wrong
    corner or a swapped axis moves or reweighs them."""
    B, H, W, C, T = shape
    curr, hist = features(shape, "dyadic")
    hist = torch.zeros_like(hist)
    hist[1:, :, :, H // 2 - 1, W // 2 + 1] = 1.0 + torch.arange(C).float() / 8
    tf = [[U.rotation(H, W, 0.3, 0.4, -0.3)] * T] * B
    slots, valid = [[t + 1 for t in range(T)]] * B, [[True] * T] * B
    want, mag = U.ref_align(curr, hist, tf, slots, valid)
    got, _ = run(shape, False, curr, hist, tf, slots, valid, 0)
    assert bool(((got.double() - want).abs() <= U.general_bound(want, mag)).all())
    lit = (got[:, C:2 * C] != 0).any(1)
    assert torch.equal(lit, (want[:, C:2 * C] != 0).any(1)) and 2 <= int(lit[0].sum()) <= 6


@pytest.mark.parametrize("bad", [(float("nan"), 0), (float("inf"), 4), (1e30, 2), (-3e38, 5), (float("-inf"), 2)],
                         ids=["nan-a00", "inf-a11", "huge-a02", "huge-a12", "inf-a02"])
def test_non_finite_and_huge_entries_give_zeros(bad):
    """Slice 1 of sample 0 carries the entry: all zeros there; every other slice is what the statement gives."""
    shape = SHAPES[1]
    B, H, W, C, T = shape
    curr, hist = features(shape, "dyadic")
    tf = [[list(U.shift(0.25, 1)) for _ in range(T)] for _ in range(B)]
    tf[0][0][bad[1]] = bad[0]
    slots, valid = [[1, 2]] * B, [[True] * T] * B
    want, _ = U.ref_align(curr, hist, tf, slots, valid)
    got, hist_after = run(shape, True, curr, hist, tf, slots, valid, 0)
    assert not bool(got[0, C:2 * C].any()) and not bool(want[0, C:2 * C].any())
    check_exact(got, hist_after, curr, want, 0)


def test_graph_replay_with_meta_rewritten():
    """Captured once; slot order, validity, transforms and write_slot change between replays through the static meta
    buffer: every replay equals the eager call on the same ring, bit for bit."""
    from bevformer_tensorrt_amd.functions import bev_align_stack, pack_bev_align_meta
    from bevformer_tensorrt_amd.graph_runner import capture
    shape = SHAPES[1]
    B, H, W, C, T = shape
    curr, hist = features(shape, "gauss")
    rot = [[U.rotation(H, W, 0.5 + t + b, 0.25, -0.5) for t in range(T)] for b in range(B)]
    metas = [pack_bev_align_meta(torch.tensor(rot).view(B, T, 2, 3), [1, 2], [1, 1], 0),
             pack_bev_align_meta(torch.tensor(rot).flip(1).view(B, T, 2, 3), [2, 0], [1, 0], 1),
             pack_bev_align_meta(torch.tensor(rot).view(B, T, 2, 3), [[1, 0], [0, 1]], [[1, 1], [0, 1]], 2)]
    order = [0, 1, 2, 1, 0]

    def buffers():
        c = curr.half().cuda().contiguous(memory_format=torch.channels_last)
        h = hist.half().cuda().permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
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
        assert torch.equal(bits(out), bits(want_out)) and torch.equal(bits(h), bits(want_hist)), i
    assert not torch.equal(bits(eager[0][0]), bits(eager[1][0]))
