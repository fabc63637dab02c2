"""CPU-only: every status of bevops_bev_align_stack_f16 in the documented order (the entry answers before any device
call), the torch statement `bev_align_stack_plain` against the float64 statement of tests/util_bev_align.py, the host
side `bev_align_transform` and the meta buffer's round trip."""
import ctypes

import pytest
import torch

import util_bev_align as U


def test_every_status_in_the_documented_order():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(**kw):
        a = dict(dtype=1, curr=p, cp=8, hist=p, hp=8, out=p, op=16, meta=p, B=0, H=2, W=3, C=8, T=1)
        a.update(kw)
        return lib.bevops_bev_align_stack_f16(a["dtype"], a["curr"], a["cp"], a["hist"], a["hp"], a["out"], a["op"], a["meta"],
                                              a["B"], a["H"], a["W"], a["C"], a["T"], None)

    assert call() == 0                                                        # B == 0: success without a launch
    for bad in (dict(curr=None), dict(hist=None), dict(out=None), dict(meta=None), dict(B=-1), dict(H=0), dict(W=-2),
                dict(C=0), dict(T=0), dict(cp=0), dict(hp=4), dict(op=8), dict(T=2, op=16), dict(cp=12), dict(hp=20),
                dict(op=20), dict(curr=p + 8), dict(hist=p + 2), dict(out=p + 8), dict(meta=p + 4)):
        assert call(**bad) == 2, bad
    for unsupported in (dict(dtype=0), dict(dtype=2), dict(C=12, cp=16, hp=16, op=24), dict(T=16, op=136), dict(H=0x10000),
                        dict(W=0x10000), dict(B=1 << 9, H=1 << 9, W=1 << 9),                 # curr reaches 2^31 bytes
                        dict(B=1 << 8, H=1 << 9, W=1 << 9),                                  # curr does not; the ring and out do
                        dict(B=1 << 10, H=1 << 9, W=1 << 9, T=3, op=32)):
        assert call(**unsupported) == 3, unsupported
    assert call(B=1 << 10, H=1 << 9, W=1 << 9, T=15, op=128) == 3 and call(B=1, dtype=0) == 3   # with B > 0 too, no launch
    # the order: BAD_PARAM wins over NOT_SUPPORTED, a pitch below the channels over its alignment
    assert call(dtype=0, curr=None) == 2 and call(C=12, cp=16, hp=16, op=24, meta=p + 4) == 2
    assert call(T=16, op=128) == 2 and call(C=12, cp=8) == 2 and call(H=0x10000, out=p + 8) == 2
    assert lib.bevops_query(b"bevops_bev_align_stack_f16")


def _exact_case():
    B, H, W, C, T = 2, 6, 9, 8, 2
    g = torch.Generator().manual_seed(3)
    curr, hist = U.dyadic((B, C, H, W), g), U.dyadic((T + 1, B, C, H, W), g)
    tf = [[U.shift(1, -1), U.shift(0.25, -1.75)], [U.rot90(H, W), U.shift(W + 5, 0)]]
    return curr, hist, tf, [[0, 1]] * B, [[True, True], [True, False]], 2


def test_plain_statement_against_the_float64_statement():
    """F.grid_sample normalises the positions and un-normalises them again: they come back within 4 ulps of W (2^-19
    here), and a bilinear sample of features below 4 moves by at most 2 * 4 * that per axis."""
    from bevformer_tensorrt_amd.functions import bev_align_stack, pack_bev_align_meta
    curr, hist, tf, slots, valid, write_slot = _exact_case()
    want, _ = U.ref_align(curr, hist, tf, slots, valid)
    ring = hist.clone()
    got = bev_align_stack(curr, ring, pack_bev_align_meta(torch.tensor(tf).view(2, 2, 2, 3), slots, valid, write_slot), 2)
    err = (got.double() - want).abs().max().item()
    print(f"plain statement vs float64: {err:.3e}")
    assert got.shape == want.shape and err <= 16 * 2.0 ** -19
    assert torch.equal(got[:, :8], curr) and torch.equal(got[1, 16:], curr[1]) and torch.equal(ring[2], curr)
    assert torch.equal(ring[:2], hist[:2]) and bool(got[0, 8:].any())


def test_transform_identity_translation_and_composition():
    from bevformer_tensorrt_amd.functions import bev_align_transform
    lower, interval = [-51.2, -51.2, -5.0], [0.8, 0.8, 8.0]
    g = torch.Generator().manual_seed(0)
    s2e = torch.eye(4).repeat(2, 6, 1, 1)
    s2e[..., :3, 3] = torch.randn(2, 6, 3, generator=g)
    bda = torch.eye(3).repeat(2, 1, 1)

    def pose(yaw, x, y):
        m = torch.eye(4)
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = torch.cos(yaw), -torch.sin(yaw), torch.sin(yaw), torch.cos(yaw)
        m[0, 3], m[1, 3] = x, y
        return m.repeat(2, 6, 1, 1)
    p0, p1, p2 = pose(torch.tensor(0.1), 3.0, -2.0), pose(torch.tensor(0.16), 4.1, -1.7), pose(torch.tensor(0.2), 5.3, -1.2)
    ident = bev_align_transform(s2e, p1, s2e, p1, bda, lower, interval)
    assert ident.shape == (2, 2, 3) and ident.dtype == torch.float32
    assert (ident - torch.eye(3)[:2]).abs().max() <= 1e-4          # (an offset of 64 cells goes through two inversions)
    # the ego drives k cells forward (+x) between the past and the current frame: a static place lies k cells further
    # ahead in the past frame's map, so the current pixel x reads the past pixel x + k
    still, ahead = torch.eye(4).repeat(2, 6, 1, 1), torch.eye(4).repeat(2, 6, 1, 1)
    ahead[..., 0, 3] = 3 * 0.8
    tf = bev_align_transform(s2e, ahead, s2e, still, bda, lower, interval)
    want = torch.tensor([[1.0, 0.0, 3.0], [0.0, 1.0, 0.0]])
    assert (tf - want).abs().max() <= 1e-4 and (bev_align_transform(s2e, still, s2e, ahead, bda, lower, interval)[:, 0, 2]
                                                + 3).abs().max() <= 1e-4

    def full(a):
        return torch.cat([a, torch.tensor([0.0, 0.0, 1.0]).expand(a.shape[0], 1, 3)], 1)
    a21, a10 = bev_align_transform(s2e, p2, s2e, p1, bda, lower, interval), bev_align_transform(s2e, p1, s2e, p0, bda, lower, interval)
    a20 = bev_align_transform(s2e, p2, s2e, p0, bda, lower, interval)
    # current -> frame 1 -> frame 0 equals current -> frame 0: entries of size <= 128 cells, a few dozen fp32 roundings each
    assert (full(a10).matmul(full(a21))[:, :2] - a20).abs().max() <= 64 * 128 * 2.0 ** -24


def test_meta_round_trip_and_checks():
    from bevformer_tensorrt_amd.functions import bev_align_meta_words, pack_bev_align_meta, unpack_bev_align_meta
    tf = torch.randn(3, 2, 2, 3)
    tf[0, 0, 0, 0] = float("nan")
    meta = pack_bev_align_meta(tf, [[1, 2], [2, 1], [1, 1]], [[1, 0], [1, 1], [0, 0]], 0)
    assert meta.dtype == torch.int32 and meta.numel() == bev_align_meta_words(3, 2) == 52 and meta[:4].tolist() == [0, 0, 0, 0]
    assert meta[4:12].tolist()[:2] == [1, 1] and meta[12:14].tolist() == [2, 0]
    ws, slots, valid, back = unpack_bev_align_meta(meta, 3, 2)
    assert ws == 0 and slots.tolist() == [[1, 2], [2, 1], [1, 1]] and valid.tolist() == [[True, False], [True, True], [False, False]]
    assert torch.equal(back.view(torch.int32), tf.view(torch.int32))
    for kw in (dict(write_slot=3), dict(slots=[1, 3]), dict(slots=[0, 1], valid=[1, 1]), dict(write_slot=-1)):
        a = dict(transforms=tf, slots=[1, 2], valid=[1, 0], write_slot=0)
        a.update(kw)
        with pytest.raises(ValueError):
            pack_bev_align_meta(**a)
