"""The numpy statements and C-ABI calls of bevops_se_gate2_nhwc_s8 and bevops_global_avgpool_nhwc_s8
(csrc/lss_depthnet_s8.hip) for tests/test_lss_depthnet_s8_cpu.py and tests/test_lss_depthnet_s8_gpu.py.

Both operation orders consist of single fp32 operations without an addition (include/bevops.h), so numpy's float32
arithmetic restates them bit for bit:

    gate:  t = f32(q) * scale_x;  v = t * gate;  r = v * inv_out (inv_out = 1.f / scale_out);  clamp(rne(r), -127, 127),
           a NaN r -> -127
    pool:  fp16((f32(sum) * scale_x) / f32(hw)),  sum the exact integer sum"""
import numpy as np

F32 = np.float32


def gate_statement(x_q, scale_x, gate, scale_out):
    """x_q int8 [n, hw, c], gate fp32 [n, c] -> int8 [n, hw, c]."""
    with np.errstate(all="ignore"):
        t = x_q.astype(F32) * F32(scale_x)
        v = t * gate.astype(F32)[:, None, :]
        r = v * (F32(1.0) / F32(scale_out))
        assert t.dtype == v.dtype == r.dtype == F32
        q = np.clip(np.rint(r), -127, 127)
    return np.where(np.isnan(r), F32(-127), q).astype(np.int8)          # max(NaN, -127) = -127


def pool_statement(x_q, scale_x):
    """x_q int8 [n, hw, c] -> fp16 [n, c]."""
    s = x_q.astype(np.int64).sum(axis=1)
    assert np.abs(s).max() < 2 ** 31
    with np.errstate(over="ignore"):
        prod = s.astype(F32) * F32(scale_x)
        return (prod / F32(x_q.shape[1])).astype(np.float16)


def handmade_gate_case():
    """-> (x_q [2, 4, 16], scale_x, gates [2, 2, 16], scale_a, scale_b, want_a, want_b) with ties, saturation, NaN and
    inf written out by hand.  scale_x 0.5, scale_a 1: r = q / 2 * gate."""
    x = np.zeros((2, 4, 16), np.int8)
    x[0, 0] = [1, 3, 5, 7, -1, -3, -5, -7, 2, 4, 127, -127, 0, 126, -128, 100]
    x[0, 1] = x[0, 0][::-1]
    x[1, 2] = [1, 1, 0, 127, -127, 3, -3, 5, 1, 1, 1, 1, 0, 0, 0, 0]
    g = np.ones((2, 2, 16), F32)
    g[0, 1, :4] = [np.nan, np.inf, -np.inf, 4.0]          # image 1, depth branch: NaN, +-inf and a large gate
    g[0, 1, 4:8] = [4.0, 0.0, 1.0, 1.0]
    g[1] = 0.5                                            # context branch: r = q / 4 with scale_b 1 ...
    want_a = np.zeros_like(x)
    # image 0, gate 1: q / 2 rounded to even -- 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    want_a[0, 0] = [0, 2, 2, 4, 0, -2, -2, -4, 1, 2, 64, -64, 0, 63, -64, 50]
    want_a[0, 1] = want_a[0, 0][::-1]
    # image 1: NaN -> -127; 0.5 * inf = inf -> 127; 0 * -inf = NaN -> -127; 63.5 * 4 -> 127; -63.5 * 4 -> -127;
    # 1.5 * 0 = 0; -1.5 -> -2; 2.5 -> 2; then 0.5 -> 0 four times
    want_a[1, 2] = [-127, 127, -127, 127, -127, 0, -2, 2, 0, 0, 0, 0, 0, 0, 0, 0]
    want_a[1, [0, 1, 3], 0] = -127                        # a NaN gate spoils its channel at every pixel of its image
    want_a[1, [0, 1, 3], 1:3] = -127                      # 0 * inf = NaN as well
    # context: scale_b 0.125 -> r = q / 2 * 0.5 * 8 = 2 q, saturating at |q| >= 64
    want_b = np.clip(2 * x.astype(np.int32), -127, 127).astype(np.int8)
    return x, 0.5, g, 1.0, 0.125, want_a, want_b


def handmade_pool_case():
    """-> (x_q [1, 32, 16], scale_x, want fp16 [1, 16]): hw = 32 and scale_x = 32, so out = fp16(sum): 12-bit sums are
    exact binary16 ties (2049 -> 2048, 2051 -> 2052), 127 * 32 = 4064 is exact."""
    x = np.zeros((1, 32, 16), np.int8)
    def fill(ch, total):
        sign = 1 if total >= 0 else -1
        left = abs(total)
        for p in range(32):
            take = min(127, left)
            x[0, p, ch] = sign * take
            left -= take
        assert left == 0
    sums = [2049, 2051, -2049, -2051, 4064, -4064, 0, 1, 2053, 2055, 4063, 4061, -1, 100, 2047, 3000]
    for ch, s in enumerate(sums):
        fill(ch, s)
    want = np.array([[2048, 2052, -2048, -2052, 4064, -4064, 0, 1, 2052, 2056, 4064, 4060, -1, 100, 2047, 3000]], np.float16)
    return x, 32.0, want


def _lib():
    import torch
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _place(arena, values, pitch, c0, name):
    import torch
    n, hw, c = values.shape
    buf = arena.empty((n, hw, pitch), torch.int8, 16, name)
    buf[..., c0:c0 + c].copy_(torch.from_numpy(np.array(values)))
    return buf, buf[..., c0:c0 + c]


def _outside_unchanged(buf_before, buf_after, c0, c):
    mask = np.zeros(buf_after.shape, bool)
    mask[..., c0:c0 + c] = True
    m8 = np.repeat(mask, buf_after.itemsize, axis=-1)
    assert np.array_equal(buf_after.view(np.uint8)[~m8], buf_before.view(np.uint8)[~m8]), \
        "bytes of the output buffer outside the slice were written"


def gate_call(arena, x_q, scale_x, gates, scale_a, scale_b, pitched):
    """-> (out_a, out_b) int8 [n, hw, c]; pitched: x, out_a and out_b are slices of wider buffers."""
    import torch
    L, h, st = _lib()
    n, hw, c = x_q.shape
    (xp, xc0), (ap, ac0), (bp, bc0) = ((c + 48, 16), (c + 32, 16), (2 * c, c)) if pitched else ((c, 0), (c, 0), (c, 0))
    _, xv = _place(arena, x_q, xp, xc0, "x")
    gd = arena.place(torch.from_numpy(np.array(gates, dtype=np.float32)), 16, "gates")
    abuf = arena.empty((n, hw, ap), torch.int8, 16, "out_a")
    bbuf = arena.empty((n, hw, bp), torch.int8, 16, "out_b")
    av, bv = abuf[..., ac0:ac0 + c], bbuf[..., bc0:bc0 + c]
    before = abuf.cpu().numpy().copy(), bbuf.cpu().numpy().copy()
    rc = h.bevops_se_gate2_nhwc_s8(xv.data_ptr(), xp, scale_x, gd.data_ptr(), av.data_ptr(), ap, scale_a, bv.data_ptr(), bp,
                                   scale_b, n, hw, c, st)
    assert rc == L.SUCCESS, rc
    arena.check()
    after = abuf.cpu().numpy(), bbuf.cpu().numpy()
    _outside_unchanged(before[0], after[0], ac0, c)
    _outside_unchanged(before[1], after[1], bc0, c)
    return after[0][..., ac0:ac0 + c].copy(), after[1][..., bc0:bc0 + c].copy()


def pool_call(arena, x_q, scale_x, pitched):
    """-> fp16 [n, c]; pitched: x is a slice of a wider buffer and out rows are wider than c."""
    import torch
    L, h, st = _lib()
    n, hw, c = x_q.shape
    (xp, xc0), op = ((c + 48, 16), c + 3) if pitched else ((c, 0), c)
    _, xv = _place(arena, x_q, xp, xc0, "x")
    obuf = arena.empty((n, op), torch.float16, 2, "out")
    before = obuf.cpu().numpy().copy()
    rc = h.bevops_global_avgpool_nhwc_s8(xv.data_ptr(), xp, scale_x, obuf.data_ptr(), op, n, hw, c, st)
    assert rc == L.SUCCESS, rc
    arena.check()
    after = obuf.cpu().numpy()
    _outside_unchanged(before, after, 0, c)
    return after[:, :c].copy()
