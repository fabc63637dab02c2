"""The cases, statements and the C-ABI call of bevops_conv_slice_s8_ex2's dilation and per-image bias
(tests/test_conv_slice_s8_ex2_cpu.py, tests/test_conv_slice_s8_ex2_gpu.py):

    sum = sum_{ky,kx,ci} x_q[b, y + (ky - 1) d, x + (kx - 1) d, ci] w_q[co, ky, kx, ci]       zero outside the image
    v = fma(f32(sum), sc, bias[co]  or  f32(image_bias[b][co]));  then bevops_conv_slice_s8_ex's epilogue

`sums_dilated` is a shift-and-add in int64 (no library convolution; the CPU test compares it with a float64
F.conv2d(dilation=)).  The lattice of tests/test_conv_slice_s8_gpu.py (scale_a 2^-5, per-channel power-of-two weight
scales, bias and image bias integers * 2^-4, scale_res 2^-5, scale_out a power of two) makes every step an fp32 number,
asserted, so the statement is exact whatever gets contracted."""
import functools

import numpy as np

import util_conv_slice_s8 as S
import util_exact_dense as X

NONE, RELU, SILU = 0, 1, 2
S_A, S_RES = 2.0 ** -5, 2.0 ** -5

# (B, H, W, Cin, Cout, dilation, layout)
#  * (1, 5, 7) 32 -> 16 at dilation 6: every tap with ky != 1 is outside, in columns 1 .. 5 every off-centre tap is;
#    Cin 32 puts two taps into one 64-byte step, so the threads of one step hold different taps
#  * (3, 5, 7) 96 -> 48 at dilation 2: 105 rows of three images in ONE row tile (the per-image bias), K = 864 = 13.5 steps
#  * (2, 16, 44) 64 -> 144 at dilation 6 / 12 / 18: the R50 map; tile 5 crosses the image boundary at row 704; two
#    column tiles, one with a tail
#  * 'slice4': x is slice 2 of a 4-slice buffer, out slice 1 of another (the ASPP buffer's layout)
LATTICE_CASES = ((1, 5, 7, 32, 16, 6, "dense"), (3, 5, 7, 96, 48, 2, "slice"), (2, 16, 44, 64, 144, 6, "slice4"),
                 (2, 16, 44, 64, 144, 12, "dense"), (2, 16, 44, 64, 144, 18, "slice"), (3, 5, 7, 96, 48, 2, "slice4"))


def sums_dilated(x_q, w_q, d):
    """int64 sums [B, H, W, Cout] of int8 x [B, H, W, Cin] and w [Cout, 3, 3, Cin] at dilation d, stride 1, pad d."""
    B, H, W, Cin = x_q.shape
    Cout = w_q.shape[0]
    assert w_q.shape[1:] == (3, 3, Cin)
    x = x_q.astype(np.int64)
    acc = np.zeros((B, H, W, Cout), np.int64)
    for ky in range(3):
        for kx in range(3):
            dy, dx = (ky - 1) * d, (kx - 1) * d
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 >= y1 or x0 >= x1:
                continue                              # the tap reads outside the image everywhere
            acc[:, y0:y1, x0:x1] += x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx] @ w_q[:, ky, kx].astype(np.int64).T
    return acc


def gen_image_bias(r, B, Cout):
    """fp16 [B, Cout] on the lattice (integers * 2^-4), every image and channel its own draw."""
    v = (r.integers(-64, 65, size=(B, Cout)) * 2.0 ** -4).astype(np.float16)
    assert len({v[b].tobytes() for b in range(B)}) == B
    return v


@functools.lru_cache(maxsize=None)
def operands(case):
    B, H, W, Cin, Cout, d, _ = case
    r = X._rng("conv_slice_s8_ex2", case)
    x = X.gen_int8(r, (B, H, W, Cin))
    w, ws = X.gen_weights_int8(r, Cout, 9 * Cin, True)
    w = w.reshape(Cout, 3, 3, Cin)
    bias = X.gen_bias(r, Cout, "s8")
    ibias = gen_image_bias(r, B, Cout)
    res = X.gen_identity(r, (B, H, W, Cout), "s8", "int8")
    acc = sums_dilated(x, w, d)
    for a in (x, w, ws, bias, ibias, res, acc):
        a.setflags(write=False)
    return x, w, ws, bias, ibias, res, acc


def lattice_statement(case, epi, act, out, res_first=False, with_res=False):
    """epi 'bias' | 'image' -> (want, scale_out, t): every step asserted to be an fp32 number."""
    x, w, ws, bias, ibias, res, acc = operands(case)
    v = X.f32_exact(X.f32_exact(acc.astype(np.float64), "(float)sum") * (S_A * ws.astype(np.float64)), "* scale")
    b = bias.astype(np.float64) if epi == "bias" else ibias.astype(np.float64)[:, None, None, :]
    v = X.f32_exact(v + b, "+ bias")
    if with_res and res_first:
        v = X.f32_exact(v + res.astype(np.float64) * S_RES, "+ identity in front")
    if act == RELU:
        v = np.maximum(v, 0.0)
    if with_res and not res_first:
        v = X.f32_exact(v + res.astype(np.float64) * S_RES, "+ identity behind")
    if out == "fp16":
        return v.astype(np.float32).astype(np.float16), 1.0, None
    s_out = 2.0 ** int(np.floor(np.log2(v.std() / 48.0)))
    t = X.f32_exact(v / s_out, "/ scale_out")
    return np.clip(np.rint(t), -127, 127).astype(np.int8), s_out, t


def order_statement(acc, scale_a, w_scales, bias, ibias, act, res_q, scale_res, res_first, scale_out, out):
    """The fp32 operation order of include/bevops.h (act none / ReLU), each fma in the extended type and rounded once."""
    s_aw, inv = S.host_scalars(scale_a, 1.0, scale_out if out == "int8" else None)
    N = acc.shape[-1]
    sc = (s_aw * S.f32(w_scales)).astype(np.float32) if w_scales is not None else np.full(N, s_aw, np.float32)
    if ibias is not None:
        b = ibias.astype(np.float32)[:, None, None, :]
    else:
        b = S.f32(bias) if bias is not None else np.zeros(N, np.float32)
    v = S._fma32(acc.astype(np.float32), np.broadcast_to(sc, acc.shape), np.broadcast_to(b, acc.shape))
    r = None if res_q is None else (res_q.astype(np.float32), np.full(acc.shape, np.float32(scale_res), np.float32))
    if r is not None and res_first:
        v = S._fma32(r[0], r[1], v)
    if act == RELU:
        v = np.maximum(v, np.float32(0))
    if r is not None and not res_first:
        v = S._fma32(r[0], r[1], v)
    if out == "fp16":
        return v.astype(np.float16)
    return np.clip(np.rint((v * inv).astype(np.float32)), -127, 127).astype(np.int8)


def place_slice(arena, values, pitch, c0, name):
    import torch
    B, H, W, C = values.shape
    t = torch.from_numpy(np.array(values))
    buf = arena.empty((B, H, W, pitch), t.dtype, 16, name)
    view = buf[..., c0:c0 + C]
    view.copy_(t)
    return buf, view


def c_call_ex2(arena, x, w, ws, bias, res, act, layout, out, res_first, dilation, ibias, scale_a=S_A, scale_res=S_RES,
               scale_out=1.0, ibias_pad=8, entry="ex2"):
    """One call of bevops_conv_slice_s8_ex2 (3 x 3 or 1 x 1, stride 1) with every operand carved from `arena` -> the
    output slice [B, H, W, Cout]; every byte of the output buffer outside the slice is compared.  entry='ex': the same
    operands through bevops_conv_slice_s8_ex (dilation 1, no image bias)."""
    import torch
    from bevformer_tensorrt_amd.utils import lib as L
    h, st = L.load_library(), L.current_stream_ptr(torch.device("cuda"))
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    odt = torch.int8 if out == "int8" else torch.float16
    wd = arena.place(torch.from_numpy(np.array(w)), 16, "weight")
    wsd = None if ws is None else arena.place(torch.from_numpy(np.array(ws, dtype=np.float32)), 4, "w_scales")
    bd = None if bias is None else arena.place(torch.from_numpy(np.array(bias, dtype=np.float32)), 4, "bias")
    ovec = 16 if out == "int8" else 8
    if layout == "dense":
        (xp, xc0), (op, oc0) = (Cin, 0), (Cout, 0)
    elif layout == "slice":
        (xp, xc0), (op, oc0) = (Cin + 48, 16), (Cout + 2 * ovec, ovec)
    else:
        assert layout == "slice4" and Cout % ovec == 0
        (xp, xc0), (op, oc0) = (4 * Cin, 2 * Cin), (4 * Cout, Cout)
    _, xv = place_slice(arena, x, xp, xc0, "x")
    obuf = arena.empty((B, H, W, op), odt, 16, "out")
    ov = obuf[..., oc0:oc0 + Cout]
    rv, rp = None, 0
    if res is not None:
        rp = (Cout if layout == "dense" else Cout + 16) + 15 & ~15
        _, rv = place_slice(arena, res, rp, 0, "identity")
    ib, ibp = None, 0
    if ibias is not None:
        ibp = Cout + ibias_pad
        ib = arena.empty((B, ibp), torch.float16, 16, "image_bias")      # the pad columns keep the poison
        ib[:, :Cout].copy_(torch.from_numpy(np.array(ibias)))
    before = obuf.cpu().numpy().view(np.uint8).copy()
    head = (xv.data_ptr(), xp, scale_a, wd.data_ptr(), None if wsd is None else wsd.data_ptr(), 1.0,
            None if bd is None else bd.data_ptr(), None if rv is None else rv.data_ptr(), rp, scale_res,
            L.I8 if out == "int8" else L.F16, ov.data_ptr(), op, scale_out, B, H, W, Cin, Cout, k, 1, act, int(res_first))
    if entry == "ex":
        assert dilation == 1 and ibias is None
        rc = h.bevops_conv_slice_s8_ex(*head, st)
    else:
        rc = h.bevops_conv_slice_s8_ex2(*head, dilation, None if ib is None else ib.data_ptr(), ibp, st)
    assert rc == L.SUCCESS, rc
    arena.check()
    after = obuf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[..., oc0:oc0 + Cout] = True
    mask8 = np.repeat(mask, after.itemsize, axis=-1)
    assert np.array_equal(after.view(np.uint8)[~mask8], before[~mask8]), "bytes of the output buffer outside the slice were written"
    return after[..., oc0:oc0 + Cout].copy()
