"""linear_bias_act -- the dense layers that wrap the sampler with their whole
epilogue in the GEMM: out = act(x @ weight.T + bias + residual) as one `bevops_linear_bias_act`
call (hipBLASLt MFMA kernel, shift + identity + ReLU in its epilogue).  Not a reference plugin:
the reference leaves these layers to cuBLAS / TensorRT."""
import ctypes
import os

import torch

from ..utils import lib as _lib
from ..utils import workspace as _ws
from . import dispatch as _dispatch
from .dispatch import (DENSE_LOG, DENSE_MISSES, DETERMINISTIC, OWN_KERNELS, _DENSE_CHOICE, _TABLE,  # noqa: F401
                       _dense_default, _dense_deterministic, _dense_own, _problem, _small_pays, _table, graph_time_us,
                       own_kernel_choice)


_TUNED = set()   # problems whose algorithm has been chosen by bevops_linear_tune in this process


def _tune_once(handle, key, args, x2, out_shape):
    """The library never synchronises inside the operator; algorithm selection by measurement is
    its own BLOCKING entry (bevops_linear_tune), called here once per problem, outside stream
    capture, with a scratch output (BEVOPS_LINEAR_TUNE=0 switches it off)."""
    _TUNED.add(key)
    if os.environ.get("BEVOPS_LINEAR_TUNE", "1") == "0":
        return
    scratch = torch.empty(out_shape, dtype=x2.dtype, device=x2.device)
    a = list(args)
    a[5] = scratch.data_ptr()
    handle.bevops_linear_tune(*a)       # status ignored: the heuristic's choice stays on failure


def _operands(x, weight, bias, residual, out, bias_dtype=torch.float16, res_dtypes=None, out_dtype=None):
    """The operands of a dense call as the C entries take them: x [..., K] as contiguous rows [M, K], weight [N, K]
    contiguous, bias cast to `bias_dtype`, residual [..., N] as contiguous [M, N], `out` allocated as [M, N] or checked
    (it may be the residual itself; False: the caller lays out its own destinations).
    -> (x2, weight, bias, r2, out, M, N, K)"""
    K, N = x.shape[-1], weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError(f"weight {tuple(weight.shape)} does not match x [..., {K}]")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if not weight.is_contiguous():
        weight = weight.contiguous()
    M = x2.shape[0]
    r2 = None
    if residual is not None:
        if residual.dtype not in (res_dtypes or (x.dtype,)) or residual.numel() != M * N:
            raise ValueError(f"residual must be {res_dtypes or x.dtype} with M*N elements")
        r2 = residual.reshape(M, N)
        if not r2.is_contiguous():
            r2 = r2.contiguous()
    if bias is not None and (bias.dtype != bias_dtype or not bias.is_contiguous()):
        bias = bias.to(bias_dtype).contiguous()
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or x.dtype, device=x.device)
    elif out is not False:
        assert out.is_contiguous() and out.numel() == M * N and out.dtype == (out_dtype or x.dtype)
    return x2, weight, bias, r2, out, M, N, K


def _like_rows(out, x, N):
    """the [M, N] result with the leading dimensions of x"""
    return out.view(*x.shape[:-1], N)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _call(entry, device, *args):
    """One call of the library's `entry` on `device` and its current stream (the entry's last argument), status checked."""
    handle = _lib.load_library()
    with torch.cuda.device(device):
        st = getattr(handle, entry)(*args, _lib.current_stream_ptr(device))
    _lib.check(st, entry)


def _gemm_f16(entry, x, weight, bias, residual, relu, out, max_rows=None, launch=None):
    """One call of an fp16 GEMM entry with the shared signature (x, weight, bias, residual, out, M, N, K, relu, stream):
    operands through _operands, no library for M == 0, the status checked, the leading dimensions of x back on the
    result.  `launch(handle, args, stream)`: a caller that passes more than the shared arguments makes the call itself."""
    assert x.is_cuda and x.dtype == torch.float16 and weight.dtype == torch.float16
    x2, weight, bias, r2, out, M, N, K = _operands(x, weight, bias, residual, out)
    if max_rows is not None and M > max_rows:
        raise _lib.BevopsError(f"{entry}: more than {max_rows} rows (the tiled GEMMs' domain)", _lib.NOT_SUPPORTED)
    if M == 0:
        return _like_rows(out, x, N)
    handle = _lib.load_library()
    stream = _lib.current_stream_ptr(x.device)
    args = (x2.data_ptr(), weight.data_ptr(), _ptr(bias), _ptr(r2), out.data_ptr(), M, N, K, int(bool(relu)))
    with torch.cuda.device(x.device):
        st = getattr(handle, entry)(*args, stream) if launch is None else launch(handle, args, stream)
    _lib.check(st, entry)
    return _like_rows(out, x, N)


def linear_bias_act(x, weight, bias=None, residual=None, relu=False, out=None):
    """x [..., K] fp16 (contiguous rows), weight [N, K], bias [N] or None, residual [..., N] or None
    -> [..., N].  `out` may be given (and may be `residual` itself).  Raises BevopsError with status
    NOT_SUPPORTED when hipBLASLt has no algorithm for the shape (callers fall back to
    mm + bias_act_nhwc_)."""
    def launch(handle, args, stream):
        nbytes = handle.bevops_linear_workspace_size() if os.environ.get("BEVOPS_LINEAR_WS", "1") != "0" else 0
        # (the hipBLASLt workspace per (device, stream): two streams never share one, utils/workspace.py)
        ws = _ws.lend("linear", nbytes, x.device, stream) if nbytes else None
        full = (_lib.F16,) + args + (_ptr(ws), nbytes, stream)
        key = (str(x.device),) + args[5:8] + (bool(relu), args[2] is not None, args[3] is not None)
        if key not in _TUNED and not torch.cuda.is_current_stream_capturing():
            _tune_once(handle, key, full, x, args[5:7])
        return handle.bevops_linear_bias_act(*full)
    return _gemm_f16("bevops_linear_bias_act", x, weight, bias, residual, relu, out, launch=launch)


def layer_norm(x, weight=None, bias=None, eps=1e-5, out=None):
    """torch.nn.functional.layer_norm over the last dimension (fp16, C in {64,128,256,512}) as one
    streaming pass (bevops_layer_norm).  Raises BevopsError (status 3) for other widths."""
    assert x.is_cuda and x.dtype == torch.float16
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    if out is None:
        out = torch.empty_like(x2)
    else:
        assert out.is_contiguous() and out.numel() == x2.numel() and out.dtype == x.dtype
    w = weight.to(torch.float16).contiguous() if weight is not None else None
    b = bias.to(torch.float16).contiguous() if bias is not None else None
    if x2.shape[0] == 0:
        return out.view(x.shape)
    _call("bevops_layer_norm", x.device, _lib.F16, x2.data_ptr(), _ptr(w), _ptr(b), out.data_ptr(), x2.shape[0], C, float(eps))
    return out.view(x.shape)


def _scaled_rows(entry, x, scale, out_dtype, out=None):
    x = x.contiguous()
    if x.numel() % 8:
        raise ValueError("element count must be a multiple of 8")
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    if x.numel() == 0:
        return out
    _call(entry, x.device, _lib.F16, x.data_ptr(), out.data_ptr(), x.numel(), float(scale))
    return out


def quantize_rows(x, scale, out=None):
    """fp16 tensor -> int8 with one per-tensor scale: clamp(rne(x / scale), -127, 127) (bevops_quantize_rows)."""
    assert x.is_cuda and x.dtype == torch.float16
    return _scaled_rows("bevops_quantize_rows", x, scale, torch.int8, out)


def dequantize_rows(q, scale):
    """int8 tensor -> fp16, q * scale with the product in fp32 and one rounding (bevops_dequantize_rows)."""
    assert q.is_cuda and q.dtype == torch.int8
    return _scaled_rows("bevops_dequantize_rows", q, scale, torch.float16)


def linear_int8(a_q, scale_a, w_q, scale_w, bias=None, residual=None, relu=False, out_dtype=torch.float16,
                scale_out=1.0):
    """INT8 GEMM with de-quantising epilogue: a_q [..., K] int8 (bevops_linear_int8) -- or the fp16 activation
    itself, quantised with scale_a inside the GEMM's operand load (bevops_linear_int8_fused: no quantise pass)
    --, w_q [N, K] int8, scale_w a float (per tensor) or an fp32 [N] tensor (per output channel), bias fp32
    [N], residual fp16 [..., N] -> fp16 (or int8 requantised with scale_out)."""
    assert a_q.is_cuda and a_q.dtype in (torch.int8, torch.float16) and w_q.dtype == torch.int8
    fused = a_q.dtype == torch.float16
    a2, w_q, b, r, out, M, N, K = _operands(a_q, w_q, bias, residual, None, bias_dtype=torch.float32,
                                            res_dtypes=(torch.float16,), out_dtype=out_dtype)
    per_channel = torch.is_tensor(scale_w)
    ws = scale_w.float().contiguous() if per_channel else None
    if M == 0:
        return _like_rows(out, a_q, N)
    _call("bevops_linear_int8_fused" if fused else "bevops_linear_int8", a_q.device,
          a2.data_ptr(), float(scale_a), w_q.data_ptr(), _ptr(ws), 1.0 if per_channel else float(scale_w), _ptr(b),
          _ptr(r), _lib.torch_dtype_code(out), out.data_ptr(), float(scale_out), M, N, K, int(bool(relu)))
    return _like_rows(out, a_q, N)


def tsgemm(x, weight, bias=None, residual=None, relu=False, out=None):
    """act(x @ weight.T + bias + residual) on the hand-written tall-skinny MFMA GEMM (bevops_tsgemm_f16):
    x [..., K] fp16 contiguous rows, weight [N, K], residual / out [..., N].  Raises BevopsError with status
    NOT_SUPPORTED outside its domain (K % 64, N % 256)."""
    return _gemm_f16("bevops_tsgemm_f16", x, weight, bias, residual, relu, out)


def tsgemm_grouped(x, weight, bias=None, out=None):
    """G dense layers of 256 columns over the SAME rows in ONE launch (bevops_tsgemm_f16_grouped): x [..., K] fp16,
    weight [G * 256, K] (the G layers' weights stacked), bias [G * 256] or None -> out [G, M, 256], out[g] bit for bit
    tsgemm(x, weight[g * 256:(g + 1) * 256], bias[g * 256:(g + 1) * 256]).  The rows are read from memory once instead
    of G times.  Raises BevopsError (NOT_SUPPORTED) unless K % 64 == 0 and K <= 256."""
    assert x.is_cuda and x.dtype == torch.float16 and weight.dtype == torch.float16
    x2, weight, bias, _, _, M, N, K = _operands(x, weight, bias, None, False)
    if N % 256 != 0 or N == 0:
        raise ValueError(f"weight {tuple(weight.shape)} must be [G * 256, {K}]")
    G = N // 256
    if out is None:
        out = torch.empty((G, M, 256), dtype=x.dtype, device=x.device)
    else:
        assert out.is_contiguous() and tuple(out.shape) == (G, M, 256) and out.dtype == x.dtype
    if M == 0:
        return out
    _call("bevops_tsgemm_f16_grouped", x.device, x2.data_ptr(), weight.data_ptr(), _ptr(bias), out.data_ptr(), M * 256, M, G, K)
    return out


def tsgemm_ln(x, weight, bias, residual, ln_weight, ln_bias, eps=1e-5):
    """layer_norm(x @ weight.T + bias + residual) * ln_weight + ln_bias in ONE launch (bevops_tsgemm_f16_ln): the dense
    layer that ends an attention / FFN block of the encoder or decoder together with the block's norm
    (modules/encoder.py:586-636).  x [..., K] fp16, weight [256, K], residual [..., 256] or None.  Equal to
    layer_norm(tsgemm(...)) up to the last bit of the normalisation (same binary16 sums, fp32 statistics).  Raises
    BevopsError (NOT_SUPPORTED) unless N == 256 and K % 64 == 0."""
    g, b = ln_weight.to(torch.float16).contiguous(), ln_bias.to(torch.float16).contiguous()
    return _gemm_f16("bevops_tsgemm_f16_ln", x, weight, bias, residual, False, None, launch=lambda handle, a, stream:
                     handle.bevops_tsgemm_f16_ln(*a[:4], g.data_ptr(), b.data_ptr(), float(eps), *a[4:8], stream))


def tile_gemm(x, weight, bias=None, residual=None, relu=False, out=None):
    """act(x @ weight.T + bias + residual) on the tiled MFMA GEMM (bevops_tile_gemm_f16, csrc/tile_gemm.hip:
    128 x 128 tiles, three blocks per CU): x [..., K] fp16 contiguous rows, weight [N, K], bias [N] fp16,
    residual / out [..., N].  K % 8 == 0."""
    return _gemm_f16("bevops_tile_gemm_f16", x, weight, bias, residual, relu, out)


class _GemmDst(ctypes.Structure):     # bevops_gemm_dst (include/bevops.h)
    _fields_ = [("col_begin", ctypes.c_int), ("col_end", ctypes.c_int), ("out", ctypes.c_void_p),
                ("out_pitch", ctypes.c_longlong), ("res", ctypes.c_void_p), ("res_pitch", ctypes.c_longlong)]


def tile_gemm_dst(x, weight, bias, widths, residuals=None, relu=False, outs=None, _entry="bevops_tile_gemm_f16_dst"):
    """Several layers over the SAME rows in ONE launch of the tiled GEMM (bevops_tile_gemm_f16_dst): weight [N, K] and
    bias [N] (or None) are the layers' parameters stacked, `widths` their column counts (multiples of 64, sum N);
    residuals[i] is None or layer i's identity [M, widths[i]] (any row pitch that is a multiple of 8).  Returns the
    list of dense [M, widths[i]] results -- each bit for bit tile_gemm(x, weight_i, bias_i, residuals[i], relu).
    `outs`: optional destinations (2-d, unit column stride, row pitch a multiple of 8)."""
    assert x.is_cuda and x.dtype == torch.float16 and weight.dtype == torch.float16
    x2, weight, bias, _, _, M, N, K = _operands(x, weight, bias, None, False)
    if sum(widths) != N:
        raise ValueError(f"weight {tuple(weight.shape)} does not match widths {list(widths)}")
    if outs is None:
        outs = [torch.empty((M, n), dtype=x.dtype, device=x.device) for n in widths]
    residuals = residuals if residuals is not None else [None] * len(widths)
    if M == 0:
        return outs
    tab = (_GemmDst * len(widths))()
    col = 0
    for i, n in enumerate(widths):
        o, r = outs[i], residuals[i]
        assert o.dtype == x.dtype and tuple(o.shape) == (M, n) and (n == 1 or o.stride(1) == 1)
        tab[i].col_begin, tab[i].col_end, tab[i].out, tab[i].out_pitch = col, col + n, o.data_ptr(), o.stride(0) if M > 1 else n
        if r is not None:
            if r.dtype != x.dtype or tuple(r.shape) != (M, n) or r.stride(1) != 1:
                raise ValueError("residual must be fp16 [M, width] with unit column stride")
            tab[i].res, tab[i].res_pitch = r.data_ptr(), r.stride(0) if M > 1 else n
        col += n
    _call(_entry, x.device, x2.data_ptr(), weight.data_ptr(), _ptr(bias), ctypes.addressof(tab), len(widths), M, N, K,
          int(bool(relu)))
    return outs


def gemm2(a1, a2, weight, bias=None, stride=1, relu=False, out=None):
    """act(a1 @ W1.T + rows(a2) @ W2.T + bias) as ONE accumulation (bevops_gemm2_f16): a1 [..., K1] fp16 contiguous rows,
    a2 a [B, K2, H, W] fp16 tensor in channels-last memory whose row m is pixel (b, stride * ho, stride * wo), weight
    [N, K1 + K2] = [W1 | W2], bias [N] -> [M, N] with M = B * Ho * Wo.  The first bottleneck of a ResNet stage: conv3 on
    the block's hidden rows and the (strided) downsample convolution on the block's input, no identity tensor in
    between.  k order: source 1, then source 2; one rounding.  Raises BevopsError (NOT_SUPPORTED) unless K1 and K2 are
    multiples of 64, N % 8 == 0 and stride is 1 or 2."""
    assert a1.is_cuda and a1.dtype == torch.float16 and a2.dtype == torch.float16 and weight.dtype == torch.float16
    if a2.dim() != 4 or not a2.is_contiguous(memory_format=torch.channels_last):
        raise ValueError("a2 must be a 4-d tensor in channels-last memory")
    B, K2, H, W = a2.shape
    K1, N = a1.shape[-1], weight.shape[0]
    if weight.shape[1] != K1 + K2:
        raise ValueError(f"weight {tuple(weight.shape)} does not match [N, {K1} + {K2}]")
    x1 = a1.reshape(-1, K1)
    if not x1.is_contiguous():
        x1 = x1.contiguous()
    if not weight.is_contiguous():
        weight = weight.contiguous()
    if bias is not None and (bias.dtype != torch.float16 or not bias.is_contiguous()):
        bias = bias.to(torch.float16).contiguous()
    M = x1.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=a1.dtype, device=a1.device)
    else:
        assert out.is_contiguous() and out.numel() == M * N and out.dtype == a1.dtype
    if M == 0:
        return out
    _call("bevops_gemm2_f16", a1.device, x1.data_ptr(), a2.data_ptr(), weight.data_ptr(), _ptr(bias), out.data_ptr(), M, N,
          K1, K2, B, H, W, int(stride), int(bool(relu)))
    return out


def small_gemm_dst(x, weight, bias, widths, residuals=None, relu=False, outs=None):
    """tile_gemm_dst's call on the few-row GEMM (bevops_small_gemm_f16_dst): every layer but the last has a width that
    is a multiple of 64, the last a multiple of 8; each result bit for bit small_gemm(x, weight_i, bias_i, residuals[i])."""
    if x.numel() // x.shape[-1] > 8192:
        raise _lib.BevopsError("small_gemm_dst: more than 8192 rows (the tiled GEMMs' domain)", _lib.NOT_SUPPORTED)
    return tile_gemm_dst(x, weight, bias, widths, residuals, relu, outs, _entry="bevops_small_gemm_f16_dst")


class _ChainDst(ctypes.Structure):    # bevops_chain_dst (include/bevops.h)
    _fields_ = [("col_begin", ctypes.c_int), ("col_end", ctypes.c_int), ("out", ctypes.c_void_p), ("pitch", ctypes.c_longlong)]


class _ChainStage(ctypes.Structure):  # bevops_chain_stage
    _fields_ = [("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("K", ctypes.c_int), ("N", ctypes.c_int),
                ("input", ctypes.c_int), ("act", ctypes.c_int), ("packed", ctypes.c_int), ("res", ctypes.c_void_p), ("res_pitch", ctypes.c_longlong),
                ("res_stage", ctypes.c_int), ("norm", ctypes.c_int), ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("eps", ctypes.c_float), ("num_dst", ctypes.c_int), ("dst", _ChainDst * 2)]


def pack_chain_weight(weight):
    """weight [..., N, K] fp16 (K % 32 == 0) in the order bevops_row_chain_f16 reads a `packed` stage: whole 16-row tiles
    (zero rows behind N), per tile and 32-value k-step the 64 lanes' 8 values each -- [..., ceil(N / 16) * 16 * K]."""
    *lead, N, K = weight.shape
    assert weight.dtype == torch.float16 and K % 32 == 0
    T = (N + 15) // 16
    w = torch.zeros(*lead, T * 16, K, dtype=weight.dtype, device=weight.device)
    w[..., :N, :] = weight.detach()
    w = w.view(*lead, T, 16, K // 32, 4, 8)           # tile, row, k-step, lane group, value
    d = len(lead)
    return w.permute(*range(d), d, d + 2, d + 3, d + 1, d + 4).reshape(*lead, T * 16 * K).contiguous()


def row_chain(x, stages, groups=1):
    """A chain of dense stages over the same rows as ONE launch (bevops_row_chain_f16, csrc/row_chain.hip): the rows of
    the intermediate stages never leave the chip.  x [groups * M, K0] fp16 (unit column stride, any row pitch that is a
    multiple of 8); `stages` a list of dicts:
        weight [N, K] (groups > 1: [G, N, K]), bias [N] / [G, N] or None, relu (False),
        packed (N, K): `weight` is pack_chain_weight of that matrix (one contiguous kilobyte per request: the fast form),
        input (-1: the stage in front; s: the output of stage s),
        res (identity tensor [groups * M, N]) or res_stage (s: the INPUT rows of stage s as identity),
        norm (gamma, beta, eps) or None: LayerNorm behind bias and identity, in front of the ReLU,
        store: False (nothing leaves the chip), True (a new dense [groups * M, N] tensor), a tensor to write, or a list
               of column widths (at most two, from column 0 on, every start a multiple of 8): one dense tensor each.
    Returns the list of stored tensors in stage order (a width list contributes one tensor per width).  Raises
    BevopsError (NOT_SUPPORTED) outside the entry's domain: K % 32 == 0, K <= 768, N <= 768, at most 8 stages."""
    assert x.is_cuda and x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    rows = x.shape[0]
    assert rows % groups == 0
    M = rows // groups
    tab = (_ChainStage * len(stages))()
    outs, keep = [], []
    for i, st in enumerate(stages):
        w, b = st["weight"], st.get("bias")
        assert w.dtype == torch.float16 and w.is_contiguous() and (b is None or (b.dtype == torch.float16 and b.is_contiguous()))
        e = tab[i]
        e.weight, e.bias = w.data_ptr(), _ptr(b)
        e.N, e.K = st["packed"] if st.get("packed") else (w.shape[-2], w.shape[-1])
        e.packed = int(bool(st.get("packed")))
        if e.packed and w.numel() != groups * ((e.N + 15) // 16) * 16 * e.K:
            raise ValueError("packed weight does not match (N, K)")
        e.input, e.act = int(st.get("input", -1)), int(bool(st.get("relu", False)))
        res = st.get("res")
        e.res_stage = int(st.get("res_stage", -1))
        if res is not None:
            if res.dtype != torch.float16 or tuple(res.shape) != (rows, e.N) or res.stride(1) != 1:
                raise ValueError("res must be fp16 [rows, N] with unit column stride")
            e.res, e.res_pitch = res.data_ptr(), res.stride(0) if rows > 1 else e.N
        norm = st.get("norm")
        if norm is not None:
            gamma, beta, eps = norm
            assert gamma.dtype == torch.float16 and beta.dtype == torch.float16 and gamma.is_contiguous() and beta.is_contiguous()
            e.norm, e.gamma, e.beta, e.eps = 1, gamma.data_ptr(), beta.data_ptr(), float(eps)
            keep += [gamma, beta]
        store = st.get("store", False)
        if store is True:
            store = torch.empty((rows, e.N), dtype=x.dtype, device=x.device)
        if torch.is_tensor(store):
            assert store.dtype == x.dtype and tuple(store.shape) == (rows, e.N) and (e.N == 1 or store.stride(1) == 1)
            e.num_dst = 1
            e.dst[0].col_begin, e.dst[0].col_end, e.dst[0].out = 0, e.N, store.data_ptr()
            e.dst[0].pitch = store.stride(0) if rows > 1 else e.N
            outs.append(store)
        elif store:
            col = 0
            e.num_dst = len(store)
            for d, n in enumerate(store):
                o = torch.empty((rows, n), dtype=x.dtype, device=x.device)
                e.dst[d].col_begin, e.dst[d].col_end, e.dst[d].out, e.dst[d].pitch = col, col + n, o.data_ptr(), n
                col += n
                outs.append(o)
    if M:
        _call("bevops_row_chain_f16", x.device, x.data_ptr(), x.stride(0) if rows > 1 else x.shape[1],
              ctypes.addressof(tab), len(stages), M, int(groups))
    return outs


def tsgemm_weight_stationary(K):
    """True when bevops_tsgemm_f16 runs its weight-stationary kernel for this K (K <= 256 under the default variant; not
    under bevops_tsgemm_set_variant(1) / BEVOPS_TSGEMM_WS=0, whose kernel rotates its k start by block index)."""
    return _lib.load_library().bevops_tsgemm_tile_rows(int(K)) == 64


def small_gemm(x, weight, bias=None, residual=None, relu=False, out=None):
    """act(x @ weight.T + bias + residual) for layers with FEW rows (the decoder's 900 queries) on the
    no-pipeline MFMA GEMM (bevops_small_gemm_f16, csrc/small_gemm.hip: 32 x 64 tiles, split-K inside the block, every
    operand fragment requested before the first matrix instruction -- one memory round trip per launch instead of a
    chain of dependent k-steps).  x [..., K] fp16, weight [N, K]; K % 64 == 0, K <= 1024; offered up to 8192 rows."""
    return _gemm_f16("bevops_small_gemm_f16", x, weight, bias, residual, relu, out, max_rows=8192)


# ---- measured choice between the dense-layer implementations -------------------------------------------------
def _torch_dense(x, weight, bias, residual, relu):
    if residual is not None or bias is None:
        raise _lib.BevopsError("torch addmm path: bias required, no identity term", _lib.NOT_SUPPORTED)
    x2 = x.reshape(-1, x.shape[-1])
    y = torch._addmm_activation(bias, x2, weight.t()) if relu else torch.addmm(bias, x2, weight.t())
    return y.view(*x.shape[:-1], weight.shape[0])


_DENSE = {"tsgemm": tsgemm, "tile": tile_gemm, "small": small_gemm, "blaslt": linear_bias_act, "torch": _torch_dense}


def dense_auto(x, weight, bias=None, residual=None, relu=False):
    """act(x @ weight.T + bias + residual), fp16, on whichever of the implementations is fastest for the
    problem on THIS device: the tall-skinny persistent GEMM (tsgemm), the tiled GEMM (tile_gemm), the hipBLASLt
    entry with the fused epilogue (linear_bias_act) or the framework's addmm.  Measured once per
    (M, N, K, epilogue) outside stream capture -- BLOCKING, like bevops_linear_tune: a few launches of each
    candidate into scratch outputs between device synchronisations -- then cached for the process.  All
    candidates accumulate in fp32 and round once; they differ in summation order only.  Who decides what:
    functions/dispatch.py (dense_choice)."""
    K, N = x.shape[-1], weight.shape[0]
    M = x.numel() // K
    if M == 0:          # a rank of the camera-sharded path that owns no camera
        return x.new_empty((*x.shape[:-1], N))
    key = (str(x.device), M, N, K, bool(relu), bias is not None, residual is not None)
    name, keep, miss = _dispatch.dense_choice(key, DETERMINISTIC["enabled"], OWN_KERNELS["enabled"],
                                              torch.cuda.is_current_stream_capturing, _dispatch._tune, _table(_TABLE),
                                              _DENSE_CHOICE.get(key))
    if miss and _problem(key) not in DENSE_MISSES:
        DENSE_MISSES.append(_problem(key))     # a problem the shipped table has never seen (bench.py reports them)
    if name == "measure":
        name = _dense_measure(key, x, weight, bias, residual, relu)
    if keep:
        _DENSE_CHOICE[key] = name
    try:
        return _DENSE[name](x, weight, bias, residual, relu)
    except _lib.BevopsError as exc:
        if exc.status != _lib.NOT_SUPPORTED or name == "blaslt":
            raise
        return linear_bias_act(x, weight, bias, residual, relu)


def _dense_measure(key, x, weight, bias, residual, relu, rounds=3, iters=8):
    with torch.cuda.device(x.device):
        times = _dispatch.measure(_DENSE, lambda name: _DENSE[name](x, weight, bias, residual, relu), iters, rounds)
    DENSE_LOG.append((key, {k: round(v, 1) for k, v in times.items()}))
    return min(times, key=times.get) if times else "blaslt"


def tsa_split(both, heads, points):
    """The stacked sampling_offsets | attention_weights projection of temporal self-attention, [nq, heads * 2 * points * 3]
    fp16 with the reference's column order ([heads][queue][points][xy] | [heads][queue][points]), as the queue-major
    operands of the MSDA call: (offsets [2, nq, heads, points * 2], weights [2, nq, heads, points]) in ONE pass
    (bevops_tsa_split) instead of two permute-copies."""
    assert both.is_cuda and both.dtype == torch.float16 and both.dim() == 2 and both.is_contiguous()
    nq = both.shape[0]
    assert both.shape[1] == heads * 2 * points * 3
    off = torch.empty((2, nq, heads, points * 2), dtype=both.dtype, device=both.device)
    w = torch.empty((2, nq, heads, points), dtype=both.dtype, device=both.device)
    _call("bevops_tsa_split", both.device, _lib.F16, both.data_ptr(), off.data_ptr(), w.data_ptr(), nq, heads, points)
    return off, w


def queue_mean2(x):
    """torch.mean(x, dim=0, keepdim=True) for x [2, ...] fp16 as one streaming pass (bevops_queue_mean2)."""
    assert x.is_cuda and x.dtype == torch.float16 and x.shape[0] == 2 and x.is_contiguous()
    out = torch.empty((1,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    _call("bevops_queue_mean2", x.device, _lib.F16, x.data_ptr(), out.data_ptr(), out.numel())
    return out
