"""Operator sets and statements for the tests of the INT8 BEV half of BEVDet (tests/test_bevdet_int8_cpu.py,
tests/test_bevdet_int8_gpu.py):

* `ShapeOps`: the entries Int8BEVDet.run calls, computing nothing -- zero tensors of the right shape and type on the
  input's device (written into `out` where one is given), so the plan runs without a GPU.
* `ScaleRecorder(inner)`: forwards every entry to `inner` and keeps, per int8 buffer and channel range, the scale it was
  written with; every int8 tensor an entry reads must have been written over its whole channel range -- by one writer
  or, for the concatenation buffer, by two -- with exactly the scale the entry reads it with.  `calls`: (entry,
  arguments, result) of every call, for the replay against the float64 statements.
* `conv_sums` / `epilogue_interval` / `check_output`: tests/util_centernet_int8.py's convolution statement in torch
  float64 on the tensors' device (the BEV half's layers are too large for numpy): exact integer sums, then the derived
  interval of the epilogue of bevops_conv_slice_s8_ex."""
import torch
import torch.nn.functional as F


def _nhwc(B, C, H, W, dtype, device):
    return torch.zeros((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


class ShapeOps:
    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False):
        B, cin, H, W = x_q.shape
        assert x_q.dtype == torch.int8 and w.shape[3] == cin
        shape = (B, w.shape[0], (H - 1) // stride + 1, (W - 1) // stride + 1)
        if residual_q is not None:
            assert tuple(residual_q.shape) == shape and residual_q.dtype == torch.int8
        if out is not None:
            assert tuple(out.shape) == shape and out.dtype == out_dtype
            return out
        return _nhwc(*shape, out_dtype, x_q.device)

    def quantize_rows(self, x, scale, out=None):
        assert x.dtype == torch.float16
        return torch.zeros(x.shape, dtype=torch.int8, device=x.device)

    def lss_depth_split_q(self, x, n, D, C, depth_offset, feat_offset, scale_depth, scale_feat, spatial=None):
        assert x.dtype == torch.float16 and x.dim() == 2 and x.is_contiguous()
        H, W = spatial
        assert x.shape[0] == n * H * W
        return (torch.zeros((n, D, H, W), dtype=torch.int8, device=x.device),
                torch.zeros((n, H, W, C), dtype=torch.int8, device=x.device))

    def bev_pool_v2_int8(self, depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths, scale_depth,
                         scale_feat, scale_out, out_height=128, out_width=128):
        assert depth.dtype == feat.dtype == torch.int8
        return torch.zeros((1, out_height, out_width, feat.shape[-1]), dtype=torch.int8, device=feat.device)

    def upsample_bilinear_nhwc_q(self, b_q, scale_b, scale_out, size=None, scale_factor=None, out=None):
        B, C, H, W = b_q.shape
        assert b_q.dtype == torch.int8
        if out is not None:
            assert out.dtype == torch.int8 and out.shape[:2] == (B, C)
            return out
        return _nhwc(B, C, H * scale_factor, W * scale_factor, torch.int8, b_q.device)


def _channels(t):
    """(buffer key, first channel, last channel + 1) of an int8 tensor: a channel slice of a channels-last buffer, or a
    contiguous tensor of its own."""
    key = t.untyped_storage().data_ptr()
    if t.dim() == 4 and t.shape[1] > 1 and t.stride(1) == 1 and t.shape[3] > 1:
        c0 = t.storage_offset() % t.stride(3)
        return key, c0, c0 + t.shape[1]
    return key, 0, None


class ScaleRecorder:
    def __init__(self, inner, keep_calls=False):
        self.inner, self.keep_calls = inner, keep_calls
        self.written, self.alive, self.reads, self.calls = {}, [], 0, []

    def _read(self, t, scale, what):
        assert t.dtype == torch.int8, what
        key, c0, c1 = _channels(t)
        assert key in self.written, f"{what}: reads an int8 tensor nobody wrote"
        have = sorted(self.written[key])
        if c1 is None or any(b is None for _, b, _ in have):      # (a tensor of its own, written whole)
            assert [s for _, _, s in have] == [float(scale)], f"{what}: read with scale {scale}, written {have}"
        else:
            at = c0
            for a, b, s in have:
                if b <= c0 or a >= c1:
                    continue
                assert a == at, f"{what}: channels {at} .. {a} were never written"
                assert s == float(scale), f"{what}: read with scale {scale}, channels {a} .. {b} written with {s}"
                at = b
            assert at == c1, f"{what}: channels {at} .. {c1} were never written"
        self.reads += 1

    def _wrote(self, t, scale, what):
        self.alive.append(t)
        if t.dtype == torch.int8:
            assert scale is not None, what
            key, c0, c1 = _channels(t)
            rows = self.written.setdefault(key, [])
            assert all(b <= c0 or (c1 is not None and a >= c1) for a, b, _ in rows if b is not None) and \
                not (rows and c1 is None), f"{what}: written twice"
            rows.append((c0, c1, float(scale)))
        return t

    def _call(self, name, args, kwargs):
        out = getattr(self.inner, name)(*args, **kwargs)
        if self.keep_calls:
            self.calls.append((name, args, kwargs, out))
        return out

    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False):
        self._read(x_q, scale_x, "conv input")
        if residual_q is not None:
            self._read(residual_q, scale_res, "conv identity")
        y = self._call("conv_slice_q_taps", (x_q, scale_x, w, ws, bias, act, residual_q, scale_res, stride, out, scale_out,
                                             out_dtype), dict(res_first=res_first))
        return self._wrote(y, scale_out, "conv output")

    def quantize_rows(self, x, scale, out=None):
        assert x.dtype == torch.float16
        return self._wrote(self._call("quantize_rows", (x, scale), {}), scale, "quantize pass")

    def lss_depth_split_q(self, x, n, D, C, depth_offset, feat_offset, scale_depth, scale_feat, spatial=None):
        d, f = self._call("lss_depth_split_q", (x, n, D, C, depth_offset, feat_offset, scale_depth, scale_feat),
                          dict(spatial=spatial))
        return self._wrote(d, scale_depth, "depth"), self._wrote(f, scale_feat, "features")

    def bev_pool_v2_int8(self, depth, feat, rd, rf, rb, ist, il, scale_depth, scale_feat, scale_out, out_height=128,
                         out_width=128):
        self._read(depth, scale_depth, "pooling depth")
        self._read(feat, scale_feat, "pooling features")
        y = self._call("bev_pool_v2_int8", (depth, feat, rd, rf, rb, ist, il, scale_depth, scale_feat, scale_out, out_height,
                                            out_width), {})
        return self._wrote(y, scale_out, "pooling output")

    def upsample_bilinear_nhwc_q(self, b_q, scale_b, scale_out, size=None, scale_factor=None, out=None):
        self._read(b_q, scale_b, "up-sampler input")
        y = self._call("upsample_bilinear_nhwc_q", (b_q, scale_b, scale_out), dict(scale_factor=scale_factor, out=out))
        return self._wrote(y, scale_out, "up-sampler output")

    def check(self):
        assert self.written and self.reads


# ---------------------------------------------------------------------------------------------- float64 statements
def conv_sums(x_q, w_q_taps, stride):
    """The exact integer sums of a convolution, float64 [B, Ho, Wo, Cout] (|sum| < 2^53): x_q int8 [B, Cin, H, W] (any
    strides), w_q_taps int8 [Cout, k, k, Cin], pad k / 2."""
    cout, k, _, cin = w_q_taps.shape
    B, _, H, W = x_q.shape
    cols = F.unfold(x_q.double().contiguous(), k, padding=k // 2, stride=stride)          # [B, Cin k k, L], (c, ky, kx) order
    wm = w_q_taps.permute(0, 3, 1, 2).reshape(cout, cin * k * k).double()
    out = torch.matmul(wm, cols)                                                          # [B, Cout, L]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return out.view(B, cout, Ho, Wo).permute(0, 2, 3, 1)


def epilogue_interval(acc, scale_a, w_scales, bias, res_q, scale_res, relu, scale_out):
    """tests/util_centernet_int8.py's `epilogue_interval` (the fused entry, identity in front of the activation) on
    torch float64 tensors [..., Cout].  -> (t, delta, y_lo, y_hi)."""
    u = 2.0 ** -24
    f32 = lambda s: float(torch.tensor(s, dtype=torch.float32))
    sc = f32(scale_a) * w_scales.float().double()
    prod = acc * sc
    v = prod + bias.float().double()
    e = u * (3.0 * prod.abs() + v.abs()) * (1.0 + 2.0 ** -20)
    if res_q is not None:
        v = v + res_q.double() * f32(scale_res)
        e = e + u * v.abs()
    act = (lambda a: a.clamp(min=0.0)) if relu else (lambda a: a)
    y = act(v)
    so = 1.0 if scale_out is None else f32(scale_out)
    return y / so, (e * (1.0 + 3.0 * u) + 2.01 * u * y.abs()) / so, act(v - e), act(v + e)


def check_output(got, t, delta, y_lo, y_hi, cap=0.01):
    """tests/util_centernet_int8.py's `check_output` on torch tensors: `got` int8 or fp16 [..., Cout] inside its
    interval; the share of outputs whose interval holds two roundings at most `cap`.  -> (that share, share differing
    from the statement's rounding)."""
    if got.dtype == torch.int8:
        q = lambda a: a.round().clamp(-127, 127)
        lo, hi, mid, g = q(t - delta), q(t + delta), q(t), got.double()
    else:
        h = lambda a: a.half().double()
        lo, hi, mid, g = h(y_lo), h(y_hi), h(0.5 * (y_lo + y_hi)), got.double()
    bad = (g < lo) | (g > hi)
    assert not bool(bad.any()), f"{int(bad.sum())} of {g.numel()} outputs outside their interval"
    share = float((lo != hi).double().mean())
    assert share <= cap, f"{share:.4%} of the outputs lie within delta of a rounding boundary (cap {cap:.0%})"
    return share, float((g != mid).double().mean())
