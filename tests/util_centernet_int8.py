"""Operator sets for the tests of the INT8 CenterNet (tests/test_centernet_int8_cpu.py, tests/test_centernet_int8_gpu.py):

* `ShapeOps`: the entries Int8CenterNet.run calls, computing nothing -- zero tensors of the right shape and type on the
  input's device, so the plan runs without a GPU.
* `ScaleRecorder(inner)`: forwards every entry to `inner` and keeps, per int8 tensor (by address; every tensor is kept
  alive, so no address is used twice), the scale it was written with; every int8 tensor an entry reads must have been
  written, with exactly the scale the entry reads it with.  `calls`: (entry, arguments, result) of every convolution,
  deconvolution and DCN call, for the replay against the float64 statements."""
import torch


def _nhwc(B, C, H, W, dtype, device):
    return torch.zeros((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


class ShapeOps:
    def __init__(self, fp):
        self.fp = fp

    def stem_conv_pool(self, x, weight, bias=None, scale_out=None):
        B, _, H, W = x.shape
        return _nhwc(B, 64, H // 4, W // 4, torch.float16 if scale_out is None else torch.int8, x.device)

    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False):
        B, _, H, W = x_q.shape
        return _nhwc(B, w.shape[0], (H - 1) // stride + 1, (W - 1) // stride + 1, out_dtype, x_q.device)

    def conv_int8_chain_nhwc(self, x_q, scale_a, w, scale_w, bias=None, relu=False, stride=1, out_dtype=torch.float16,
                             scale_out=1.0):
        B, _, H, W = x_q.shape
        return _nhwc(B, w.shape[0], H, W, out_dtype, x_q.device)

    def modulated_deformable_conv2d_int8_nhwc(self, x_q, scale_in, om, scale_offset, scale_mask, weight_q, scale_weight, bias,
                                              scale_out, relu=False, stride=1, padding=1, dilation=1, groups=1,
                                              deform_groups=1, exact=False):
        B, _, H, W = x_q.shape
        return _nhwc(B, weight_q.shape[0], H, W, torch.int8, x_q.device)

    def conv_transpose2d_q_nhwc(self, x_q, scale_x, weight_q, w_scales, bias, relu, scale_out=None, out_dtype=torch.int8):
        B, _, H, W = x_q.shape
        return _nhwc(B, weight_q.shape[1], 2 * H, 2 * W, out_dtype, x_q.device)

    def quantize_rows(self, x, scale, out=None):
        return torch.zeros(x.shape, dtype=torch.int8, device=x.device)

    def neck_fp16(self, x, ops):
        """Stands in for CTResNetNeck.forward_nhwc (monkey-patched in by the CPU test): fp16 in, fp16 out, 8 x the size."""
        B, _, H, W = x.shape
        assert x.dtype == torch.float16
        return _nhwc(B, 64, 8 * H, 8 * W, torch.float16, x.device)


class ScaleRecorder:
    def __init__(self, inner, keep_calls=False):
        self.inner, self.keep_calls = inner, keep_calls
        self.written, self.alive, self.reads, self.calls = {}, [], 0, []

    def __getattr__(self, name):            # (entries this class does not define: the fp16 neck's)
        return getattr(self.inner, name)

    def _read(self, t, scale, what):
        assert t.dtype == torch.int8, what
        key = t.data_ptr()
        assert key in self.written, f"{what}: reads an int8 tensor nobody wrote"
        assert self.written[key] == float(scale), f"{what}: read with scale {scale}, written with {self.written[key]}"
        self.reads += 1

    def _wrote(self, t, scale, what):
        self.alive.append(t)
        if t.dtype == torch.int8:
            assert scale is not None and t.data_ptr() not in self.written, what
            self.written[t.data_ptr()] = float(scale)
        return t

    def _call(self, name, args, kwargs):
        out = getattr(self.inner, name)(*args, **kwargs)
        if self.keep_calls:
            self.calls.append((name, args, kwargs, out))
        return out

    def stem_conv_pool(self, x, weight, bias=None, scale_out=None):
        return self._wrote(self.inner.stem_conv_pool(x, weight, bias, scale_out), scale_out, "stem")

    def conv_slice_q_taps(self, x_q, scale_x, w, ws, bias, act, residual_q=None, scale_res=1.0, stride=1, out=None,
                          scale_out=None, out_dtype=torch.int8, res_first=False):
        self._read(x_q, scale_x, "conv input")
        if residual_q is not None:
            self._read(residual_q, scale_res, "conv identity")
        y = self._call("conv_slice_q_taps", (x_q, scale_x, w, ws, bias, act, residual_q, scale_res, stride, out, scale_out,
                                             out_dtype), dict(res_first=res_first))
        return self._wrote(y, scale_out, "conv output")

    def conv_int8_chain_nhwc(self, x_q, scale_a, w, scale_w, bias=None, relu=False, stride=1, out_dtype=torch.float16,
                             scale_out=1.0):
        self._read(x_q, scale_a, "offset convolution input")
        y = self._call("conv_int8_chain_nhwc", (x_q, scale_a, w, scale_w, bias, relu, stride, out_dtype, scale_out), {})
        return self._wrote(y, scale_out, "offset convolution output")

    def modulated_deformable_conv2d_int8_nhwc(self, x_q, scale_in, om, scale_offset, scale_mask, weight_q, scale_weight, bias,
                                              scale_out, relu=False, stride=1, padding=1, dilation=1, groups=1,
                                              deform_groups=1, exact=False):
        self._read(x_q, scale_in, "DCN input")
        y = self._call("modulated_deformable_conv2d_int8_nhwc",
                       (x_q, scale_in, om, scale_offset, scale_mask, weight_q, scale_weight, bias, scale_out, relu, stride,
                        padding, dilation, groups, deform_groups, exact), {})
        return self._wrote(y, scale_out, "DCN output")

    def conv_transpose2d_q_nhwc(self, x_q, scale_x, weight_q, w_scales, bias, relu, scale_out=None, out_dtype=torch.int8):
        self._read(x_q, scale_x, "deconvolution input")
        y = self._call("conv_transpose2d_q_nhwc", (x_q, scale_x, weight_q, w_scales, bias, relu, scale_out, out_dtype), {})
        return self._wrote(y, scale_out, "deconvolution output")

    def quantize_rows(self, x, scale, out=None):
        assert x.dtype == torch.float16
        return self._wrote(self.inner.quantize_rows(x, scale), scale, "quantize pass")

    def check(self):
        assert self.written and self.reads


# ---------------------------------------------------------------------------------------------- float64 statements
def epilogue_interval(acc, scale_a, w_scales, bias, res_q, scale_res, relu, scale_out, unfused=False):
    """General scales, the epilogue of bevops_conv_slice_s8_ex(res_first = 1) / bevops_deconv4x4s2_s8 /
    bevops_conv_tile_int8 on exact integer sums `acc` [..., Cout]:  v = sum sc + bias;  v += res_q scale_res (in front of
    the activation);  y = relu(v);  t = y / scale_out.  The half-width of the interval the kernel's fp32 value lies in,
    derived as tests/util_deconv_s8.py derives it (u = 2^-24, P = |sum| sc):
        e_v = u (3 P + |v|)(1 + 2^-20)     two roundings of sc, (float)sum beyond 2^24, the fma's one rounding
              (unfused: 4 P -- an entry that multiplies and adds separately rounds the product too)
        e_v += u |v + r|                   the identity's fma: the product res_q * scale_res is exact inside it
        delta = (e_v (1 + 3 u) + 2.01 u |y|) / scale_out
    -> (t, delta, y_lo, y_hi) float64: int8 outputs lie in [clamp(rne(t - delta)), clamp(rne(t + delta))], fp16 outputs in
    [f16(y_lo), f16(y_hi)]."""
    import numpy as np
    u = 2.0 ** -24
    sc = float(np.float32(scale_a)) * np.asarray(w_scales, dtype=np.float32).astype(np.float64)
    prod = acc.astype(np.float64) * sc
    v = prod + np.asarray(bias, dtype=np.float32).astype(np.float64)
    e = u * ((4.0 if unfused else 3.0) * np.abs(prod) + np.abs(v)) * (1.0 + 2.0 ** -20)
    if res_q is not None:
        v = v + res_q.astype(np.float64) * float(np.float32(scale_res))
        e = e + u * np.abs(v)
    act = (lambda a: np.maximum(a, 0.0)) if relu else (lambda a: a)
    y = act(v)
    so = 1.0 if scale_out is None else float(np.float32(scale_out))
    return y / so, (e * (1.0 + 3.0 * u) + 2.01 * u * np.abs(y)) / so, act(v - e), act(v + e)


def check_output(got, t, delta, y_lo, y_hi, cap=0.01):
    """`got` int8 or fp16 [..., Cout] inside its interval; EQUAL to the statement's rounding wherever the interval's two
    ends round alike; the share of the other outputs at most `cap`.  -> (that share, share differing from the rounding)."""
    import numpy as np
    if got.dtype == np.int8:
        lo = np.clip(np.rint(t - delta), -127, 127).astype(np.int8)
        hi = np.clip(np.rint(t + delta), -127, 127).astype(np.int8)
        mid = np.clip(np.rint(t), -127, 127).astype(np.int8)
    else:
        lo, hi, mid = y_lo.astype(np.float16), y_hi.astype(np.float16), (0.5 * (y_lo + y_hi)).astype(np.float16)
    bad = np.argwhere((got < lo) | (got > hi))
    assert len(bad) == 0, (f"{len(bad)} of {got.size} outputs outside their interval, first at {tuple(bad[0])}: got "
                           f"{got[tuple(bad[0])]}, allowed {lo[tuple(bad[0])]} .. {hi[tuple(bad[0])]}")
    share = float((lo != hi).mean())
    assert share <= cap, f"{share:.4%} of the outputs lie within delta of a rounding boundary (cap {cap:.0%})"
    return share, float((got != mid).mean())
