"""The layers of BEVDepth's DepthNet that are no convolution (csrc/lss_depthnet.hip): the camera-aware squeeze-excite
gates from the 27 calibration values of every camera (`lss_camera_gate`, fp32 throughout), the gate applied to the depth
and the context branch in one pass (`se_gate2_nhwc`) and ASPP's global average pool (`global_avgpool_nhwc`), and
the INT8 siblings of those two on int8 channel slices (`se_gate2_nhwc_q`, `global_avgpool_nhwc_q`;
csrc/lss_depthnet_s8.hip).  Not reference plugins (TensorRT owns these layers there), so none is in TRT_FUNCTIONS.

`pack_camera_gate` builds the one fp32 parameter block `lss_camera_gate` reads -- the frozen BatchNorm1d(27) folded
into fc1, every matrix k-major; include/bevops.h states the layout.  `camera_gate_packed` caches it per weight stamp
and never builds it inside a stream capture (RuntimeError)."""
import torch

from ..utils import lib as _lib
from .linear import _call
from .multi_scale_deformable_attn import _TensorCache
from .yolox_ops import _check_f16, _check_s8, _dest, _scale, slice_pitch

GATE_INPUTS = 27
_GATE_PACKED = _TensorCache()    # depth branch's fc1 weight -> (stamps of all sixteen tensors, block)


def _branch_block(mlp_w1, mlp_b1, mlp_w2, mlp_b2, red_w, red_b, exp_w, exp_b, scale, shift):
    """One branch's words, in float64 until the last step: W1 [27][mid] | b1 | W2 [mid][mid] | b2 | Wr | br | We | be."""
    w1 = mlp_w1.detach().double().cpu()
    mid = w1.shape[0]
    if tuple(w1.shape) != (mid, GATE_INPUTS):
        raise ValueError(f"pack_camera_gate: fc1.weight [mid, {GATE_INPUTS}], got {tuple(w1.shape)}")
    parts = [(w1 * scale[None, :]).t(), mlp_b1.detach().double().cpu() + w1 @ shift]
    for w, b in ((mlp_w2, mlp_b2), (red_w, red_b), (exp_w, exp_b)):
        w = w.detach().double().cpu().reshape(w.shape[0], -1)
        if tuple(w.shape) != (mid, mid) or b.numel() != mid:
            raise ValueError(f"pack_camera_gate: a [{mid}, {mid}] layer with {mid} biases, got {tuple(w.shape)}")
        parts += [w.t(), b.detach().double().cpu()]
    return torch.cat([p.contiguous().reshape(-1) for p in parts])


def pack_camera_gate(bn, depth_mlp, depth_se, context_mlp, context_se, device=None):
    """The fp32 block of bevops_lss_camera_gate for a DepthNet's `bn` (BatchNorm1d(27), frozen: its running statistics),
    `depth_mlp` / `context_mlp` (fc1, fc2) and `depth_se` / `context_se` (conv_reduce, conv_expand; 1 x 1 convolutions
    or linear layers).  Branch 0 = depth, 1 = context.  The fold is evaluated in float64 and rounded once:
    s = gamma / sqrt(var + eps), t = beta - mean s, W1[k][j] = fc1.w[j][k] s[k], b1[j] = fc1.b[j] + sum_k fc1.w[j][k] t[k]."""
    var, mean = bn.running_var.detach().double().cpu(), bn.running_mean.detach().double().cpu()
    gamma = bn.weight.detach().double().cpu() if bn.weight is not None else torch.ones_like(var)
    beta = bn.bias.detach().double().cpu() if bn.bias is not None else torch.zeros_like(var)
    scale = gamma / torch.sqrt(var + bn.eps)
    shift = beta - mean * scale
    blocks = [_branch_block(mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, se.conv_reduce.weight,
                            se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias, scale, shift)
              for mlp, se in ((depth_mlp, depth_se), (context_mlp, context_se))]
    mid = depth_mlp.fc1.weight.shape[0]
    packed = torch.cat(blocks).to(torch.float32)
    assert packed.numel() == 2 * mid * (3 * mid + GATE_INPUTS + 4)
    if device is None:
        device = depth_mlp.fc1.weight.device
    return packed.to(device).contiguous()


def _gate_tensors(bn, depth_mlp, depth_se, context_mlp, context_se):
    ts = [bn.running_mean, bn.running_var, bn.weight, bn.bias]
    for mlp, se in ((depth_mlp, depth_se), (context_mlp, context_se)):
        ts += [mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, se.conv_reduce.weight, se.conv_reduce.bias,
               se.conv_expand.weight, se.conv_expand.bias]
    return [t for t in ts if t is not None]


def camera_gate_packed(bn, depth_mlp, depth_se, context_mlp, context_se, build=True):
    """`pack_camera_gate` cached on the stamps of every tensor that enters it; rebuilt when one of them changes.
    build=False: None when missing or stale.  Never built inside a stream capture (RuntimeError)."""
    key = depth_mlp.fc1.weight
    ts = _gate_tensors(bn, depth_mlp, depth_se, context_mlp, context_se)
    stamps = tuple((id(t),) + _TensorCache._stamp(t) for t in ts)
    hit = _GATE_PACKED.get(key)
    if hit is not None and hit[0] == stamps:
        return hit[1]
    if not build:
        return None
    if key.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("lss_camera_gate: the packed gate parameters are missing or stale and the stream is capturing; "
                           "call camera_gate_packed(...) (or the model's prepare_bev_half) before the capture")
    packed = pack_camera_gate(bn, depth_mlp, depth_se, context_mlp, context_se)
    _GATE_PACKED.put(key, (stamps, packed))
    return packed


def lss_camera_gate(mlp_input, packed, mid, out=None):
    """mlp_input [n, 27] fp32 (rows may be strided, the 27 values contiguous), packed: `pack_camera_gate`'s block for
    `mid` channels -> gates [2, n, mid] fp32, gates[0] the depth branch's and gates[1] the context branch's
    sigmoid(expand(relu(reduce(fc2(relu(fc1(bn(v)))))))), all in fp32.  mid % 8 == 0, 8 <= mid <= 512 (else BevopsError
    NOT_SUPPORTED).  One launch."""
    if not (torch.is_tensor(mlp_input) and mlp_input.is_cuda and mlp_input.dtype == torch.float32):
        raise ValueError("lss_camera_gate: mlp_input an fp32 CUDA tensor")
    if mlp_input.dim() != 2 or mlp_input.shape[1] != GATE_INPUTS or mlp_input.stride(1) != 1:
        raise ValueError(f"lss_camera_gate: mlp_input [n, {GATE_INPUTS}] with contiguous rows, got {tuple(mlp_input.shape)}")
    mid = int(mid)
    if mid % 8 or not 8 <= mid <= 512:
        raise _lib.BevopsError("bevops_lss_camera_gate: mid % 8 == 0 and 8 <= mid <= 512", _lib.NOT_SUPPORTED)
    words = 2 * mid * (3 * mid + GATE_INPUTS + 4)
    if not (packed.is_cuda and packed.dtype == torch.float32 and packed.is_contiguous() and packed.numel() == words and
            packed.device == mlp_input.device):
        raise ValueError(f"lss_camera_gate: packed a contiguous fp32 block of {words} words on the input's device")
    n = mlp_input.shape[0]
    pitch = mlp_input.stride(0) if n > 1 else GATE_INPUTS
    if pitch < GATE_INPUTS:
        raise ValueError("lss_camera_gate: overlapping rows")
    if out is None:
        out = torch.empty((2, n, mid), dtype=torch.float32, device=mlp_input.device)
    elif tuple(out.shape) != (2, n, mid) or out.dtype != torch.float32 or not out.is_contiguous() or \
            out.device != mlp_input.device:
        raise ValueError(f"lss_camera_gate: out a contiguous fp32 {(2, n, mid)} tensor on the input's device")
    if n:
        _call("bevops_lss_camera_gate", mlp_input.device, mlp_input.data_ptr(), pitch, packed.data_ptr(), out.data_ptr(),
              n, mid)
    return out


def se_gate2_nhwc(x, gates, out_a=None, out_b=None):
    """x a channel slice [n, c, H, W] (fp16, channels-last), gates [2, n, c] fp32 contiguous ->
    (x * gates[0][:, :, None, None], x * gates[1][:, :, None, None]) as fp16: one fp32 product and one rounding per
    value, x read once, one launch.  out_a / out_b: channel slices to write into (new channels-last tensors without).
    c % 8 == 0."""
    _check_f16(x, "x")
    n, c, H, W = x.shape
    if not (torch.is_tensor(gates) and gates.is_cuda and gates.dtype == torch.float32 and gates.is_contiguous() and
            tuple(gates.shape) == (2, n, c) and gates.device == x.device):
        raise ValueError(f"se_gate2_nhwc: gates a contiguous fp32 {(2, n, c)} tensor on the input's device")
    if c % 8:
        raise _lib.BevopsError("bevops_se_gate2_nhwc: c % 8 == 0", _lib.NOT_SUPPORTED)
    xp = slice_pitch(x, "x")
    out_a = _dest(out_a, (n, c, H, W), x, "se_gate2_nhwc")
    out_b = _dest(out_b, (n, c, H, W), x, "se_gate2_nhwc")
    ap, bp = slice_pitch(out_a, "out_a"), slice_pitch(out_b, "out_b")
    if n and H * W:
        _call("bevops_se_gate2_nhwc", x.device, x.data_ptr(), xp, gates.data_ptr(), out_a.data_ptr(), ap, out_b.data_ptr(),
              bp, n, H * W, c)
    return out_a, out_b


def global_avgpool_nhwc(x, out=None):
    """x a channel slice [n, c, H, W] (fp16, channels-last) -> [n, c] fp16 = adaptive_avg_pool2d(x, 1): an fp32 sum in
    a fixed order (include/bevops.h), one IEEE division by H W, one rounding; two calls give equal bits.  out: [n, >= c]
    fp16 rows to write the first c columns of.  c % 8 == 0."""
    _check_f16(x, "x")
    n, c, H, W = x.shape
    if c % 8:
        raise _lib.BevopsError("bevops_global_avgpool_nhwc: c % 8 == 0", _lib.NOT_SUPPORTED)
    if H * W == 0:
        raise ValueError("global_avgpool_nhwc: an empty map has no mean")
    xp = slice_pitch(x, "x")
    if out is None:
        out = torch.empty((n, c), dtype=x.dtype, device=x.device)
    elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < c or out.dtype != x.dtype or out.device != x.device or \
            (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"global_avgpool_nhwc: out [n, >= c] fp16 rows on the input's device, got {tuple(out.shape)}")
    op = out.stride(0) if n > 1 else out.shape[1]
    if n:
        _call("bevops_global_avgpool_nhwc", x.device, x.data_ptr(), xp, out.data_ptr(), op, n, H * W, c)
    return out


def se_gate2_nhwc_q(x_q, scale_x, gates, scale_a, scale_b, out_a=None, out_b=None):
    """bevops_se_gate2_nhwc_s8: x_q an int8 channel slice [n, c, H, W] (real = q scale_x), gates [2, n, c] fp32
    contiguous -> (x * gates[0], x * gates[1]) as int8 slices requantised with scale_a / scale_b:
    q = clamp(rne(((float(q) * scale_x) * gate) * (1 / scale_out)), -127, 127), every step one fp32 product
    (include/bevops.h); a NaN gate leaves as -127.  x read once, one launch.  c % 16 == 0."""
    _check_s8(x_q, "x_q")
    n, c, H, W = x_q.shape
    if not (torch.is_tensor(gates) and gates.is_cuda and gates.dtype == torch.float32 and gates.is_contiguous() and
            tuple(gates.shape) == (2, n, c) and gates.device == x_q.device):
        raise ValueError(f"se_gate2_nhwc_q: gates a contiguous fp32 {(2, n, c)} tensor on the input's device")
    if c % 16:
        raise _lib.BevopsError("bevops_se_gate2_nhwc_s8: c % 16 == 0", _lib.NOT_SUPPORTED)
    sx, sa, sb = _scale(scale_x, "scale_x"), _scale(scale_a, "scale_a"), _scale(scale_b, "scale_b")
    xp = slice_pitch(x_q, "x_q")
    out_a = _dest(out_a, (n, c, H, W), x_q, "se_gate2_nhwc_q")
    out_b = _dest(out_b, (n, c, H, W), x_q, "se_gate2_nhwc_q")
    ap, bp = slice_pitch(out_a, "out_a"), slice_pitch(out_b, "out_b")
    if n and H * W:
        _call("bevops_se_gate2_nhwc_s8", x_q.device, x_q.data_ptr(), xp, sx, gates.data_ptr(), out_a.data_ptr(), ap, sa,
              out_b.data_ptr(), bp, sb, n, H * W, c)
    return out_a, out_b


def global_avgpool_nhwc_q(x_q, scale_x, out=None):
    """bevops_global_avgpool_nhwc_s8: x_q an int8 channel slice [n, c, H, W] (real = q scale_x) -> [n, c] fp16 =
    fp16((float(sum) * scale_x) / float(H W)) with the exact int32 sum over the map: independent of the summation order.
    out: [n, >= c] fp16 rows to write the first c columns of.  c % 16 == 0, H W <= 2^24."""
    _check_s8(x_q, "x_q")
    n, c, H, W = x_q.shape
    if c % 16 or H * W > 1 << 24:
        raise _lib.BevopsError("bevops_global_avgpool_nhwc_s8: c % 16 == 0 and H W <= 2^24", _lib.NOT_SUPPORTED)
    if H * W == 0:
        raise ValueError("global_avgpool_nhwc_q: an empty map has no mean")
    sx = _scale(scale_x, "scale_x")
    xp = slice_pitch(x_q, "x_q")
    if out is None:
        out = torch.empty((n, c), dtype=torch.float16, device=x_q.device)
    elif out.dim() != 2 or out.shape[0] != n or out.shape[1] < c or out.dtype != torch.float16 or \
            out.device != x_q.device or (out.shape[1] > 1 and out.stride(1) != 1):
        raise ValueError(f"global_avgpool_nhwc_q: out [n, >= c] fp16 rows on the input's device, got {tuple(out.shape)}")
    op = out.stride(0) if n > 1 else out.shape[1]
    if n:
        _call("bevops_global_avgpool_nhwc_s8", x_q.device, x_q.data_ptr(), xp, sx, out.data_ptr(), op, n, H * W, c)
    return out
