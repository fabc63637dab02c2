"""The float64 statement of bevops_dwsep_conv_f16 (csrc/dwsep_conv.hip) and the derived error bound of its SiLU flavour
(design/yolox_depthwise.md, "Bounds"), shared by test_dwsep_conv_gpu.py and test_yolox_depthwise_gpu.py."""
import torch
import torch.nn.functional as F

from test_conv_slice_gpu import silu64, silu_bound   # the fp32 SiLU / fp16 rounding terms derived there

ACT64 = {"none": lambda v: v, "relu": lambda v: v.clamp_min(0.0), "silu": lambda v: torch.from_numpy(silu64(v.numpy()))}
SILU_SLOPE = 1.1          # max |d silu / dv| = 1.0998 (at v = 2.3994)


def statement(x, wd, bd, wp, bp, act_dw, act_pw, res=None, stride=1):
    """x [B, C, H, W], wd [C, 1, 3, 3], wp [Co, C, 1, 1], biases or None, res [B, Co, Ho, Wo] or None (any dtype / device)
    -> float64 CPU (e, s, t, mag): e the unrounded output, s the pointwise sum + bias, t the fp16-rounded intermediate,
    mag = sum_c |t w_pw|."""
    f = lambda v: None if v is None else v.detach().double().cpu()     # noqa: E731
    t = ACT64[act_dw](F.conv2d(f(x), f(wd), f(bd), stride, 1, 1, x.shape[1])).half().double()     # ONE rounding of t
    s = F.conv2d(t, f(wp), f(bp))
    e = ACT64[act_pw](s) + (0.0 if res is None else f(res))
    return e, s, t, F.conv2d(t.abs(), f(wp).abs())


def ulp16(t):
    """The spacing of fp16 numbers at |t| (float64 tensor): 2^(max(floor(log2 |t|), -14) - 10)."""
    return torch.exp2((torch.frexp(t.abs())[1] - 1).clamp_min(-14).double() - 10.0)


def bound(e, s, t, mag, wp):
    """|got - e| allowed per output: conv_slice's SiLU + final rounding term; in front of act_pw (slope <= 1.1) one fp16
    ulp of every t[c] (a near tie flipped by the fp32 evaluation of stage 1) weighted by |w_pw|, and the fp32
    accumulation of Cin products."""
    flip = F.conv2d(ulp16(t), wp.detach().double().cpu().abs())
    return torch.from_numpy(silu_bound(s.numpy(), e.numpy())) + SILU_SLOPE * (flip + (t.shape[1] + 1) * 2.0 ** -24 * mag)
