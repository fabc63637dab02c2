"""The float64 statement of bevops_lss_depth_head_f16 (csrc/depth_head.hip), the derived bounds of design/depth_head.md
("Error bound") and the seeded operands of its tests, shared by test_depth_head_cpu.py and test_depth_head_gpu.py."""
import numpy as np
import torch

U16, U32, FLOOR = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
# relative error of exp / sum / divide in fp32 on given fp32 logits: 4 x what a numpy float32 restatement shows against
# float64 over these tests' logit range (test_depth_head_cpu.py::test_the_fp32_softmax_term_is_measured holds the factor)
T = 2.0 ** -18
CASES = [(32, 8, 1), (64, 64, 59), (256, 64, 88), (96, 80, 118), (512, 128, 128), (32, 8, 248)]   # (Cin, C, D)


def operands(Cin, C, D, rows, seed=0):
    """x [rows, Cin], weight [D + C, Cin] (depth rows first) and bias [D + C] in fp16: unit Gaussian x, weights scaled so
    that the logits have standard deviation 2 (they span a few units), unit Gaussian bias."""
    g = torch.Generator().manual_seed(seed + 1000 * Cin + D)
    x = torch.randn(rows, Cin, generator=g).half()
    W = (torch.randn(D + C, Cin, generator=g) * (2.0 / Cin ** 0.5)).half()
    return x, W, torch.randn(D + C, generator=g).half()


def statement(x, W, b, D, C):
    """float64 from the fp16 operands -> (feat [rows, C], depth [rows, D], eps_feat, eps_depth): the derived bounds
    |feat| <= (Cin + 1) u32 (sum |x W| + |b|) + u16 |v| + 2^-25 and
    |depth| <= p (2 max_d dv + T) + u16 p + 2^-25 with dv the logit bound (the first term above)."""
    x, W, b = (t.double().numpy() for t in (x, W, b))
    v = x @ W.T + b
    dv = (x.shape[1] + 1) * U32 * (np.abs(x) @ np.abs(W).T + np.abs(b))
    z = v[:, :D]
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    f = v[:, D:D + C]
    return f, p, dv[:, D:D + C] + U16 * np.abs(f) + FLOOR, p * (2 * dv[:, :D].max(1, keepdims=True) + T) + U16 * p + FLOOR
