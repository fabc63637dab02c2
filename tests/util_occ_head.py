"""The float64 statement of bevops_occ_head_f16 (csrc/occ_head.hip), the derived per-logit bound of design/flashocc.md
("Error bound") and the operands of its tests, shared by test_occ_head_cpu.py, test_occ_head_gpu.py and
test_flashocc_gpu.py."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SOFTPLUS_ERR = 2.0 ** -20      # |kernel's fp32 Softplus - exact| <= SOFTPLUS_ERR max(1, softplus): measured 1.7e-7, x 5.6
U16, U32 = 2.0 ** -11, 2.0 ** -23     # fp16 half-ulp (RNE); one fp32 ulp per accumulation step (order and rounding unstated)
EXACT_CASES = ((32, 64, 1, 2), (64, 128, 3, 18), (256, 512, 16, 18))       # (C, Hd, Dz, Ncls)
GENERAL_CASES = ((64, 128, 3, 18), (256, 128, 16, 18))
MAX_ROWS = 300


def softplus_f32(v):
    """The kernel's formula in numpy float32: v above 20, else ln2 log2(1 + exp2(v log2e))."""
    v = np.asarray(v, dtype=np.float32)
    s = np.float32(0.69314718055994530942) * np.log2(np.float32(1) + np.exp2(np.minimum(v, np.float32(20)) * np.float32(1.44269504088896340736)))
    return np.where(v > 20, v, s)


def statement(y, W1, b1, W2, b2, Dz, Ncls):
    """Rows y [rows, C] -> float64 (occ [rows, Dz] int64 with ties to the LOWEST class, logits [rows, Dz Ncls], v, h)."""
    y, W1, b1, W2, b2 = (t.detach().double().cpu() for t in (y, W1, b1, W2, b2))
    v = y @ W1.t() + b1
    h = torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp_max(20.0))))
    lg = h @ W2.t() + b2
    vox = lg.view(-1, Dz, Ncls)
    cls = torch.arange(Ncls).expand_as(vox)
    return torch.where(vox == vox.amax(-1, keepdim=True), cls, Ncls).amin(-1), lg, v, h


def bound(y, W1, b1, W2, b2, lg, h):
    """Per-logit |fp16 logit - float64 logit| allowed, from the operation order (design/flashocc.md): the hidden value's
    error (fp32 accumulation of C products in front of a slope <= 1, the Softplus evaluation, ONE fp16 rounding) weighted
    by |W2|, the fp32 accumulation of Hd products, the output's fp16 rounding."""
    y, W1, b1, W2, b2 = (t.detach().double().cpu() for t in (y, W1, b1, W2, b2))
    dv = (W1.shape[1] + 1) * U32 * (y.abs() @ W1.abs().t() + b1.abs())
    dh = dv + SOFTPLUS_ERR * h.clamp_min(1.0)
    dh = dh + U16 * (h + dh) + 2.0 ** -25
    e = dh @ W2.abs().t() + (W2.shape[1] + 2) * U32 * ((h + dh) @ W2.abs().t() + b2.abs())
    return e + U16 * (lg.abs() + e) + 2.0 ** -25


def decided(lg, eps, Dz, Ncls):
    """bool [rows, Dz]: voxels whose float64 top-two gap exceeds twice the largest bound among their classes."""
    top = lg.view(-1, Dz, Ncls).topk(min(2, Ncls), -1).values
    gap = top[..., 0] - top[..., -1] if Ncls > 1 else torch.full_like(top[..., 0], float("inf"))
    return gap > 2.0 * eps.view(-1, Dz, Ncls).amax(-1)


@functools.lru_cache(maxsize=None)
def exact_operands(C, Hd, Dz, Ncls):
    """Integer operands of the exact chain: y in {-1, 0, 1}, W1 eight +-1 per row, b1 in [29, 33] (every pre-activation
    an integer in [21, 41]: Softplus is the identity, h an exact fp16), W2 sixteen +-1 per row, b2 in [-8, 8] (|logit|
    <= 16 * 41 + 8 = 664).  In every EVEN voxel class c + Ncls // 2 repeats class c's row and bias: its maximum is tied."""
    g = torch.Generator().manual_seed(C + Hd + 7 * Dz + Ncls)
    y = torch.randint(-1, 2, (MAX_ROWS, C), generator=g).half()

    def sparse(rows, cols, nnz):
        w = torch.zeros(rows, cols)
        for r in range(rows):
            idx = torch.randperm(cols, generator=g)[:nnz]
            w[r, idx] = torch.randint(0, 2, (nnz,), generator=g).float() * 2 - 1
        return w

    W1, b1 = sparse(Hd, C, 8).half(), torch.randint(29, 34, (Hd,), generator=g).half()
    W2, b2 = sparse(Dz * Ncls, Hd, 16), torch.randint(-8, 9, (Dz * Ncls,), generator=g).float()
    half = Ncls // 2
    for z in range(0, Dz, 2):
        W2[z * Ncls + half:z * Ncls + 2 * half] = W2[z * Ncls:z * Ncls + half]
        b2[z * Ncls + half:z * Ncls + 2 * half] = b2[z * Ncls:z * Ncls + half]
    return (y, W1, b1, W2.half(), b2.half()), statement(y, W1, b1, W2, b2, Dz, Ncls)


@functools.lru_cache(maxsize=None)
def general_operands(C, Hd, Dz, Ncls):
    """Gaussian operands: pre-activations of standard deviation ~2 around the Softplus knee, logits of spread ~1."""
    g = torch.Generator().manual_seed(3 * C + Hd + Dz)
    n = lambda *s: torch.randn(s, generator=g)                                                        # noqa: E731
    ops = (n(MAX_ROWS, C).half(), (2.0 * n(Hd, C) / C ** 0.5).half(), (0.5 * n(Hd)).half(),
           (n(Dz * Ncls, Hd) / Hd ** 0.5).half(), (0.5 * n(Dz * Ncls)).half())
    occ, lg, v, h = statement(*ops, Dz, Ncls)
    eps = bound(*ops, lg, h)
    return ops, (occ, lg, v, h), eps, decided(lg, eps, Dz, Ncls)


def plain64(y, W1, b1, W2, b2, Dz, Ncls):
    """functions.occ_head_plain in float64 on rows -> (occ [rows, Dz], logits)."""
    from bevformer_tensorrt_amd.functions import occ_head_plain
    occ, lg = occ_head_plain(y.double().t().reshape(1, y.shape[1], 1, -1), W1, b1, W2, b2, Dz, Ncls, logits=True)
    return occ[0, 0], lg[0, 0]
