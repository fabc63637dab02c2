#!/usr/bin/env python3
"""Golden vectors for qkv and inverse, made by the REFERENCE's own Python: det2trt/models/functions/multi_head_attn.py
(qkv: scale, matmul, softmax, matmul) and inverse.py (torch.linalg.inv), loaded by file path (both import only torch)
and run on the CPU in fp32.

Run in the build container only (needs the reference tree, see make_golden.py); the .npz files it writes are
committed so that no test reads the reference at run time:
    python tests/golden/make_qkv_inverse_golden.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import _load  # noqa: E402

# (B, Lq, Lkv, E): ragged lengths, every supported width class
QKV_CASES = [(2, 33, 47, 32), (1, 64, 64, 64), (3, 5, 130, 16), (1, 17, 9, 128)]


def well_conditioned(count, n, g, cond=20.0):
    """count random n x n matrices U diag(s) V^T with singular values from 1 down to 1 / cond (fp64 -> fp32)."""
    out = []
    for _ in range(count):
        u, _r = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
        v, _r = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
        s = torch.logspace(0, -np.log10(cond), n, dtype=torch.float64)
        out.append(u @ torch.diag(s) @ v.T)
    return torch.stack(out).float()


def make_qkv():
    mha = _load("det2trt/models/functions/multi_head_attn.py", "ref_multi_head_attn")
    g = torch.Generator().manual_seed(7)
    res = {"shapes": np.array(QKV_CASES, np.int32)}
    for i, (B, Lq, Lkv, E) in enumerate(QKV_CASES):
        q = torch.randn(B, Lq, E, generator=g)
        k = torch.randn(B, Lkv, E, generator=g)
        v = torch.randn(B, Lkv, E, generator=g)
        with torch.no_grad():
            out = mha.qkv(q, k, v)
        for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
            res[f"{name}{i}"] = t.numpy()
    np.savez_compressed(os.path.join(OUT, "qkv.npz"), **res)
    print("qkv", [tuple(c) for c in QKV_CASES])


def make_inverse():
    inv = _load("det2trt/models/functions/inverse.py", "ref_inverse")
    g = torch.Generator().manual_seed(8)
    perm = torch.eye(5)[torch.tensor([3, 0, 4, 1, 2])]
    cases = {
        "identity32": torch.eye(32).repeat(4, 1, 1),           # the reference test's input (test_inverse.py:19-21)
        "rand3": well_conditioned(8, 3, g),
        "rand4": well_conditioned(8, 4, g),
        "rand32": well_conditioned(4, 32, g),
        "perm5": perm[None],
    }
    res = {}
    for name, a in cases.items():
        with torch.no_grad():
            res["a_" + name], res["x_" + name] = a.numpy(), inv.inverse(a).numpy()
    np.savez_compressed(os.path.join(OUT, "inverse.npz"), **res)
    print("inverse", {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    torch.set_num_threads(4)
    make_qkv()
    make_inverse()
