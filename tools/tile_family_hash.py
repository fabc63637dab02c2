#!/usr/bin/env python3
"""Output bytes of the 128-row tile family (csrc/tile_mma.h and its five users) as SHA-256 hashes: one JSON line per case
and entry, on seeded Gaussian operands with general (non-dyadic) scales.  Two builds of the library compute the same
function bit for bit exactly when the two outputs of this script are equal line by line.

Entries: bevops_conv_slice_f16 / _ex, bevops_conv_slice_s8 / _ex / _ex2, bevops_deconv4x4s2_f16 / _s8, bevops_conv_tile_f16,
bevops_conv_tile_int8 -- called through the C ABI, not the Python wrappers, so that every entry is reached by its name.
Cases: the small shapes of the exact tests (M = 2 * 13 * 11 = 286 rows: three row tiles, the last one partial; a narrow
Cout of 48 and a wide one of 144 with a partial second column tile; Cin 96 for conv_slice_s8, K = 13.5 steps) and the
paths those tests bound without pinning their bits: SiLU with and without identity, int8 output with per-channel scales,
res_first, dilation 2 with a per-image bias.  Outputs are pitched (Cout + 16 channels) over a 0x5a fill and hashed whole:
a byte written outside the slice changes the hash.

The library comes from BEVOPS_LIB (utils/lib.py), else the package's own.

    BEVOPS_LIB=/path/to/libbevops_hip.so python tools/tile_family_hash.py [--out hash.jsonl]"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F16, I8 = 1, 2
ACTS = {"none": 0, "relu": 1, "silu": 2}
SCALE_A, SCALE_W, SCALE_RES = 0.0173, 0.0041, 0.0291


def load(path):
    """A ctypes handle of its own on `path` with the signatures of utils/lib.py (two paths: two copies of the library)."""
    import torch  # noqa: F401  (the HIP runtime torch ships is the one both sides use)
    from bevformer_tensorrt_amd.utils import lib as _lib
    handle = ctypes.CDLL(os.path.realpath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    return handle


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Case:
    """Operands of one layer, made once and shared by the entries (and the builds) that run it.  kind: "conv" (k, stride,
    dilation; rows = output pixels) or "deconv" (4 x 4 / 2: the packed parity-major weight, rows = input pixels)."""

    def __init__(self, kind, B, H, W, cin, cout, k=1, stride=1, dilation=1, seed=0, pitched=True):
        import torch
        self.kind, self.B, self.H, self.W, self.cin, self.cout = kind, B, H, W, cin, cout
        self.k, self.stride, self.dilation = k, stride, dilation
        g = torch.Generator().manual_seed(seed)
        dev = "cuda"
        rn = lambda *s: torch.randn(*s, generator=g)
        if kind == "conv":
            self.ho, self.wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
            self.kk = k * k * cin
            wshape = (cout, k, k, cin)
        else:
            self.ho, self.wo = 2 * H, 2 * W
            self.kk = 4 * cin
            wshape = (4, cout, 2, 2, cin)
        self.op = cout + 16 if pitched else cout   # elements between two output pixels
        self.x = rn(B, H, W, cin).half().to(dev)
        self.w = (rn(*wshape) / self.kk ** 0.5).half().to(dev)
        self.bias_h = rn(cout).half().to(dev)
        self.res_h = rn(B, self.ho, self.wo, cout).half().to(dev)
        self.ibias_h = rn(B, cout + 8).half().to(dev)
        q = lambda t: torch.clamp(torch.round(t), -127, 127).to(torch.int8).to(dev)
        self.x_q = q(rn(B, H, W, cin) * 30)
        self.w_q = q(rn(*wshape) * 30)
        self.res_q = q(rn(B, self.ho, self.wo, cout) * 30)
        self.wsc = (torch.rand(cout, generator=g) * 0.9 + 0.1).to(dev)
        self.bias_f = rn(cout).to(dev)
        # the requantisation scale: sums have a standard deviation near 900 sqrt(K); the outputs then fill the int8 range
        self.sum_std = 900.0 * self.kk ** 0.5

    def scale_out(self, wscales):
        return SCALE_A * SCALE_W * (0.55 if wscales else 1.0) * self.sum_std / 40.0

    def out(self, dtype):
        import torch
        return torch.full((self.B, self.ho, self.wo, self.op), 0x5a, dtype=torch.uint8, device="cuda").repeat_interleave(
            2 if dtype == F16 else 1, dim=3).view(torch.float16 if dtype == F16 else torch.int8)


def run(lib, c, entry, act="none", res=False, ibias=False, out_dtype=F16, wscales=True, res_first=False, out=None):
    """Launch `entry` of `lib` on case c on the current stream; returns the (pitched) output tensor."""
    s8 = entry.endswith("s8") or "_s8_" in entry or entry.endswith("int8")
    out = c.out(out_dtype if s8 else F16) if out is None else out
    wsc = c.wsc if wscales else None
    so = c.scale_out(wscales)
    fn = getattr(lib, entry)
    if entry in ("bevops_conv_slice_f16", "bevops_conv_slice_f16_ex"):
        head = (c.x.data_ptr(), c.cin, c.w.data_ptr(), _ptr(c.ibias_h if ibias else c.bias_h), _ptr(c.res_h if res else None),
                c.cout, out.data_ptr(), c.op, c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride, ACTS[act])
        if entry.endswith("_ex"):
            st = fn(*head, c.dilation, c.ibias_h.shape[1] if ibias else 0, _stream())
        else:
            st = fn(*head, _stream())
    elif entry.startswith("bevops_conv_slice_s8"):
        head = (c.x_q.data_ptr(), c.cin, SCALE_A, c.w_q.data_ptr(), _ptr(wsc), SCALE_W, _ptr(None if ibias else c.bias_f),
                _ptr(c.res_q if res else None), c.cout, SCALE_RES, out_dtype, out.data_ptr(), c.op, so, c.B, c.H, c.W, c.cin,
                c.cout, c.k, c.stride, ACTS[act])
        if entry.endswith("_ex2"):
            st = fn(*head, int(res_first), c.dilation, _ptr(c.ibias_h if ibias else None), c.ibias_h.shape[1] if ibias else 0,
                    _stream())
        elif entry.endswith("_ex"):
            st = fn(*head, int(res_first), _stream())
        else:
            st = fn(*head, _stream())
    elif entry == "bevops_deconv4x4s2_f16":
        st = fn(F16, c.x.data_ptr(), c.w.data_ptr(), c.bias_h.data_ptr(), out.data_ptr(), c.B, c.H, c.W, c.cin, c.cout, 4, 2, 1,
                int(act == "relu"), _stream())
    elif entry == "bevops_deconv4x4s2_s8":
        st = fn(c.x_q.data_ptr(), SCALE_A, c.w_q.data_ptr(), _ptr(wsc), SCALE_W, c.bias_f.data_ptr(), out_dtype, out.data_ptr(), so,
                c.B, c.H, c.W, c.cin, c.cout, int(act == "relu"), _stream())
    elif entry == "bevops_conv_tile_f16":
        st = fn(c.x.data_ptr(), c.w.data_ptr(), c.bias_h.data_ptr(), _ptr(c.res_h if res else None), out.data_ptr(), c.B, c.H, c.W,
                c.cin, c.cout, c.k, c.stride, int(act == "relu"), _stream())
    elif entry == "bevops_conv_tile_int8":
        st = fn(c.x_q.data_ptr(), SCALE_A, c.w_q.data_ptr(), _ptr(wsc), SCALE_W, c.bias_f.data_ptr(),
                _ptr(c.res_h if res else None), out_dtype, out.data_ptr(), so, c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride,
                int(act == "relu"), _stream())
    else:
        raise ValueError(entry)
    if st != 0:
        raise RuntimeError(f"{entry}: status {st}")
    return out


def cases():
    """(case description, Case kwargs, [(entry, run kwargs)])."""
    B, H, W = 2, 13, 11
    both = (F16, I8)
    for cout in (48, 144):
        # fp16 slices: every activation, the identity behind it; stride 2; dilation 2 with a per-image bias
        conv = dict(kind="conv", B=B, H=H, W=W, cin=64, cout=cout)
        yield dict(conv, k=3), [("bevops_conv_slice_f16", dict(act=a, res=r)) for a in ACTS for r in (False, True)]
        yield dict(conv, k=1), [("bevops_conv_slice_f16", dict(act="silu", res=True))]
        yield dict(conv, k=3, stride=2), [("bevops_conv_slice_f16", dict(act="silu")),
                                          ("bevops_conv_slice_f16_ex", dict(act="silu"))]
        yield dict(conv, k=3, dilation=2), [("bevops_conv_slice_f16_ex", dict(act="relu", ibias=ib, res=ib))
                                            for ib in (False, True)]
        # int8 slices at Cin 96 (a step straddles a tap, the last one is half empty)
        conv = dict(kind="conv", B=B, H=H, W=W, cin=96, cout=cout)
        yield dict(conv, k=3), \
            [("bevops_conv_slice_s8", dict(act=a, res=r, out_dtype=d, wscales=ws))
             for a in ACTS for r in (False, True) for d in both for ws in (True, False) if ws or a == "silu"] + \
            [("bevops_conv_slice_s8_ex", dict(act=a, res=True, res_first=True, out_dtype=d)) for a in ("none", "relu") for d in both] + \
            [("bevops_conv_slice_s8_ex", dict(act="silu", res=True, out_dtype=I8))]
        yield dict(conv, k=1, stride=2), [("bevops_conv_slice_s8", dict(act="silu", out_dtype=d)) for d in both]
        yield dict(conv, k=3, dilation=2), \
            [("bevops_conv_slice_s8_ex2", dict(act="relu", ibias=ib, res=ib, res_first=ib, out_dtype=d))
             for ib in (False, True) for d in both]
        # transposed convolutions
        dec = dict(kind="deconv", B=B, H=H, W=W, cin=64, cout=cout, pitched=False)
        yield dec, [("bevops_deconv4x4s2_f16", dict(act=a)) for a in ("none", "relu")] + \
            [("bevops_deconv4x4s2_s8", dict(act=a, out_dtype=d, wscales=ws)) for a in ("none", "relu") for d in both
             for ws in (True, False)]
        # the convolution mode of tile_gemm.hip
        til = dict(kind="conv", B=B, H=H, W=W, cin=64, cout=cout, pitched=False)
        for k, s in ((3, 1), (1, 2)):
            yield dict(til, k=k, stride=s), \
                [("bevops_conv_tile_f16", dict(act=a, res=r)) for a in ("none", "relu") for r in (False, True)] + \
                [("bevops_conv_tile_int8", dict(act="relu", res=r, out_dtype=d, wscales=ws))
                 for r in (False, True) for d in both for ws in (True, False) if not (r and d == I8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import torch
    from bevformer_tensorrt_amd.utils import lib as _lib
    lib = load(_lib.lib_path())
    lines = []
    for n, (kw, launches) in enumerate(cases()):
        c = Case(seed=n, **kw)
        for entry, rk in launches:
            out = run(lib, c, entry, **rk)
            torch.cuda.synchronize()
            raw = out.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            rec = {"entry": entry, "shape": {k: v for k, v in kw.items() if k != "kind"}, "args": rk, "bytes": len(raw),
                   "sha256": hashlib.sha256(raw).hexdigest()}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
