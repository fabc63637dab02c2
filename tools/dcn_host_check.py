#!/usr/bin/env python3
"""Do two builds of the DCNv2 host code compute and launch the same?  Calls every forward entry of LIB.so under every
accepted bevops_mdconv_set_variant value on seeded inputs, at one small shape per branch of the launch plan, and prints
one line per call: `entry  v=variant  shape  -> status  sha256(output buffer)[:16]`.  Two builds agree when their outputs are
equal line for line.  All inputs are made on the host; on the device the tool itself launches exactly one fill kernel
(of the output buffer) in front of every call (and a fill of bytes in front of its own weight packing), so a `rocprofv3 --kernel-trace --output-format csv` run of it splits into
calls at those fills (the runtime's copy kernels, which move the tool's inputs and outputs, are left out; its memset
kernel, the int8 ragged-K path's hipMemsetAsync, is listed):

    dcn_host_check.py --launches KERNEL_TRACE.csv CALLS.txt

prints the lines of CALLS.txt (a saved run), each followed by the launches the call made: kernel name, grid, block, LDS
bytes.

    dcn_host_check.py --group FILE

folds the lines of either output that differ only in the variant into one (`v=0,4,5`): the form kept under profiles/.

usage: dcn_host_check.py LIB.so        (needs a GPU)"""
import csv
import ctypes
import hashlib
import re
import sys

F32, F16, I8 = 0, 1, 2
VARIANTS = [0, 1, 2, 3, 4, 5, 6, 8, 9]
P, I, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

# name: Cin, Cout, H, W, G, DG -- B = 1, 3 x 3, stride 1, pad 1.  The branch each one targets:
FP_SHAPES = {
    "64>64@9x9": (64, 64, 9, 9, 1, 1),            # fused domain, narrow tiles (HW % 4 != 0: generic copy)
    "64>64@8x8": (64, 64, 8, 8, 1, 1),            # ... with the 4 x 4 transposing copy
    "64>64@8x8+2": (64, 64, 8, 8, 1, 1),          # input 2 bytes off 16-byte alignment: generic copy
    "64>64@7x9": (64, 64, 7, 9, 1, 1),            # HW % 4 != 0: generic copy
    "64>64@182x182": (64, 64, 182, 182, 1, 1),    # 259 tiles of 128 pixels on 256 slots: wide tiles, 3-tile split-K tail
    "64>320@182x182": (64, 320, 182, 182, 1, 1),  # two Cout tile rows: tail off
    "128>128@9x9g2dg2": (128, 128, 9, 9, 2, 2),   # group loop
    "128>64@9x9dg2": (128, 64, 9, 9, 1, 2),       # the group spans two deform groups: register-staged; nhwc answers 3
    "48>64@9x9": (48, 64, 9, 9, 1, 1),            # im2col + gemm_tn_f16
    "4>8@9x9": (4, 8, 9, 9, 1, 1),                # ragged K
}
F32_SHAPES = {"16>16@9x9": (16, 16, 9, 9, 1, 1)}
S8_SHAPES = {
    "128>64@182x182": (128, 64, 182, 182, 1, 1),  # LDS-DMA, wide, tail
    "128>64@9x9": (128, 64, 9, 9, 1, 1),          # the pair by default; the fused kernel under 8; LDS-DMA under 9
    "64>64@9x9": (64, 64, 9, 9, 1, 1),            # outside the LDS-DMA domain
    "4>8@9x9": (4, 8, 9, 9, 1, 1),                # Kp != Kg: the memset path
}


def calls():
    """(entry, shape name, geometry, options) in a fixed order"""
    for name, geo in FP_SHAPES.items():
        for entry in ("forward", "forward_packed"):
            yield entry, name, geo, dict(dtype=F16)
        if "+2" not in name:
            yield "forward_nhwc", name, geo, dict(dtype=F16, relu=0, om=0)
            yield "forward_nhwc", name, geo, dict(dtype=F16, relu=1, om=28)
    for name, geo in F32_SHAPES.items():
        yield "forward", name, geo, dict(dtype=F32)
    for name, geo in S8_SHAPES.items():
        for entry in ("forward_int8", "forward_int8_packed"):
            yield entry, name, geo, dict(dtype=I8)
    for name in ("128>64@182x182", "128>64@9x9"):
        for exact in (1, 0):
            for relu in (0, 1):
                yield "forward_int8_nhwc", name, S8_SHAPES[name], dict(dtype=I8, exact=exact, relu=relu, om=32)


def run(lib_path):
    import torch
    lib = ctypes.CDLL(lib_path)
    lib.bevops_mdconv_workspace_size.restype = lib.bevops_mdconv_packed_weight_size.restype = SZ
    lib.bevops_mdconv_int8_nhwc_workspace_size.restype = SZ
    dev = torch.device("cuda:0")
    tdt = {F32: torch.float32, F16: torch.float16, I8: torch.int8}

    def up(t, shift=0):
        """host tensor -> device (a copy, no kernel); shift: elements the device copy starts off its allocation"""
        buf = torch.empty(t.numel() + shift, dtype=t.dtype, device=dev)
        buf[shift:].copy_(t.reshape(-1))     # host -> device copy
        return buf[shift:]

    for idx, (entry, name, (Cin, Cout, H, W, G, DG), o) in enumerate(calls()):
        g = torch.Generator().manual_seed(1000 + idx)
        dt, nhwc, s8 = o["dtype"], entry.endswith("nhwc"), o["dtype"] == I8
        geo = (1, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1, 1, 1, G, DG)
        n_off, n_mask = DG * 18 * H * W, DG * 9 * H * W
        if s8:
            x = torch.randint(-127, 128, (Cin * H * W,), generator=g, dtype=torch.int8)
            w = torch.randint(-127, 128, (Cout * (Cin // G) * 9,), generator=g, dtype=torch.int8)
            off = torch.randint(-127, 128, (n_off,), generator=g, dtype=torch.int8)
            mask = torch.randint(0, 128, (n_mask,), generator=g, dtype=torch.int8)
            bias = torch.randn(Cout, generator=g)
        else:
            x = torch.randn(Cin * H * W, generator=g).to(tdt[dt])
            w = (torch.randn(Cout * (Cin // G) * 9, generator=g) / (Cin // G * 9) ** 0.5).to(tdt[dt])
            off = (torch.randn(n_off, generator=g) * 2).to(tdt[dt])
            mask = torch.rand(n_mask, generator=g).to(tdt[dt])
            bias = torch.randn(Cout, generator=g).to(tdt[dt])
        if o.get("om"):     # raw channels-last output of the offset convolution: fp16 [Ho, Wo, om] (also for int8)
            off, mask = (torch.randn(H * W * o["om"], generator=g) * 2).half(), None
        x_d = up(x, 1 if "+2" in name else 0)
        w_d, off_d, bias_d = up(w), up(off), up(bias)
        mask_d = up(mask) if mask is not None else None
        out = torch.empty(Cout * H * W, dtype=tdt[dt], device=dev)
        if entry == "forward_int8_nhwc":
            ws_bytes = lib.bevops_mdconv_int8_nhwc_workspace_size()
        else:
            ws_bytes = lib.bevops_mdconv_workspace_size(I(dt), *map(I, geo))
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        packed = torch.empty(max(lib.bevops_mdconv_packed_weight_size(I(dt), I(Cout), I(Cin // G), I(3), I(3)), 16),
                             dtype=torch.uint8, device=dev)
        ptr = lambda t: P(t.data_ptr()) if t is not None else None
        packed.fill_(0)                         # a fill of BYTES: what follows is the tool's own packing, not a call
        lib.bevops_mdconv_pack_weight(I(dt), ptr(w_d), ptr(packed), I(Cout), I(Cin // G), I(3), I(3), None)
        for v in VARIANTS:
            lib.bevops_mdconv_set_variant(v)
            out.fill_(1)                        # the ONE kernel of the tool's own per call (see --launches)
            wp = ptr(w_d) if entry in ("forward", "forward_int8") else ptr(packed)
            tail = [ptr(ws), SZ(ws_bytes)] + [I(a) for a in geo] + [None]
            sc = [F(0.02), F(0.03), F(1 / 127), F(0.01), F(0.05)]   # in, offset, mask, weight, out
            fn = getattr(lib, "bevops_mdconv_" + entry)
            if entry == "forward_nhwc":
                st = fn(I(dt), ptr(x_d), ptr(off_d), ptr(mask_d), wp, ptr(bias_d), ptr(out), I(o["relu"]), I(o["om"]), *tail)
            elif entry == "forward_int8_nhwc":
                st = fn(ptr(x_d), sc[0], ptr(off_d), I(o["om"]), sc[1], sc[2], wp, sc[3], ptr(bias_d), ptr(out), sc[4],
                        I(o["relu"]), I(o["exact"]), *tail)
            elif s8:
                st = fn(ptr(x_d), sc[0], ptr(off_d), sc[1], ptr(mask_d), sc[2], wp, sc[3], ptr(bias_d), ptr(out), sc[4], *tail)
            else:
                st = fn(I(dt), ptr(x_d), ptr(off_d), ptr(mask_d), wp, ptr(bias_d), ptr(out), *tail)
            torch.cuda.synchronize()
            opts = " ".join(f"{k}={o[k]}" for k in ("relu", "om", "exact") if k in o)
            digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
            print(f"{entry}  v={v}  {name}{' ' + opts if opts else ''}  -> {st}  {digest}", flush=True)
    lib.bevops_mdconv_set_variant(0)


def launches(trace_csv, calls_txt):
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Start_Timestamp"]))
    lines = [ln for ln in open(calls_txt).read().splitlines() if "  -> " in ln]
    segs, own = [], True
    for r in rows:
        kern = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        if "FillFunctor<unsigned char>" in kern:
            own = True                          # the tool packs weights: not a call
        elif "FillFunctor" in kern:
            segs.append([])                     # the tool's fill of the output buffer: a new call begins
            own = False
        elif not own and "rocclr_copyBuffer" not in kern:
            dims = lambda k: re.sub(r"(x1)+$", "", "x".join(r[f"{k}_{a}"] for a in "XYZ"))
            name = re.sub(r"^void |bevops::", "", kern).split("(")[0]
            segs[-1].append(f"{name} grid={dims('Grid_Size')} block={dims('Workgroup_Size')} lds={r['LDS_Block_Size']}")
    assert len(segs) == len(lines), f"{len(segs)} fills in the trace, {len(lines)} calls in {calls_txt}"
    for ln, seg in zip(lines, segs):
        print(ln, "|", "; ".join(seg) if seg else "no launch")


def group(path):
    by = {}
    for ln in open(path).read().splitlines():
        entry, v, rest = ln.split("  ", 2)
        by.setdefault((entry, rest), []).append(v[2:])
    for (entry, rest), vs in by.items():
        print(f"{entry}  v={','.join(vs)}  {rest}")


if __name__ == "__main__":
    if sys.argv[1] == "--launches":
        launches(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "--group":
        group(sys.argv[2])
    else:
        run(sys.argv[1])
