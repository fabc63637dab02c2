"""Which implementation runs a dense layer (functions/linear.py: dense_auto) or a plain convolution (functions/conv.py:
conv3x3_auto): the two per-thread mode flags, the shipped table, BEVOPS_DENSE_TUNE, the rules, the measurement, the
process caches / logs / miss lists, and one pure function per family that turns all of these into a choice
(design/dense.md, "Dispatch: who decides").  The candidates themselves -- the ctypes wrappers -- stay in linear.py
(`_DENSE`) and conv.py (`_CONV`); both modules re-export the names below that tests and tools read there."""
import contextlib
import json
import os
import threading

import torch

from ..utils import lib as _lib


class _PerThreadFlag(threading.local):
    """`flag["enabled"]` with one value per THREAD (two frame runners on two threads -- a sharded and a plain one --
    must not see each other's setting; advisor, round 4).  Dict-style access, default False."""
    enabled = False

    def __getitem__(self, key):
        assert key == "enabled"
        return self.enabled

    def __setitem__(self, key, value):
        assert key == "enabled"
        self.enabled = bool(value)


# Rule mode: no per-process timing, no table: the choice is a function of the problem alone and falls on the hand-written
# kernels (fixed summation order, no library heuristic).  The camera-sharded frame loop switches it on: ranks that each
# measured their own winner would evaluate the REPLICATED layers (TSA, FFN, decoder) in different summation orders and
# drift apart bitwise.  No value of BEVOPS_DENSE_TUNE selects this mode (see _tune).
DETERMINISTIC = _PerThreadFlag()
# The hand-written kernels only, the FASTEST of them per problem by the shipped table's own measurements (the rule of
# DETERMINISTIC for a problem the table has not seen): what the model runs behind its backbone (bevformer.py:
# _OWN_ENCODER) -- one kernel per layer, summation order a function of the block index, same choice in every process.
# Dense layers only; DETERMINISTIC wins where both are set.
OWN_KERNELS = _PerThreadFlag()


@contextlib.contextmanager
def using(rule=None, own=None):
    """DETERMINISTIC (`rule`) and / or OWN_KERNELS (`own`) set to the given value for the calling thread inside the
    block, and both as they were after it; None leaves a flag alone."""
    was = DETERMINISTIC["enabled"], OWN_KERNELS["enabled"]
    DETERMINISTIC["enabled"], OWN_KERNELS["enabled"] = (was[0] if rule is None else rule), (was[1] if own is None else own)
    try:
        yield
    finally:
        DETERMINISTIC["enabled"], OWN_KERNELS["enabled"] = was


def _tune():
    """BEVOPS_DENSE_TUNE, read HERE and nowhere else -- by _table once, at the first table load of the process ("0" or
    "1": the table is NOT loaded, so every problem is unseen and OWN_KERNELS decides by the DETERMINISTIC rule), and by the
    two choices on every call that meets an unseen problem ("0": not measured, the no-measurement default -- mostly
    LIBRARY kernels, not the rule mode; otherwise measured once per process).  design/dense.md has the table."""
    return os.environ.get("BEVOPS_DENSE_TUNE", "")


# Shipped choices (bevformer_tensorrt_amd/dispatch_gfx950.json, written by tools/dump_dispatch.py from one MI355X's
# measurements): a problem found there takes its recorded winner WITHOUT a measurement, so the kernel that runs is the
# same on every box and in every process; only problems the table has never seen are timed.
_TABLE = {"loaded": False, "dense": {}, "conv": {}, "measured_dense": {}}


def _table(state=_TABLE):
    """The shipped table, loaded on the first call of the process into `state`."""
    if not state["loaded"]:
        state["loaded"] = True
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dispatch_gfx950.json")
        if os.path.exists(path) and _tune() not in ("0", "1"):
            try:
                t = json.load(open(path))
                state["dense"], state["conv"] = t.get("dense", {}), t.get("conv", {})
                state["measured_dense"] = t.get("measured_us", {}).get("dense", {})
            except (OSError, ValueError):
                pass
    return state


def _problem(key):
    return ",".join(str(int(v)) if isinstance(v, bool) else str(v) for v in key[1:])   # without the device name


_OWN = ("tile", "tsgemm", "small")
_DENSE_NAMES = _OWN + ("blaslt", "torch")     # the keys of linear._DENSE (tests/test_host_logic_cpu.py pins the set)
_CONV_NAMES = ("tile", "library", "halo")     # ... and of conv._CONV
_DENSE_CHOICE = {}     # problem -> name of the implementation the table lists or this process measured fastest
DENSE_LOG = []         # (problem, {name: us}) of every measurement, for tools / profiles
DENSE_MISSES = []      # problems dense_auto met that dispatch_gfx950.json does not list (measured or defaulted instead)
_CHOICE = {}           # the same three for conv3x3_auto: problem -> "tile" | "halo" | "library"
CONV_LOG = []
CONV_MISSES = []


def _small_pays(M, N, K):
    """The no-pipeline few-row GEMM is for problems of a few tiles (the decoder's 900 object queries); the shipped
    table's own measurements show it 2-3 x slower than the tiled kernels once M x N grows (2 250 x 2 048 x 512: 33.8
    against 18.0 us)."""
    return K % 64 == 0 and K <= 1024 and M * N <= 1024 * 512


def _dense_deterministic(N, K, M=1 << 30):
    if _small_pays(M, N, K):
        return "small"
    return "tsgemm" if (N % 256 == 0 and K % 64 == 0 and K >= 256) else "tile"


def _dense_own(key, N, K, M, table=None):
    times = (table or _table()).get("measured_dense", {}).get(_problem(key), {})
    own = {k: v for k, v in times.items() if k in _OWN}
    return min(own, key=own.get) if own else _dense_deterministic(N, K, M)


def own_kernel_choice(device, M, N, K, relu, has_bias, has_res):
    """The implementation dense_auto runs for this problem under OWN_KERNELS (a function of the problem and the shipped
    table alone).  The model's merged launches ask it: they replace a per-layer GEMM only where that GEMM runs on
    tile_gemm or tsgemm -- tile_gemm and the weight-stationary tsgemm (tsgemm_weight_stationary) share matrix
    instruction, k order and epilogue arithmetic and give the same bits (tests/test_gemm_grouped_gpu.py); the original
    tsgemm kernel rotates its k start by block index, small_gemm splits K inside the block: neither does."""
    return _dense_own((str(device), M, N, K, bool(relu), bool(has_bias), bool(has_res)), N, K, M)


def _dense_default(N, K, has_res):
    """Choice without a measurement (inside stream capture before the problem was seen, or BEVOPS_DENSE_TUNE=0)."""
    if N == 256 and K % 64 == 0 and K >= 256:
        return "tsgemm"
    return "blaslt"


def _ask(value):
    return value() if callable(value) else value


def dense_choice(key, rule, own, capturing, tune, table, cached=None):
    """-> (name | "measure", keep, miss): what dense_auto runs for the problem `key` = (device, M, N, K, relu, has_bias,
    has_res); `keep`: the answer goes to the process cache (after the measurement, for "measure"); `miss`: the problem goes
    to DENSE_MISSES.  `rule` / `own`: the two flags; `cached`: the process cache's answer for the key.  `capturing` (is the
    stream capturing) and `tune` (BEVOPS_DENSE_TUNE) may each be the value or a function that tells it, asked only where
    the choice depends on it.  A function of its arguments alone."""
    _, M, N, K, _, _, has_res = key
    if rule and K % 8 == 0:
        return _dense_deterministic(N, K, M), False, False
    if own and K % 8 == 0:
        return _dense_own(key, N, K, M, table), False, False
    if cached is not None:
        return cached, False, False
    name = table["dense"].get(_problem(key))
    if name in _DENSE_NAMES:
        return name, True, False
    if _ask(capturing) or _ask(tune) == "0" or M < 64:
        return ("small" if _small_pays(M, N, K) else _dense_default(N, K, has_res)), False, True
    return "measure", True, True


def halo_ok(key, halo):
    """64 -> 64 channels, 3x3, stride 1, no identity rows (conv2 of the ResNet stage-1 bottlenecks): the LDS-resident
    kernel (csrc/conv_halo.hip) -- bit-identical to the tiled implicit GEMM, so also the rule-based dispatch may take it"""
    _, _, _, _, Cin, Cout, k, stride, _, has_res = key
    return bool(halo) and Cin == 64 and Cout == 64 and stride == 1 and not has_res and k == 3


def conv_choice(key, rule, capturing, tune, table, halo, cached=None):
    """dense_choice for conv3x3_auto: `key` = (device, B, H, W, Cin, Cout, k, stride, relu, has_res), `halo` = HALO's
    setting.  OWN_KERNELS does not bear on convolutions."""
    Cin = key[4]
    if rule and Cin % 32 == 0:
        return ("halo" if halo_ok(key, halo) else "tile"), False, False
    if cached is not None:
        return cached, False, False
    name = table["conv"].get(_problem(key))     # shipped choice: no measurement, the same kernel on every box
    if name == "tile" and halo_ok(key, halo):
        # (the table was measured before this kernel existed: 47 against 88 us at the base shape, faster at every
        # shape of the four models, profiles/r06/conv_halo_time.jsonl)
        name = "halo"
    if name in _CONV_NAMES and (name == "library" or Cin % 32 == 0) and (name != "halo" or halo_ok(key, halo)):
        return name, True, False
    if Cin % 32 != 0:
        return "library", True, True
    if _ask(capturing) or _ask(tune) == "0":
        return "library", False, True
    return "measure", True, True


def graph_time_us(fn, iters=8, rounds=3):
    """Microseconds per call of `fn` on the device, measured under HIP-graph replay: `iters` calls are captured once
    and the replay is timed between two events (best of `rounds`).  Launching the same calls eagerly measures the HOST
    for anything shorter than the ~12 us a Python operator wrapper takes per call -- the decoder's few-row layers all
    looked alike (12-13 us) that way, whatever the kernel did."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    best = float("inf")
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / iters)
    return best


def measure(candidates, call, iters, rounds):
    """{name: microseconds per call} of `call(name)` for every candidate inside its domain: two warm-up calls each, one
    device synchronisation, then graph_time_us.  BLOCKING."""
    times = {}
    for name in candidates:
        try:
            for _ in range(2):
                call(name)
            times[name] = float("inf")
        except _lib.BevopsError as exc:   # outside the candidate's domain / no library algorithm -- and only that:
            if exc.status != _lib.NOT_SUPPORTED:      # a launch failure must not be mistaken for "not applicable"
                raise
    torch.cuda.synchronize()
    for name in times:
        times[name] = graph_time_us(lambda: call(name), iters, rounds)
    return times
