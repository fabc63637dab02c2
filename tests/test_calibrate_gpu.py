"""PTQ calibration on the device: bevops_calib_collect / bevops_calib_threshold (csrc/calibrate.hip), the *_device
calibrators of quantization.py, the calibration cache and the INT8 engine built through them.

Reference of every histogram test: tests/util_calibrate.py (numpy binning, Python-integer merge); of every threshold
test: quantization.entropy_threshold_bin / PercentileCalibrator's rule on the host.  All comparisons of the state are
exact (histogram, the bits of range and amax, count, nonfinite, batches)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import util_calibrate as U
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

MiB = 1 << 20
DTYPES = {"fp32": torch.float32, "fp16": torch.float16}


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def unpack(state):
    from bevformer_tensorrt_amd.quantization import unpack_calibration_states
    return unpack_calibration_states(state.detach().cpu().numpy().reshape(-1, U.STATE_BYTES))


def offset_by_one(values, dtype):
    """The values on the device with the base pointer one element past a 16-byte boundary (the vector path then has a
    head), and the same values as the host sees them (numpy, in `dtype`)."""
    host = torch.as_tensor(np.asarray(values)).to(dtype)
    raw = torch.empty(host.numel() + 1, dtype=dtype, device="cuda")
    x = raw[1:]
    x.copy_(host)
    assert x.data_ptr() % 16 == host.element_size()
    return x, host.numpy()


def collect_guarded(batches, dtype):
    """Every batch into one fresh state carved from the guarded arena at exactly 64-byte alignment, under both poisons;
    returns the unpacked fields (identical under both poisons, which is asserted)."""
    from bevformer_tensorrt_amd.functions import calib_collect, calib_state_size
    seen = []
    for poison in POISONS:
        arena = Arena(1 * MiB, poison)
        state = arena.carve(calib_state_size(), 64, "state")
        state.zero_()
        for b in batches:
            calib_collect(b, state)
        arena.check()
        seen.append(unpack(state))
    for k in seen[0]:
        assert np.array_equal(seen[0][k], seen[1][k]), f"{k} differs between the two poisons"
    return seen[0]


def expect_equal(got, ref):
    g, r = U.describe(got), U.describe(ref.fields())
    for name, a, b in zip(("range bits", "amax bits", "batches", "count", "nonfinite"), g, r):
        assert a == b, f"{name}: device {a}, reference {b}"
    bad = [(k, a, b) for k, (a, b) in enumerate(zip(g[5], r[5])) if a != b]
    assert not bad, f"{len(bad)} bins differ, first (bin, device, reference): {bad[:4]}"


# ---- bevops_calib_collect
@pytest.mark.parametrize("count", [1, 7, 63, 64, 65, 255, 4099, (1 << 20) + 5])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_collect_sizes_and_alignment(dtype, count):
    g = np.random.default_rng(count)
    x, host = offset_by_one(g.standard_normal(count).astype(np.float32), DTYPES[dtype])
    expect_equal(collect_guarded([x], DTYPES[dtype]), U.RefState().collect(host))


def _contents(name, dtype):
    g = np.random.default_rng(7)
    n = 4099
    if name == "randn":
        return [g.standard_normal(n)]
    if name == "relu":
        return [np.maximum(g.standard_normal(3 * n), 0.0)]
    if name == "zeros":
        return [np.zeros(n)]
    if name == "edges":      # range 32: every edge k / 64 is a binary16 number
        return [np.concatenate([np.arange(2048) * (32.0 / 2048), [32.0]])]
    if name == "edges_after_doubling":
        return [np.array([16.0, 0.25]), np.concatenate([np.arange(2048) * (32.0 / 2048), [32.0]])]
    if name == "subnormals":
        tiny = 2.0 ** -24 if dtype == "fp16" else 2.0 ** -149
        return [np.arange(0, 1024, dtype=np.float64) * tiny, np.array([0.0, tiny, 3 * tiny, -5 * tiny])]
    if name == "nonfinite_sprinkled":
        v = g.standard_normal(n)
        v[::97] = np.nan
        v[5::131] = np.inf
        v[11::211] = -np.inf
        return [v, np.maximum(v, 0.0)]
    if name == "nonfinite_only_then_data":
        return [np.array([np.nan, np.inf, -np.inf] * 50), g.standard_normal(n), np.array([np.nan] * 65)]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["randn", "relu", "zeros", "edges", "edges_after_doubling", "subnormals",
                                  "nonfinite_sprinkled", "nonfinite_only_then_data"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_collect_contents(dtype, name):
    pairs = [offset_by_one(v.astype(np.float32), DTYPES[dtype]) for v in _contents(name, dtype)]
    ref = U.RefState()
    for _, host in pairs:
        ref.collect(host)
    got = collect_guarded([x for x, _ in pairs], DTYPES[dtype])
    expect_equal(got, ref)
    if name == "zeros":
        assert got["range"][0] == np.float32(1e-12) and int(got["hist"][0, 0]) == 4099
    if name == "edges":
        assert int(got["hist"][0, 2047]) == 2 and int(got["hist"][0, :2047].max()) == 1   # range itself lands in bin 2047
    if name == "nonfinite_only_then_data":
        assert int(got["batches"][0]) == 3 and int(got["nonfinite"][0]) == 150 + 65


def test_collect_nonfinite_only_batch_leaves_the_state():
    from bevformer_tensorrt_amd.functions import calib_collect, calib_state_size
    g = np.random.default_rng(3)
    x, _ = offset_by_one(g.standard_normal(777).astype(np.float32), torch.float32)
    bad, _ = offset_by_one(np.array([np.nan, -np.inf] * 40, dtype=np.float32), torch.float32)
    state = torch.zeros(calib_state_size(), dtype=torch.uint8, device="cuda")
    calib_collect(x, state)
    before = state.cpu().numpy().copy()
    calib_collect(bad, state)
    after = state.cpu().numpy()
    a, b = unpack(torch.from_numpy(before)), unpack(torch.from_numpy(after))
    assert int(b["nonfinite"][0]) == 80 and int(b["batches"][0]) == int(a["batches"][0]) + 1 == 2
    same = np.ones(U.STATE_BYTES, dtype=bool)
    same[12:16] = same[24:32] = False       # batches, nonfinite
    assert np.array_equal(before[same], after[same])


def test_collect_doubling_sequence():
    """Batch maxima 1.0, 1.5 (one doubling), 9.0 (three), 1e6 (more than eleven: everything folds into bin 0), 0.3."""
    from bevformer_tensorrt_amd.functions import calib_collect, calib_state_size
    g = np.random.default_rng(11)
    arenas = [Arena(1 * MiB, p) for p in POISONS]
    states = [a.carve(calib_state_size(), 64, "state").zero_() for a in arenas]
    ref = U.RefState()
    ranges = []
    for top in (1.0, 1.5, 9.0, 1e6, 0.3):
        v = (g.uniform(-1.0, 1.0, 3001) * top).astype(np.float32)
        v[1234] = -top
        x, host = offset_by_one(v, torch.float32)
        ref.collect(host)
        for state in states:
            calib_collect(x, state)
            expect_equal(unpack(state), ref)
        ranges.append(float(ref.range))
    assert ranges == [1.0, 2.0, 16.0, 1048576.0, 1048576.0]
    assert ref.hist[0] >= 3 * 3001          # the first three batches sit in bin 0 after the fold
    for a in arenas:
        a.check()


def test_collect_graph_replay():
    """One collect captured after the site exists, replayed three times on the same data: exactly three times the
    single histogram.  One stream, no parallel branches."""
    from bevformer_tensorrt_amd.functions import calib_collect, calib_state_size
    g = np.random.default_rng(5)
    x, host = offset_by_one(np.maximum(g.standard_normal(50001), 0.0).astype(np.float32), torch.float16)
    ref = U.RefState().collect(host)
    state = torch.zeros(calib_state_size(), dtype=torch.uint8, device="cuda")
    calib_collect(x, state)                 # the site exists
    expect_equal(unpack(state), ref)
    state.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calib_collect(x, state)
    torch.cuda.synchronize()
    assert int(unpack(state)["count"][0]) == 0      # capture runs nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    got = unpack(state)
    assert [int(v) for v in got["hist"][0]] == [3 * v for v in ref.hist]
    assert int(got["count"][0]) == 3 * ref.count and int(got["batches"][0]) == 3
    assert got["range"][0] == ref.range and got["amax"][0] == ref.amax


# ---- bevops_calib_threshold
@pytest.fixture(scope="module")
def host_curves():
    """Per fixture: (RefState, host KL curve, host bin).  Computed once, never modified."""
    from bevformer_tensorrt_amd.quantization import entropy_kl_curve, entropy_threshold_bin
    out = []
    for st in U.entropy_fixtures():
        h = torch.tensor([float(v) for v in st.hist], dtype=torch.float64)
        out.append((st, entropy_kl_curve(h).numpy(), entropy_threshold_bin(h)))
    return out


def degenerate_states():
    g = np.random.default_rng(2)
    empty = U.RefState()
    zero = U.RefState().collect(np.zeros(1000, dtype=np.float32))
    top = U.RefState()
    top.range, top.amax, top.batches, top.count = np.float32(1), np.float32(1), 1, 5000
    top.hist[2047] = 5000
    low = U.RefState()
    low.range, low.amax, low.batches = np.float32(1), np.float32(0.05), 1
    low.hist[:100] = [int(v) for v in g.integers(1, 1000, 100)]
    low.count = sum(low.hist)
    return [("empty", empty), ("all in bin 0", zero), ("all in bin 2047", top), ("below bin 128", low)]


def run_threshold(lib, states, method, percentile=99.99, pad=128, want_kl=True):
    """The C entry on states uploaded into the guarded arena with a stride larger than the state, exact-size scratch;
    under both poisons.  Returns (bins, kl) as numpy."""
    from bevformer_tensorrt_amd.quantization import pack_calibration_states
    raw = pack_calibration_states(U.stack_fields(states))
    n, stride = len(states), U.STATE_BYTES + pad
    need = lib.bevops_calib_threshold_workspace_size(n)
    assert need == n * 1921 * 8
    seen = []
    for poison in POISONS:
        arena = Arena(n * stride + need + 4 * MiB, poison)
        buf = arena.carve(n * stride, 64, "states").view(n, stride)
        buf[:, :U.STATE_BYTES] = torch.from_numpy(raw).cuda()
        bins = arena.empty((n,), torch.int32, 4, "bins")
        kl = arena.empty((n,), torch.float64, 8, "kl")
        ws = arena.carve(need, 8, "scratch", scratch=True)
        before = buf.clone()
        st = lib.bevops_calib_threshold(method, ctypes.c_double(percentile), buf.data_ptr(), n, stride, bins.data_ptr(),
                                        kl.data_ptr() if want_kl else None, ws.data_ptr(), need, None)
        assert st == 0
        arena.check()
        assert torch.equal(buf, before), "the search wrote into the states"
        seen.append((bins.cpu().numpy().copy(), kl.cpu().numpy().copy()))
    assert np.array_equal(seen[0][0], seen[1][0])
    if want_kl:
        assert np.array_equal(seen[0][1], seen[1][1]), "KL minima differ between the two poisons"
    return seen[0]


def gap(curve):
    """Relative gap between the best and the runner-up of a KL curve (inf with fewer than two finite candidates)."""
    v = np.sort(curve[np.isfinite(curve)])
    return math.inf if v.size < 2 else (v[1] - v[0]) / max(abs(v[0]), 1e-300)


def test_threshold_entropy_fixtures(lib, host_curves):
    for i, (_, curve, _) in enumerate(host_curves):
        assert gap(curve) > 1e-9, f"fixture {i}: the host minimum is not separated (gap {gap(curve):.3g})"
    bins, kl = run_threshold(lib, [st for st, _, _ in host_curves], 0)
    for i, (_, curve, host_bin) in enumerate(host_curves):
        print(f"fixture {i}: host bin {host_bin} device bin {int(bins[i])} host KL {curve.min():.17g} device KL "
              f"{kl[i]:.17g} gap {gap(curve):.3g}")
    for i, (_, curve, host_bin) in enumerate(host_curves):
        assert int(bins[i]) == host_bin, f"fixture {i}: device bin {int(bins[i])}, host bin {host_bin}"
        assert abs(kl[i] - curve.min()) <= 1e-9 * abs(curve.min()), f"fixture {i}: KL {kl[i]} vs {curve.min()}"


def test_threshold_degenerate_states(lib):
    from bevformer_tensorrt_amd.quantization import entropy_threshold_bin
    named = degenerate_states()
    bins, kl = run_threshold(lib, [st for _, st in named], 0)
    want = {"empty": -1, "all in bin 0": 2047, "all in bin 2047": 2047, "below bin 128": 127}
    for i, (name, st) in enumerate(named):
        assert int(bins[i]) == want[name], f"{name}: {int(bins[i])}"
        if name != "empty":
            assert int(bins[i]) == entropy_threshold_bin(torch.tensor([float(v) for v in st.hist], dtype=torch.float64)), name
    assert math.isinf(kl[0]) and math.isinf(kl[1]) and kl[2] == 0.0 and kl[3] == 0.0
    # without the optional KL output
    bins2, _ = run_threshold(lib, [st for _, st in named], 0, want_kl=False)
    assert np.array_equal(bins, bins2)


@pytest.mark.parametrize("num_states", [1, 3, 65])
def test_threshold_state_counts(lib, host_curves, num_states):
    extra = [st for _, st in degenerate_states()]
    pool = [(st, b) for st, _, b in host_curves] + [(extra[0], -1), (extra[1], 2047)]
    pick = [pool[(3 * s + 1) % len(pool)] for s in range(num_states)]
    bins, _ = run_threshold(lib, [st for st, _ in pick], 0, pad=64 * (1 + num_states % 3))
    assert [int(b) for b in bins] == [b for _, b in pick]


@pytest.mark.parametrize("percentile", [50, 99.99, 100])
def test_threshold_percentile(lib, percentile):
    states = list(U.entropy_fixtures()) + [st for _, st in degenerate_states()]
    bins, _ = run_threshold(lib, states, 1, percentile)
    want = [U.host_percentile_bin(st.hist, percentile) if st.count else -1 for st in states]
    assert [int(b) for b in bins] == want


def test_threshold_workspace_and_methods(lib):
    from bevformer_tensorrt_amd.quantization import pack_calibration_states
    raw = torch.from_numpy(pack_calibration_states(U.stack_fields(U.entropy_fixtures()[:2]))).cuda()
    bins = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    need = lib.bevops_calib_threshold_workspace_size(2)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    args = (raw.data_ptr(), 2, U.STATE_BYTES, bins.data_ptr(), None, ws.data_ptr())
    assert lib.bevops_calib_threshold(0, ctypes.c_double(99.99), *args, need - 1, None) == 2
    assert lib.bevops_calib_threshold(1, ctypes.c_double(99.99), *args, need - 1, None) == 2
    assert lib.bevops_calib_threshold(2, ctypes.c_double(99.99), *args, need, None) == 3
    torch.cuda.synchronize()
    assert bins.tolist() == [-7, -7]        # a refused call launches nothing


# ---- calibrators
def test_device_minmax_matches_host_bit_for_bit():
    from bevformer_tensorrt_amd.quantization import DeviceMinMaxCalibrator, MinMaxCalibrator
    g = torch.Generator().manual_seed(0)
    dev_cal, host_cal = DeviceMinMaxCalibrator(), MinMaxCalibrator()
    for scale in (1.0, 3.7, 0.2):
        for name, dtype in (("a", torch.float16), ("b", torch.float32)):
            t = (torch.randn(3, 5, 41, generator=g) * scale).to(dtype).cuda()
            dev_cal.collect(name, t)
            host_cal.collect(name, t)
    dev_cal.collect("zeros", torch.zeros(9, device="cuda"))
    host_cal.collect("zeros", torch.zeros(9, device="cuda"))
    assert dev_cal.scales() == host_cal.scales()
    assert dev_cal.scale("zeros") == 1e-12 / 127.0


def test_device_entropy_scale_is_the_host_search_on_the_restated_histogram():
    from bevformer_tensorrt_amd.quantization import (DeviceEntropyCalibrator, DevicePercentileCalibrator,
                                                     entropy_kl_curve, entropy_threshold_bin)
    g = np.random.default_rng(21)
    batches = [g.standard_normal(1 << 17).astype(np.float32) * s for s in (1.0, 1.0, 2.5)]
    ref = U.RefState()
    cal, pct = DeviceEntropyCalibrator(), DevicePercentileCalibrator(99.9)
    for b in batches:
        ref.collect(b)
        t = torch.from_numpy(b).cuda()
        cal.collect("site", t)
        pct.collect("site", t)
    h = torch.tensor([float(v) for v in ref.hist], dtype=torch.float64)
    assert gap(entropy_kl_curve(h).numpy()) > 1e-9
    assert cal.scale("site") == (entropy_threshold_bin(h) + 0.5) * float(ref.range) / 2048 / 127.0
    assert pct.scale("site") == (U.host_percentile_bin(ref.hist, 99.9) + 0.5) * float(ref.range) / 2048 / 127.0
    assert cal.scales() == {"site": cal.scale("site")}


def test_device_calibrator_inputs():
    from bevformer_tensorrt_amd.quantization import DeviceEntropyCalibrator
    g = torch.Generator().manual_seed(4)
    x = torch.randn(6, 32, 14, 10, generator=g).half().cuda()
    cal = DeviceEntropyCalibrator()
    cal.CHUNK = 2                                   # five sites: three chunks
    cal.collect("slice", x[:, :18])
    cal.collect("copy", x[:, :18].contiguous())
    cal.collect("nhwc", x.contiguous(memory_format=torch.channels_last))
    cal.collect("nchw", x)
    cal.collect("empty", x[:0])
    assert not cal.has("empty") and cal.has("slice") and list(cal._stats) == ["slice", "copy", "nhwc", "nchw"]
    cal.collect("strided", x[..., ::3])
    raw = unpack(cal._states())
    assert len(cal._chunks) == 3 and raw["hist"].shape == (5, 2048)
    assert np.array_equal(raw["hist"][0], raw["hist"][1]) and np.array_equal(raw["hist"][2], raw["hist"][3])
    expect_equal({k: v[4:5] for k, v in raw.items()}, U.RefState().collect(x[..., ::3].cpu().numpy()))
    assert cal.scale("slice") == cal.scale("copy") and cal.scale("nhwc") == cal.scale("nchw")
    with pytest.raises(TypeError):
        cal.collect("host", torch.zeros(4))
    cal.collect("bad", torch.full((70,), float("nan"), device="cuda"))
    assert cal.has("bad")
    with pytest.raises(ValueError, match="NaN or infinite"):
        cal.scale("bad")
    # reserve() pre-sizes the arena: no further chunk for the sites it covers
    pre = DeviceEntropyCalibrator().reserve(10)
    for i in range(10):
        pre.collect(f"s{i}", x[i % 6])
    assert len(pre._chunks) == 1 and len(pre.scales()) == 10


def test_calibration_cache_round_trip_and_continued_collection(tmp_path):
    from bevformer_tensorrt_amd.quantization import DeviceEntropyCalibrator
    g = torch.Generator().manual_seed(8)
    batches = [(torch.randn(4, 3001, generator=g) * s).cuda() for s in (1.0, 2.0, 5.0)]
    names = ["msda#0.value", "linear:encoder.0.ffn", "chain:1.2.t1"]

    def feed(cal, batch):
        for j, name in enumerate(names):
            cal.collect(name, batch[j] if j else batch.half())

    whole, first = DeviceEntropyCalibrator(), DeviceEntropyCalibrator()
    for b in batches[:2]:
        feed(whole, b)
        feed(first, b)
    path = str(tmp_path / "calib.npz")
    first.save_calibration(path, {"site_bs": {"msda#0": 2}})
    loaded = DeviceEntropyCalibrator()
    assert loaded.load_calibration(path) == {"site_bs": {"msda#0": 2}}
    assert list(loaded._stats) == names
    assert torch.equal(loaded._states().cpu(), first._states().cpu())
    assert loaded.scales() == first.scales() == whole.scales()
    feed(whole, batches[2])
    feed(loaded, batches[2])
    assert torch.equal(loaded._states().cpu(), whole._states().cpu())
    assert loaded.scales() == whole.scales() and loaded.scales() != first.scales()


# ---- the INT8 engine, tiny configuration
def test_int8_engine_tiny_device_calibration_and_cache(tmp_path):
    """The frames of test_int8_engine_tiny_runs_and_tracks_fp16 (tests/test_int8_chain_gpu.py) and its bar."""
    from bevformer_tensorrt_amd import bevformer as B, geometry as G
    from bevformer_tensorrt_amd.quantization import ConvTapsQ, LinearQ, build_int8_engine
    dev, dtype = torch.device("cuda"), torch.float16
    H, W = B.CONFIGS["tiny"]["image"]
    l2i = G.synthetic_lidar2img((H, W)).to(dev)
    g = torch.Generator().manual_seed(1)

    def frame(i):
        can = torch.zeros(18)
        can[0], can[1], can[-1] = 0.4 * i, -0.1 * i, 1.0 * i
        return torch.randn(1, 6, 3, H, W, generator=g).to(dev, dtype), can, l2i

    cache = str(tmp_path / "tiny_calib.npz")
    model, qops, note = build_int8_engine(B, "tiny", dev, [frame(i) for i in range(3)], calibrator="entropy_device",
                                          calibration_cache=cache)
    assert os.path.exists(cache) and note["calibration_frames"] == 3
    assert note["activation_chain"] and note["int8_dense_layers"] > 0
    assert qops._scales and all(math.isfinite(s) and s > 0 for s in qops._scales.values())
    ref = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    rq, rf = B.FrameRunner(model, dev, dtype), B.FrameRunner(ref, dev, dtype)
    for i in range(2):
        f = frame(10 + i)
        cq, bq = rq.step(*f, "s")
        cf, bf = rf.step(*f, "s")
    assert torch.isfinite(cq.float()).all() and torch.isfinite(bq.float()).all()
    rel = ((rq.prev_bev.float() - rf.prev_bev.float()).abs().mean() / rf.prev_bev.float().std()).item()
    print(f"prev_bev mean |diff| / sigma = {rel:.4f}; {len(qops._scales)} sites")
    assert rel <= 0.1, rel
    rg = B.FrameRunner(model, dev, dtype, graph=True)
    f = frame(20)
    a = rg.step(*f, "g")
    b = rg.step(*f, "g")
    assert torch.isfinite(a[0].float()).all() and torch.isfinite(b[0].float()).all()

    # the second build reads the cache and runs no frame
    model2, qops2, note2 = build_int8_engine(B, "tiny", dev, [], calibrator="entropy_device", calibration_cache=cache)
    assert qops2._scales == qops._scales and qops2._site_bs == qops._site_bs
    assert note2 == note

    def module_scales(m):
        return {n: (q.scale_in, q.scale_w) for n, q in m.named_modules() if isinstance(q, (LinearQ, ConvTapsQ))}

    s1, s2 = module_scales(model), module_scales(model2)
    assert s1 and s1 == s2
    assert all(si is not None and sw is not None for si, sw in s1.values())
    with pytest.raises(ValueError, match="device calibrator"):
        build_int8_engine(B, "tiny", dev, [], calibrator="entropy", calibration_cache=cache)
