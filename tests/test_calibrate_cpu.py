"""CPU-only: the calibration entries of the C ABI answer bad arguments before they touch a device, the device
calibrators are registered, and the calibration cache's .npz schema round-trips on the host."""
import ctypes

import numpy as np
import pytest
import torch

import util_calibrate as U


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def test_state_size_and_workspace_query(lib):
    assert lib.bevops_calib_state_size() == 16448 == U.STATE_BYTES
    assert lib.bevops_calib_threshold_workspace_size(1) == 1921 * 8
    assert lib.bevops_calib_threshold_workspace_size(65) == 65 * 1921 * 8
    assert lib.bevops_calib_threshold_workspace_size(0) == 0 and lib.bevops_calib_threshold_workspace_size(-3) == 0
    from bevformer_tensorrt_amd import quantization as Q
    assert Q._STATE_BYTES == 16448


def test_collect_rejects_bad_arguments_without_gpu(lib):
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 63) & ~63          # a 64-byte aligned host address: never dereferenced
    size = ctypes.c_size_t
    assert lib.bevops_calib_collect(2, p, size(8), p, None) == 3           # int8
    assert lib.bevops_calib_collect(3, p, size(8), p, None) == 3           # uint8
    assert lib.bevops_calib_collect(7, None, size(0), None, None) == 3     # the dtype is judged first
    assert lib.bevops_calib_collect(0, None, size(0), None, None) == 0     # nothing to do
    assert lib.bevops_calib_collect(1, None, size(0), None, None) == 0
    assert lib.bevops_calib_collect(0, None, size(8), p, None) == 2        # no input
    assert lib.bevops_calib_collect(0, p, size(8), None, None) == 2        # no state
    assert lib.bevops_calib_collect(0, p + 2, size(8), p, None) == 2       # fp32 at a 2-byte address
    assert lib.bevops_calib_collect(1, p + 1, size(8), p, None) == 2       # fp16 at an odd address
    assert lib.bevops_calib_collect(1, p, size(8), p + 32, None) == 2      # state not 64-byte aligned
    assert lib.bevops_calib_collect(1, p + 2, size((1 << 40) + 1), p, None) == 3


def test_threshold_rejects_bad_arguments_without_gpu(lib):
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 63) & ~63
    size, dbl = ctypes.c_size_t, ctypes.c_double
    need = lib.bevops_calib_threshold_workspace_size(2)
    ok = dict(method=0, pct=99.99, states=p, n=2, stride=16448, bins=p, kl=None, ws=p, ws_bytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.bevops_calib_threshold(a["method"], dbl(a["pct"]), a["states"], a["n"], size(a["stride"]), a["bins"],
                                          a["kl"], a["ws"], size(a["ws_bytes"]), None)

    assert call(method=2) == 3 and call(method=-1) == 3
    assert call(ws_bytes=need - 1) == 2 and call(method=1, ws_bytes=need - 1) == 2
    assert call(ws=None) == 2 and call(ws=p + 4) == 2
    assert call(states=None) == 2 and call(bins=None) == 2
    assert call(n=0) == 2 and call(n=-1) == 2
    assert call(stride=16447) == 2 and call(stride=16448 + 8) == 2      # shorter than a state; not a multiple of 64
    assert call(states=p + 32) == 2 and call(bins=p + 2) == 2 and call(kl=p + 4) == 2
    assert call(method=1, pct=-1.0) == 2 and call(method=1, pct=float("nan")) == 2
    assert call(n=(1 << 20) + 1, ws_bytes=((1 << 20) + 1) * 1921 * 8) == 3


def test_device_calibrators_are_registered():
    from bevformer_tensorrt_amd import quantization as Q
    assert Q.get_calibrator("minmax_device") is Q.DeviceMinMaxCalibrator
    assert Q.get_calibrator("percentile_device") is Q.DevicePercentileCalibrator
    assert Q.get_calibrator("entropy_device") is Q.DeviceEntropyCalibrator
    # the host names keep their classes
    assert Q.get_calibrator("entropy") is Q.EntropyCalibrator and Q.get_calibrator("minmax") is Q.MinMaxCalibrator
    assert Q.get_calibrator("percentile") is Q.get_calibrator("legacy") is Q.PercentileCalibrator
    cal = Q.DevicePercentileCalibrator(99.9)
    assert cal.percentile == 99.9 and cal.scales() == {} and not cal.has("x")
    import bevformer_tensorrt_amd.functions as F
    for name in ("calib_state_size", "calib_collect", "calib_threshold"):
        assert name in F.__all__ and callable(getattr(F, name))
    assert F.calib_state_size() == 16448


def test_host_tensors_are_refused():
    from bevformer_tensorrt_amd import quantization as Q
    from bevformer_tensorrt_amd.functions import calib_collect, calib_threshold
    with pytest.raises(TypeError):
        calib_collect(torch.zeros(8), torch.zeros(16448, dtype=torch.uint8))
    with pytest.raises(TypeError):
        calib_threshold(torch.zeros(1, 16448, dtype=torch.uint8))
    with pytest.raises(TypeError):
        Q.DeviceEntropyCalibrator().collect("site", torch.zeros(8))
    with pytest.raises(ValueError, match="device calibrator"):
        Q.build_int8_engine(None, "tiny", torch.device("cpu"), [], calibrator="entropy", calibration_cache="calib.npz")
    with pytest.raises(ValueError, match="device calibrator"):
        Q.build_int8_engine(None, "tiny", torch.device("cpu"), [], calibrator=Q.MinMaxCalibrator(),
                            calibration_cache="calib.npz")


def test_state_bytes_pack_and_unpack():
    from bevformer_tensorrt_amd import quantization as Q
    g = np.random.default_rng(1)
    a = U.RefState().collect(g.standard_normal(5000).astype(np.float32)).collect(np.array([np.nan, 7.0], np.float32))
    b = U.RefState()
    b.hist[5], b.count, b.range = (1 << 40) + 3, (1 << 40) + 3, np.float32(0.5)      # counts beyond 32 bits
    fields = U.stack_fields([a, b])
    raw = Q.pack_calibration_states(fields)
    assert raw.shape == (2, 16448) and raw.dtype == np.uint8
    # the layout of include/bevops.h: range, amax, batch_amax, batches, count, nonfinite, 32 zero bytes, hist
    assert raw[0, 0:4].view(np.float32)[0] == a.range and raw[0, 4:8].view(np.float32)[0] == a.amax
    assert raw[0, 12:16].view(np.uint32)[0] == 2 and raw[0, 16:24].view(np.uint64)[0] == 5001
    assert raw[0, 24:32].view(np.uint64)[0] == 1 and not raw[:, 8:12].any() and not raw[:, 32:64].any()
    assert raw[1, 64 + 5 * 8:64 + 6 * 8].view(np.uint64)[0] == (1 << 40) + 3
    back = Q.unpack_calibration_states(raw)
    for k in fields:
        assert back[k].dtype == fields[k].dtype and np.array_equal(back[k], fields[k]), k
    assert U.describe(back, 0) == U.describe(a.fields()) and U.describe(back, 1) == U.describe(b.fields())


def test_calibration_cache_schema_round_trips(tmp_path):
    from bevformer_tensorrt_amd import quantization as Q
    g = np.random.default_rng(2)
    states = [U.RefState().collect((g.standard_normal(3000) * s).astype(np.float32)) for s in (1.0, 4.0, 0.1)]
    names = ["msda#0.value", "linear:encoder.layers.0.ffn.0", "chain:0.1.t1"]
    fields = U.stack_fields(states)
    extra = {"site_bs": {"msda#0": 2, "msda#1": 6}, "calibration_frames": 3}
    path = str(tmp_path / "cache.npz")
    Q.write_calibration_cache(path, names, fields, extra)
    with np.load(path, allow_pickle=False) as z:          # no pickle inside
        assert sorted(z.files) == sorted(["format", "names", "range", "amax", "count", "nonfinite", "batches", "hist",
                                          "extra"])
        assert z["hist"].dtype == np.uint64 and z["hist"].shape == (3, 2048)
        assert z["range"].dtype == np.float32 and z["count"].dtype == np.uint64 and z["batches"].dtype == np.uint32
        assert str(z["format"]) == "bevops-calibration-1"
    names2, fields2, extra2 = Q.read_calibration_cache(path)
    assert names2 == names and extra2 == extra
    for k in fields:
        assert np.array_equal(fields2[k], fields[k]) and fields2[k].dtype == fields[k].dtype, k
    assert np.array_equal(Q.pack_calibration_states(fields2), Q.pack_calibration_states(fields))
    # an empty calibrator's cache, and files that are not caches
    Q.write_calibration_cache(path, [], Q.unpack_calibration_states(np.zeros((0, 16448), np.uint8)))
    assert Q.read_calibration_cache(path)[0] == [] and Q.read_calibration_cache(path)[2] == {}
    other = str(tmp_path / "other.npz")
    with open(other, "wb") as f:
        np.savez(f, names=np.array(names))
    with pytest.raises(ValueError, match="not a calibration cache"):
        Q.read_calibration_cache(other)


def test_kl_curve_is_what_the_threshold_search_minimises():
    """entropy_kl_curve was split out of entropy_threshold_bin for the device tests: same first minimum, and the
    host reference agrees with the integer form of the level index the kernel uses."""
    from bevformer_tensorrt_amd import quantization as Q
    st = U.RefState().collect(np.random.default_rng(6).standard_normal(20000).astype(np.float32))
    h = torch.tensor([float(v) for v in st.hist], dtype=torch.float64)
    curve = Q.entropy_kl_curve(h)
    assert curve.shape == (1921,) and Q.entropy_threshold_bin(h) == 128 + int(torch.argmin(curve)) - 1
    assert Q.entropy_threshold_bin(torch.zeros(2048, dtype=torch.float64)) == 2047
    for i in range(128, 2049):
        k = np.arange(i)
        integer = ((2 * k + 1) * 64 + i - 1) // i - 1
        assert np.array_equal(integer, np.ceil((k + 0.5) * 128 / i).astype(np.int64) - 1)
        assert integer.min() == 0 and integer.max() == 127
