"""Host restatement of the device calibration state (include/bevops.h, "PTQ calibration on the device") for
tests/test_calibrate_gpu.py and tests/test_calibrate_cpu.py: numpy for the binning, Python integers for the merge."""
import functools

import numpy as np

BINS = 2048
STATE_BYTES = 64 + 8 * BINS


def reference_bins(x32, rng):
    """bin of every element of the float32 array x32 (finite values) for the float32 range `rng`."""
    x32 = np.asarray(x32, dtype=np.float32)
    inv = np.float32(2048) / np.float32(rng)
    return np.minimum((np.abs(x32) * inv).astype(np.int32), 2047)


class RefState:
    """One calibration site on the host.  collect(x) follows bevops_calib_collect step by step."""

    def __init__(self):
        self.range = np.float32(0)
        self.amax = np.float32(0)
        self.batches = 0
        self.count = 0
        self.nonfinite = 0
        self.hist = [0] * BINS          # Python integers

    def collect(self, x):
        x32 = np.asarray(x).astype(np.float32).ravel()        # fp16 -> fp32 is exact
        if x32.size == 0:
            return self
        finite = np.isfinite(x32)
        self.nonfinite += int((~finite).sum())
        self.batches += 1
        v = np.abs(x32[finite])
        if v.size == 0:
            return self
        batch_amax = np.float32(v.max())
        if self.range == 0:
            self.range = np.maximum(batch_amax, np.float32(1e-12))
        d = 0
        while batch_amax > self.range:
            self.range = np.float32(self.range * np.float32(2))
            d += 1
        if d:
            d = min(d, 11)
            live = BINS >> d
            self.hist = [sum(self.hist[j << d:(j + 1) << d]) if j < live else 0 for j in range(BINS)]
        self.amax = np.maximum(self.amax, batch_amax)
        for b, c in zip(*np.unique(reference_bins(v, self.range), return_counts=True)):
            self.hist[int(b)] += int(c)
        self.count += int(v.size)
        return self

    def fields(self):
        return {"range": np.array([self.range], np.float32), "amax": np.array([self.amax], np.float32),
                "batches": np.array([self.batches], np.uint32), "count": np.array([self.count], np.uint64),
                "nonfinite": np.array([self.nonfinite], np.uint64), "hist": np.array([self.hist], np.uint64)}


def stack_fields(states):
    """fields of several RefStates as the [S] / [S, 2048] arrays quantization.pack_calibration_states takes."""
    parts = [s.fields() for s in states]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def describe(fields, i=0):
    """The comparable content of state i: (range bits, amax bits, batches, count, nonfinite, hist list)."""
    return (int(np.asarray(fields["range"], np.float32).view(np.uint32)[i]),
            int(np.asarray(fields["amax"], np.float32).view(np.uint32)[i]), int(fields["batches"][i]),
            int(fields["count"][i]), int(fields["nonfinite"][i]), [int(v) for v in fields["hist"][i]])


@functools.lru_cache(maxsize=None)
def entropy_fixtures():
    """The eight sample sets of the threshold tests, drawn in this order from ONE numpy.random.default_rng(0) and each
    binned at range = max |x|: a tuple of RefStates.  With numpy 2.x streams quantization.entropy_threshold_bin answers
    1938, 1935, 1625, 127, 2047, 1501, 316, 734 on them and the smallest relative gap between the best and the
    runner-up KL is 4.5e-4; the tests recompute both and do not rely on these figures."""
    g = np.random.default_rng(0)
    n = 1 << 20
    samples = [
        g.standard_normal(n),
        np.maximum(g.standard_normal(n), 0.0),
        g.laplace(size=n),
        np.concatenate([g.standard_normal(n - 64), g.standard_normal(64) * 40.0]),
        g.uniform(-1.0, 1.0, 1 << 18),
        g.standard_normal(4096),
        g.lognormal(0.0, 1.0, 1 << 19),
        np.concatenate([0.01 * g.standard_normal(1 << 19), g.standard_normal(1 << 15)]),
    ]
    return tuple(RefState().collect(s.astype(np.float32)) for s in samples)


def host_percentile_bin(hist, percentile):
    """PercentileCalibrator.scale's bin for a histogram given as integers."""
    import torch
    cdf = torch.cumsum(torch.tensor([float(v) for v in hist], dtype=torch.float64), 0)
    return min(int(torch.searchsorted(cdf, cdf[-1] * percentile / 100.0)), BINS - 1)
