"""Per-tensor PTQ calibrators producing the scales the INT8 operators take.

In the reference the scales come from TensorRT: `get_calibrator("minmax" | "entropy" | "legacy")`
wraps `trt.IInt8MinMaxCalibrator` / `IInt8EntropyCalibrator2` / `IInt8LegacyCalibrator`
(det2trt/quantization/calibrator_trt.py:6-92) and the engine hands each plugin its tensors'
`PluginTensorDesc::scale` (multiScaleDeformableAttnPlugin.cpp:75-77); the QDQ flow uses
pytorch_quantization's max / 99.99-percentile histogram calibrators
(det2trt/quantization/calibrator_qdq.py:29-80).  Neither library exists on ROCm, so the
published algorithms are restated here as host logic (torch tensors, histograms on the
device the data lives on); the `*_device` calibrators further down keep the same statistics on the
device (csrc/calibrate.hip) and add the calibration cache the reference's calibrator leaves empty:

  * MinMaxCalibrator      scale = max|x| / 127 over all calibration batches
  * PercentileCalibrator  scale = percentile(|x|, p) / 127 from a running histogram (p = 99.99)
  * EntropyCalibrator     TensorRT "entropy calibration 2" (8-bit Inference with TensorRT,
                          S. Migacz, GTC 2017): 2048-bin histogram of |x|; for every candidate
                          clip bin i in [128, 2048): reference P = hist[:i] with the outliers
                          folded into the last bin, candidate Q = P merged into 128 levels and
                          expanded back over P's non-empty bins; threshold = argmin KL(P || Q).  The
                          zero bin is given its neighbour's count first (the spike of exact zeros behind
                          a ReLU carries no information about the clip point).

`get_calibrator(name)` mirrors the reference's factory; `Calibrator.collect(name, tensor)` is
called per boundary tensor per calibration frame; `scales()` returns {name: scale}.
"""
import math

import os

import torch

from .functions.multi_scale_deformable_attn import _TensorCache

_NUM_BINS = 2048
_NUM_LEVELS = 128


class _Base:
    def __init__(self):
        self._stats = {}

    def collect(self, name, tensor):
        raise NotImplementedError

    def scale(self, name):
        raise NotImplementedError

    def scales(self):
        return {k: self.scale(k) for k in self._stats}

    def has(self, name):
        """False for a site that never saw data (a layer fed empty tensors only: a rank of the camera-sharded
        path without cameras runs its per-camera layers on empty batches)."""
        return name in self._stats

    @staticmethod
    def quantize(tensor, scale):
        """real -> int8 with round-to-nearest-even and saturation to [-127, 127]."""
        return torch.clamp(torch.round(tensor.float() / scale), -127, 127).to(torch.int8)


class MinMaxCalibrator(_Base):
    def collect(self, name, tensor):
        if tensor.numel() == 0:
            return
        m = float(tensor.detach().abs().max())
        self._stats[name] = max(self._stats.get(name, 0.0), m)

    def scale(self, name):
        return max(self._stats[name], 1e-12) / 127.0


class _Histogram(_Base):
    """Running histogram of |x| with a range that doubles when a batch exceeds it (bins merge
    pairwise, so earlier batches stay exactly accounted for)."""

    def collect(self, name, tensor):
        if tensor.numel() == 0:
            return
        x = tensor.detach().abs().float().flatten()
        amax = float(x.max())
        st = self._stats.get(name)
        if st is None:
            st = {"hist": torch.zeros(_NUM_BINS, dtype=torch.float64), "range": max(amax, 1e-12)}
            self._stats[name] = st
        while amax > st["range"]:
            st["hist"] = torch.cat([st["hist"].view(-1, 2).sum(1), torch.zeros(_NUM_BINS // 2, dtype=torch.float64)])
            st["range"] *= 2
        h = torch.histc(x, bins=_NUM_BINS, min=0.0, max=st["range"])
        st["hist"] += h.double().cpu()


class PercentileCalibrator(_Histogram):
    def __init__(self, percentile=99.99):
        super().__init__()
        self.percentile = percentile

    def scale(self, name):
        st = self._stats[name]
        cdf = torch.cumsum(st["hist"], 0)
        idx = int(torch.searchsorted(cdf, cdf[-1] * self.percentile / 100.0))
        return (min(idx, _NUM_BINS - 1) + 0.5) * st["range"] / _NUM_BINS / 127.0


class EntropyCalibrator(_Histogram):
    def scale(self, name):
        st = self._stats[name]
        i = entropy_threshold_bin(st["hist"])
        return (i + 0.5) * st["range"] / _NUM_BINS / 127.0


def entropy_threshold_bin(hist, num_levels=_NUM_LEVELS):
    """Clip bin minimising KL(P || Q) as described in the module docstring.  All candidate clip
    bins are evaluated at once (a [candidates, bins] batch) instead of one Python iteration each."""
    kl = entropy_kl_curve(hist, num_levels)
    best = int(torch.argmin(kl))                                 # first minimum, like the loop
    return num_levels + best - 1 if math.isfinite(float(kl[best])) else hist.numel() - 1


def entropy_kl_curve(hist, num_levels=_NUM_LEVELS):
    """KL(P || Q) for every candidate i = num_levels .. bins kept bins (float64 [bins - num_levels + 1], +inf where
    P or Q is empty): the curve entropy_threshold_bin takes the first minimum of."""
    hist = hist.double().cpu().clone()
    # the bin at zero takes the count of its neighbour (pytorch_quantization's histogram calibrator does the same,
    # `bins[0] = bins[1]` in _compute_amax_entropy): the exact zeros a ReLU emits -- half of the tensor or more --
    # are represented exactly at ANY threshold, yet as one spike they dominate KL(P || Q) and drag the threshold
    # towards it (a ReLU of a unit Gaussian: T = 1.8 sigma, 17 % rms error; with a shifted ReLU 66 %)
    hist[0] = hist[1]
    n = hist.numel()
    cand = torch.arange(num_levels, n + 1)                       # i = number of bins kept
    k = torch.arange(n)
    keep = k[None, :] < cand[:, None]                            # [I, n]
    csum = torch.cumsum(hist, 0)
    tail = csum[-1] - csum[cand - 1]                             # mass beyond the clip bin
    src = hist[None, :] * keep                                   # hist[:i]
    p = src.clone()
    p[torch.arange(cand.numel()), cand - 1] += tail              # outliers folded into the last bin
    # merge the i kept bins into num_levels levels, expand back over the non-empty bins
    idx = torch.ceil((k[None, :].double() + 0.5) * num_levels / cand[:, None].double()).long() - 1
    idx = idx.clamp_(0, num_levels - 1)
    nonzero = (src > 0).double()
    level_sum = torch.zeros(cand.numel(), num_levels, dtype=torch.float64).scatter_add_(1, idx, src)
    level_cnt = torch.zeros(cand.numel(), num_levels, dtype=torch.float64).scatter_add_(1, idx, nonzero)
    q = torch.gather(level_sum / level_cnt.clamp(min=1), 1, idx) * nonzero
    psum, qsum = p.sum(1, keepdim=True), q.sum(1, keepdim=True)
    ok = (psum > 0) & (qsum > 0)
    pn = p / psum.clamp(min=1e-300)
    qn = (q / qsum.clamp(min=1e-300)).clamp(min=1e-12)           # P > 0 with Q == 0: the folded bin only
    term = torch.where(pn > 0, pn * torch.log(pn.clamp(min=1e-300) / qn), torch.zeros_like(pn))
    kl = term.sum(1)
    kl[~ok[:, 0]] = math.inf
    return kl

_CACHE_FORMAT = "bevops-calibration-1"
_STATE_BYTES = 64 + 8 * _NUM_BINS          # bevops_calib_state_size(): tests hold the two equal
_CACHE_KEYS = ("format", "names", "range", "amax", "count", "nonfinite", "batches", "hist", "extra")


def unpack_calibration_states(raw):
    """uint8 [S, 16448] state bytes (include/bevops.h, "PTQ calibration on the device") -> dict of numpy fields."""
    import numpy as np
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1, _STATE_BYTES)
    head = raw[:, :64]
    f32 = np.ascontiguousarray(head[:, :12]).view(np.float32)
    return {"range": f32[:, 0].copy(), "amax": f32[:, 1].copy(),
            "batches": np.ascontiguousarray(head[:, 12:16]).view(np.uint32)[:, 0].copy(),
            "count": np.ascontiguousarray(head[:, 16:24]).view(np.uint64)[:, 0].copy(),
            "nonfinite": np.ascontiguousarray(head[:, 24:32]).view(np.uint64)[:, 0].copy(),
            "hist": np.ascontiguousarray(raw[:, 64:]).view(np.uint64).reshape(-1, _NUM_BINS).copy()}


def pack_calibration_states(fields):
    """The inverse of unpack_calibration_states: uint8 [S, 16448] (the scratch fields of the header are zero)."""
    import numpy as np
    n = len(fields["range"])
    raw = np.zeros((n, _STATE_BYTES), dtype=np.uint8)
    raw[:, 0:4] = np.asarray(fields["range"], dtype=np.float32).reshape(n, 1).view(np.uint8)
    raw[:, 4:8] = np.asarray(fields["amax"], dtype=np.float32).reshape(n, 1).view(np.uint8)
    raw[:, 12:16] = np.asarray(fields["batches"], dtype=np.uint32).reshape(n, 1).view(np.uint8)
    raw[:, 16:24] = np.asarray(fields["count"], dtype=np.uint64).reshape(n, 1).view(np.uint8)
    raw[:, 24:32] = np.asarray(fields["nonfinite"], dtype=np.uint64).reshape(n, 1).view(np.uint8)
    raw[:, 64:] = np.ascontiguousarray(fields["hist"], dtype=np.uint64).reshape(n, _NUM_BINS).view(np.uint8)
    return raw


def write_calibration_cache(path, names, fields, extra=None):
    """One .npz (no pickle): format, names, range, amax, count, nonfinite, batches, hist [S, 2048] uint64, and `extra`
    as a JSON string.  What the reference's calibrator leaves as `pass`
    (det2trt/quantization/calibrator_trt.py:86-90)."""
    import json

    import numpy as np
    names = list(names)
    assert len(names) == len(fields["range"]) and len(set(names)) == len(names)
    with open(path, "wb") as f:
        np.savez(f, format=np.array(_CACHE_FORMAT), names=np.array(names, dtype=np.str_),
                 range=np.asarray(fields["range"], dtype=np.float32), amax=np.asarray(fields["amax"], dtype=np.float32),
                 count=np.asarray(fields["count"], dtype=np.uint64),
                 nonfinite=np.asarray(fields["nonfinite"], dtype=np.uint64),
                 batches=np.asarray(fields["batches"], dtype=np.uint32),
                 hist=np.asarray(fields["hist"], dtype=np.uint64).reshape(len(names), _NUM_BINS),
                 extra=np.array(json.dumps(extra if extra is not None else {}, sort_keys=True)))


def read_calibration_cache(path):
    """-> (names, fields, extra) as write_calibration_cache took them."""
    import json

    import numpy as np
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _CACHE_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not a calibration cache (missing {missing})")
        if str(z["format"]) != _CACHE_FORMAT:
            raise ValueError(f"{path}: calibration cache format {str(z['format'])!r}, expected {_CACHE_FORMAT!r}")
        names = [str(n) for n in z["names"]]
        fields = {k: z[k] for k in ("range", "amax", "count", "nonfinite", "batches", "hist")}
        extra = json.loads(str(z["extra"]))
    if fields["hist"].shape != (len(names), _NUM_BINS) or any(fields[k].shape != (len(names),) for k in
                                                              ("range", "amax", "count", "nonfinite", "batches")):
        raise ValueError(f"{path}: calibration cache arrays do not match its {len(names)} names")
    return names, fields, extra


class _DeviceCalibrator(_Base):
    """Calibration state on the device (functions/calibrate.py, csrc/calibrate.hip): every site owns one 16 448-byte
    slot of a zero-filled arena; `collect` is three launches and no host synchronisation, so it can sit inside a
    captured frame; `scale` / `scales` run one threshold search over all sites and copy the headers and the bins to
    the host once, cached until the next `collect`.  `_stats` maps a site to its slot index."""

    CHUNK = 64            # slots per arena chunk; chunks are never moved (a captured graph may hold their addresses)
    method = None         # calib_threshold's method; None: no search (min-max)
    percentile = 99.99

    def __init__(self):
        super().__init__()
        self._chunks = []
        self._used = 0
        self._device = None
        self._cache = None

    # ---- arena
    @staticmethod
    def _cuda_device(device):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise TypeError(f"device calibrators keep their state on a CUDA device, not on {device}")
        return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())

    def reserve(self, n, device=None):
        """Make room for `n` sites in all (one chunk holding the missing slots)."""
        from .functions import calibrate as _c
        if self._device is None:
            self._device = self._cuda_device(device)
        have = sum(c.shape[0] for c in self._chunks)
        if n > have:
            size = _c.calib_state_size()
            assert size == _STATE_BYTES
            self._chunks.append(torch.zeros(n - have, size, dtype=torch.uint8, device=self._device))
        return self

    def _slot(self, index):
        for c in self._chunks:
            if index < c.shape[0]:
                return c[index]
            index -= c.shape[0]
        raise IndexError(index)

    def _states(self):
        """uint8 [sites, 16448]: the used slots in slot order (a device copy when they span chunks)."""
        parts, left = [], self._used
        for c in self._chunks:
            if left <= 0:
                break
            parts.append(c[:min(left, c.shape[0])])
            left -= c.shape[0]
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    # ---- the calibrator interface
    def collect(self, name, tensor):
        from .functions import calibrate as _c
        if not isinstance(tensor, torch.Tensor) or not tensor.is_cuda:
            raise TypeError(f"{type(self).__name__}.collect: expected a CUDA tensor")
        if tensor.numel() == 0:
            return
        if self._device is not None and tensor.device != self._device:
            raise ValueError(f"{type(self).__name__}: state lives on {self._device}, tensor on {tensor.device}")
        index = self._stats.get(name)
        if index is None:
            have = sum(c.shape[0] for c in self._chunks)
            if self._used >= have:
                self.reserve(have + self.CHUNK, tensor.device)
            index = self._stats[name] = self._used
            self._used += 1
        _c.calib_collect(tensor, self._slot(index))
        self._cache = None

    def _results(self):
        """{name: (range, amax, count, bin)} as Python numbers: one search, one device-to-host copy."""
        if self._cache is None:
            import numpy as np
            from .functions import calibrate as _c
            names = list(self._stats)
            out = {}
            if names:
                states = self._states()
                n = states.shape[0]
                packed = torch.zeros(n, 72, dtype=torch.uint8, device=states.device)
                packed[:, :64] = states[:, :64]
                if self.method is not None:
                    bins, _ = _c.calib_threshold(states, self.method, self.percentile)
                    packed[:, 64:68] = bins.view(torch.uint8).view(n, 4)
                host = packed.cpu().numpy()
                f32 = np.ascontiguousarray(host[:, :8]).view(np.float32)
                count = np.ascontiguousarray(host[:, 16:24]).view(np.uint64)[:, 0]
                bins = np.ascontiguousarray(host[:, 64:68]).view(np.int32)[:, 0]
                for i, name in enumerate(names):
                    out[name] = (float(f32[i, 0]), float(f32[i, 1]), int(count[i]), int(bins[i]))
            self._cache = out
        return self._cache

    def _entry(self, name):
        rng, amax, count, b = self._results()[name]
        if count == 0:
            raise ValueError(f"calibration site '{name}': every element it saw was NaN or infinite")
        return rng, amax, b

    def scales(self):
        return {k: self.scale(k) for k in self._stats}

    # ---- calibration cache
    def save_calibration(self, path, extra=None):
        """Write every site's state to `path` (write_calibration_cache); `extra`: a JSON-serialisable dict."""
        raw = self._states().cpu().numpy() if self._stats else torch.zeros(0, _STATE_BYTES, dtype=torch.uint8).numpy()
        write_calibration_cache(path, list(self._stats), unpack_calibration_states(raw), extra)

    def load_calibration(self, path, device=None):
        """Replace this calibrator's state with the cache at `path`; collection can go on afterwards.  Returns `extra`."""
        names, fields, extra = read_calibration_cache(path)
        self._stats, self._chunks, self._used, self._cache = {}, [], 0, None
        if device is not None:
            self._device = self._cuda_device(device)
        if names:
            self.reserve(len(names))
            self._chunks[0].copy_(torch.from_numpy(pack_calibration_states(fields)))
            self._stats = {n: i for i, n in enumerate(names)}
            self._used = len(names)
        return extra


class DeviceMinMaxCalibrator(_DeviceCalibrator):
    """MinMaxCalibrator on the device state: scale = running max|x| / 127, the host class's expression."""

    def scale(self, name):
        return max(self._entry(name)[1], 1e-12) / 127.0


class DevicePercentileCalibrator(_DeviceCalibrator):
    """PercentileCalibrator's rule on the device histogram."""
    method = "percentile"

    def __init__(self, percentile=99.99):
        super().__init__()
        self.percentile = percentile

    def scale(self, name):
        rng, _, b = self._entry(name)
        return (b + 0.5) * rng / _NUM_BINS / 127.0


class DeviceEntropyCalibrator(_DeviceCalibrator):
    """EntropyCalibrator's search (entropy_threshold_bin) on the device histogram, all sites in one call."""
    method = "entropy"

    def scale(self, name):
        rng, _, b = self._entry(name)
        return (b + 0.5) * rng / _NUM_BINS / 127.0


CALIBRATORS = {"minmax": MinMaxCalibrator, "entropy": EntropyCalibrator, "percentile": PercentileCalibrator,
               "legacy": PercentileCalibrator, "minmax_device": DeviceMinMaxCalibrator,
               "percentile_device": DevicePercentileCalibrator, "entropy_device": DeviceEntropyCalibrator}


def get_calibrator(calibrator):
    """Factory with the reference's names (det2trt/quantization/calibrator_trt.py:6-16)."""
    assert calibrator in CALIBRATORS, f"calibrator should be in {sorted(CALIBRATORS)}"
    return CALIBRATORS[calibrator]


class Int8PluginOps:
    """INT8 scale plumbing for the plugin call sites of a model.

    An operator namespace that can be handed to `BEVFormer(ops=...)` in place of
    `bevformer_tensorrt_amd.functions`.  Two phases, like a TensorRT PTQ build
    (tools/bevformer/onnx2trt.py:110-241 feeds calibration batches through the network, TensorRT
    records one scale per plugin tensor, the engine then hands `PluginTensorDesc::scale` to
    `enqueue`):

      calibrate : every plugin call runs the fp operator while the calibrator collects its boundary
                  tensors under a stable name  "<op>#<call index within the frame>.<tensor>";
      int8      : the same call sites quantise their inputs with the recorded scales, run the
                  INT8 flavour of the operator (`*_int8`) and de-quantise the result.

    Only the sampling operators are quantised (the scope of the custom plugins); dense layers stay
    in the model's dtype.  `begin_frame()` resets the per-frame call counters (the model's
    forward pre-hook installed by `attach`).  The fused / channels-last entries are deliberately not
    exposed, so a model built on this namespace takes the reference op sequence.
    """

    # fp entries a `channels_last=True` namespace passes through: the channels-last backbone (its DCNv2
    # block, offset convolution and epilogues stay in the model's dtype there -- the INT8 DCNv2 operator
    # exists for the plugin layout only), the fused dense / norm entries for layers that were not swapped
    # for LinearQ, and -- `fused_sca=True` -- the fused fp16 SCA sampler.  Like a TensorRT INT8 engine the
    # build is then mixed: INT8 where an INT8 implementation exists and pays, fp16 elsewhere.
    _PASS = ("bias_act_nhwc_", "conv_offset_nhwc", "modulated_deformable_conv2d_nhwc", "layer_norm",
             "linear_bias_act", "dense_auto", "tsgemm_ln", "self_attention_qkv", "refine_reference_points", "decode_boxes", "conv3x3_auto", "conv_nhwc", "conv_int8_nhwc", "bias_relu_maxpool_nhwc", "stem_conv_pool",
             "image_normalize_pad", "image_normalize_resize_pad", "upsample_add_nhwc_", "feat_embed_nhwc", "tsa_split", "queue_mean2")
    # `engine=True` (the build bench.py times, build_int8_engine below) additionally passes the entries whose fp16
    # form is FASTER than any int8 form on MI355X: the channels-last nearest-neighbour rotate of prev_bev (pure data
    # movement: rotating commutes with quantising, the int8 plugin would only add a quantise and a de-quantise pass
    # around it) and the value projection that writes the SCA sampler's planes itself.
    # ... and the camera projection of the BEV pillars (index generation: fp32 and bit-exact in every build).
    _ENGINE_PASS = ("rotate_hwc", "spatial_cross_attention_projected", "spatial_cross_attention_plan", "point_sampling")

    def __init__(self, calibrator="entropy", fp_ops=None, channels_last=False, fused_sca=False, engine=False):
        from . import functions as _f
        self.fp = fp_ops if fp_ops is not None else _f
        self.cal = get_calibrator(calibrator)() if isinstance(calibrator, str) else calibrator
        self.mode = "calibrate"
        self._scales = {}
        self._n = {}
        self._wq = _TensorCache()      # float weight tensor -> (int8 weight, scale)
        self._pass = self._PASS + (("spatial_cross_attention_sample",) if fused_sca else ()) if channels_last else ()
        if engine:
            self._pass = self._pass + self._ENGINE_PASS
        self._site_bs = {}             # msda site -> batch dimension of its call (2: TSA, cameras: SCA, 1: decoder)
        # optional predicate site -> bool: in the int8 phase a site it rejects keeps its fp operator (a layer-precision
        # fallback, as a TensorRT build allows per layer; tools/int8_attribution.py switches groups of sites with it)
        self.site_filter = None
        self.int8_ln_fused = None      # bevformer._INT8_LN_FUSED for the model on this namespace (None: the switch's value)

    def __getattr__(self, name):       # only reached for names this class does not define
        if name in self.__dict__.get("_pass", ()) and hasattr(self.fp, name):
            return getattr(self.fp, name)
        raise AttributeError(name)

    # ---- bookkeeping
    def begin_frame(self):
        self._n = {}

    def attach(self, model):
        model.register_forward_pre_hook(lambda m, args: self.begin_frame())
        return self

    def freeze(self):
        """End of calibration: fix the scales and switch the call sites to their INT8 flavours."""
        self._scales = self.cal.scales()
        self._wq = _TensorCache()
        self.mode = "int8"
        return self._scales

    def _site(self, op):
        i = self._n.get(op, 0)
        self._n[op] = i + 1
        return f"{op}#{i}"

    def site_batch(self, site):
        """Batch dimension the MSDA site was calibrated with (None: not an MSDA site / never seen)."""
        return self._site_bs.get(site)

    def _fp_site(self, site):
        return self.mode == "int8" and self.site_filter is not None and not self.site_filter(site)

    def _q(self, name, t):
        s = self._scales[name]
        if t.is_cuda and t.dtype == torch.float16 and t.numel() % 8 == 0 and hasattr(self.fp, "quantize_rows"):
            # one pass (bevops_quantize_rows: clamp(rne(x / s)) with the division in fp32, the calibrators' host
            # formula) instead of the five framework launches and the fp32 copy of `_Base.quantize`
            return self.fp.quantize_rows(t.contiguous(), s), s
        return self.cal.quantize(t, s), s

    def _dq(self, q, s, dtype):
        """int8 result of a plugin -> the model's dtype: q * s, one pass when the operator set has the entry."""
        if q.is_cuda and dtype == torch.float16 and q.numel() % 8 == 0 and hasattr(self.fp, "dequantize_rows"):
            return self.fp.dequantize_rows(q, s)
        return q.to(dtype) * s

    # ---- call sites
    def multi_scale_deformable_attn(self, value, shapes, ref, off, w):
        site = self._site("msda")
        if self.mode == "calibrate":
            self._site_bs[site] = int(value.shape[0])
            out = self.fp.multi_scale_deformable_attn(value, shapes, ref, off, w)
            for k, t in (("value", value), ("offsets", off), ("weights", w), ("out", out)):
                self.cal.collect(f"{site}.{k}", t)
            return out
        if self._fp_site(site):
            return self.fp.multi_scale_deformable_attn(value, shapes, ref, off, w)
        (qv, sv), (qo, so), (qw, sw) = (self._q(f"{site}.{k}", t) for k, t in
                                        (("value", value), ("offsets", off), ("weights", w)))
        s_out = self._scales[f"{site}.out"]
        # reference points stay fp16: the <__half2> flavour (multiScaleDeformableAttnPlugin.cpp:118-125)
        out = self.fp.multi_scale_deformable_attn_int8(qv, shapes, ref.to(torch.float16).contiguous(),
                                                       qo.contiguous(), qw.contiguous(), sv, so, sw, s_out)
        return self._dq(out, s_out, value.dtype)

    multi_scale_deformable_attn2 = multi_scale_deformable_attn

    def rotate(self, img, angle, center, interpolation="nearest"):
        site = self._site("rotate")
        if self.mode == "calibrate":
            out = self.fp.rotate(img, angle, center, interpolation)
            self.cal.collect(f"{site}.img", img)
            return out
        if self._fp_site(site):
            return self.fp.rotate(img, angle, center, interpolation)
        q, s = self._q(f"{site}.img", img)
        out = self.fp.rotate_int8(q.contiguous(), angle, center, s, s, interpolation)
        return self._dq(out, s, img.dtype)

    rotate2 = rotate

    def modulated_deformable_conv2d(self, x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1,
                                    groups=1, deform_groups=1):
        site = self._site("dcn")
        if self.mode == "calibrate":
            out = self.fp.modulated_deformable_conv2d(x, offset, mask, weight, bias, stride, padding, dilation,
                                                      groups, deform_groups)
            for k, t in (("x", x), ("offset", offset), ("mask", mask), ("weight", weight), ("out", out)):
                self.cal.collect(f"{site}.{k}", t)
            return out
        if self._fp_site(site):
            return self.fp.modulated_deformable_conv2d(x, offset, mask, weight, bias, stride, padding, dilation,
                                                       groups, deform_groups)
        (qx, sx), (qo, so), (qm, sm) = (self._q(f"{site}.{k}", t) for k, t in
                                        (("x", x), ("offset", offset), ("mask", mask)))
        hit = self._wq.get(weight)           # the weights of a deployed model are quantised (and packed) once
        if hit is None:
            hit = self._wq.put(weight, self._q(f"{site}.weight", weight))
        qw, sw = hit
        s_out = self._scales[f"{site}.out"]
        out = self.fp.modulated_deformable_conv2d_int8(qx, qo, qm, qw, None if bias is None else bias.float(),
                                                       sx, so, sm, sw, s_out, stride, padding, dilation, groups,
                                                       deform_groups)
        return self._dq(out, s_out, x.dtype)

    modulated_deformable_conv2d2 = modulated_deformable_conv2d

    def bev_pool_v2(self, depth, feat, ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths,
                    out_height=128, out_width=128):
        """BEVPoolV2TRT[2] (bevPoolKernel.cu:115-149 in its INT8 flavour): depth and features int8, int32 sums,
        one requantisation with the output's calibrated scale."""
        site = self._site("bev_pool")
        args = (ranks_depth, ranks_feat, ranks_bev, interval_starts, interval_lengths)
        if self.mode == "calibrate" or self._fp_site(site):
            out = self.fp.bev_pool_v2_2(depth, feat, *args, out_height, out_width)
            if self.mode == "calibrate":
                for k, t in (("depth", depth), ("feat", feat), ("out", out)):
                    self.cal.collect(f"{site}.{k}", t)
            return out
        (qd, sd), (qf, sf) = self._q(f"{site}.depth", depth), self._q(f"{site}.feat", feat)
        s_out = self._scales[f"{site}.out"]
        out = self.fp.bev_pool_v2_int8(qd.contiguous(), qf.contiguous(), *args, sd, sf, s_out, out_height, out_width)
        return self._dq(out, s_out, depth.dtype)

    bev_pool_v2_2 = bev_pool_v2


FUSED_QUANT = {"enabled": os.environ.get("BEVOPS_FUSED_QUANT", "1") != "0"}   # A/B: LinearQ hands the fp16 activation to bevops_linear_int8_fused


class LinearQ(torch.nn.Linear):
    """`LinearQ` of the reference (det2trt/models/utils/register.py:83: pytorch_quantization's
    QuantLinear, selected through LINEAR_LAYERS at modules/spatial_cross_attention.py:58,329): a
    Linear whose input and weight are quantised per tensor (symmetric, amax / 127, round half even,
    clamp to +-127).  Three phases, like the reference's calibrator_qdq flow
    (det2trt/quantization/calibrator_qdq.py:29-80):

      "float"     plain Linear (what a freshly built or un-calibrated module does);
      "calibrate" plain Linear while the calibrator collects the input under `self.site`;
      "int8"      after `freeze()`: the fp16 input goes straight into an int8 x int8 -> int32 GEMM on the matrix
                  cores that quantises it in its operand load, q = clamp(rne(x * fl(1 / s)), +-127)
                  (bevops_linear_int8_fused; FUSED_QUANT off: bevops_quantize_rows, q = clamp(rne(x / s)), then
                  bevops_linear_int8), de-quantising epilogue, output in the input's dtype.

    Deviations from the reference's set-up (det2trt/quantization/calibrator_qdq.py:8-26), both at the level of
    rounding ties / the calibrator's choice, neither of the data flow: pytorch_quantization rounds x * (127 / amax),
    here the scale is s = amax / 127 and the quantiser multiplies by fl(1 / s) (fused) or divides by s (pass) -- the
    three forms agree except on near-ties; and `freeze()` calibrates the WEIGHT with max calibration unless a
    calibrator class is passed (the reference's init_quant_desc gives weights the same calib_method as inputs, "max"
    or "histogram": pass `weight_calibrator=type(self.cal)` for the histogram set-up).

    `fake_quant_reference(x)` is the QuantLinear formula itself -- F.linear(dq(q(x)), dq(q(w))) + b --
    which the int8 path must reproduce up to the fp32 summation order."""

    def __init__(self, in_features, out_features, bias=True, calibrator=None, site=None):
        super().__init__(in_features, out_features, bias)
        self.cal = calibrator
        self.site = site or f"linear@{id(self):x}"
        self.mode = "float"
        self.scale_in = None
        self.register_buffer("weight_q", None, persistent=False)
        self.scale_w = None
        self.bias_f32 = None      # the epilogue's fp32 shift, made once at freeze()

    @classmethod
    def from_linear(cls, lin, calibrator, site):
        m = cls(lin.in_features, lin.out_features, lin.bias is not None, calibrator, site)
        m.weight, m.bias = lin.weight, lin.bias
        return m.to(lin.weight.device, lin.weight.dtype)

    def calibrate(self):
        self.mode = "calibrate"
        return self

    def freeze(self, weight_calibrator=None):
        """Fix the input scale from the collected statistics, quantise the weight (per tensor;
        max calibration unless a calibrator class is given, as QuantDescriptor's weight default)."""
        # (a site without statistics only ever sees empty batches: any positive scale will do)
        self.scale_in = float(self.cal.scale(self.site)) if self.cal.has(self.site) else 1.0
        wc = (weight_calibrator or MinMaxCalibrator)()
        wc.collect("w", self.weight.detach())
        self.scale_w = float(wc.scale("w"))
        self.weight_q = _Base.quantize(self.weight.detach(), self.scale_w).contiguous()
        self.bias_f32 = None if self.bias is None else self.bias.detach().float().contiguous()
        self.mode = "int8"
        return self

    def fake_quant_reference(self, x):
        xq = torch.clamp(torch.round(x.float() / self.scale_in), -127, 127) * self.scale_in
        wq = self.weight_q.float() * self.scale_w
        return torch.nn.functional.linear(xq, wq, None if self.bias is None else self.bias.float())

    def forward(self, x, residual=None, relu=False):
        if self.mode != "int8":
            if self.mode == "calibrate":
                self.cal.collect(self.site, x)
            y = super().forward(x)
            if residual is not None:
                y = y + residual
            return torch.relu(y) if relu else y
        from . import functions as _f
        xh = x if x.dtype == torch.float16 else x.to(torch.float16)
        res = None if residual is None else residual.to(torch.float16)
        if self.bias_f32 is None and self.bias is not None:
            self.bias_f32 = self.bias.detach().float().contiguous()
        # the fp16 activation goes straight into the GEMM (quantised in its operand load: no quantise pass)
        a = xh if FUSED_QUANT["enabled"] and xh.shape[-1] % 16 == 0 else _f.quantize_rows(xh, self.scale_in)
        y = _f.linear_int8(a, self.scale_in, self.weight_q, self.scale_w, self.bias_f32, res, relu)
        return y if y.dtype == x.dtype else y.to(x.dtype)

    def forward_q(self, x, scale_out, relu=False):
        """"int8" mode only: the layer on an fp16 operand with its output requantised to int8 at `scale_out` (a consumer's
        `scale_in`) in the GEMM's epilogue -- bevops_linear_int8_chain, the operand quantised as rne(x / scale_in) from the
        fp32 value inside the operand load.  -> int8 [..., out_features]."""
        assert self.mode == "int8" and x.dtype == torch.float16
        from .functions import int8_chain as C
        return C.linear_int8_chain(x, self.scale_in, self.weight_q, self.scale_w, self.bias_f32, None, 1.0, relu,
                                   torch.int8, scale_out)

    def forward_norm_from_q(self, a_q, residual, norm):
        """"int8" mode only: norm(layer(a_q) + residual) in ONE launch (bevops_tsgemm_s8_ln) on an operand that is already
        int8 at this layer's `scale_in` (what `forward_q` of the producer wrote); residual fp16 or None, `norm` an
        nn.LayerNorm over 256 columns.  -> fp16 [..., 256]."""
        assert self.mode == "int8" and a_q.dtype == torch.int8
        from .functions import int8_chain as C
        return C.linear_int8_ln(a_q, self.scale_in, self.weight_q, self.scale_w, self.bias_f32, residual, 1.0,
                                norm.weight, norm.bias, norm.eps)


class Conv2dQ(torch.nn.Conv2d):
    """`Conv2dQ` (register.py:79: QuantConv2d) for the 1x1 convolutions of the channels-last backbone:
    a 1x1 convolution on NHWC activations is the LinearQ GEMM over the [N*H*W, C] rows.  Other kernel
    sizes stay on the library convolution in the model's dtype (TensorRT is free to do the same)."""

    def __init__(self, conv, calibrator, site):
        assert conv.kernel_size == (1, 1) and conv.groups == 1 and conv.padding == (0, 0)
        super().__init__(conv.in_channels, conv.out_channels, 1, conv.stride, bias=conv.bias is not None)
        self.weight, self.bias = conv.weight, conv.bias
        lin = torch.nn.Linear(conv.in_channels, conv.out_channels, conv.bias is not None)
        lin.weight = torch.nn.Parameter(conv.weight.detach().view(conv.out_channels, conv.in_channels))
        lin.bias = conv.bias
        self.lin = LinearQ.from_linear(lin, calibrator, site)

    def calibrate(self):
        self.lin.calibrate()
        return self

    def freeze(self):
        self.lin.freeze()
        return self

    def forward(self, x):
        s = self.stride[0]
        if s > 1:
            x = x[:, :, ::s, ::s]
        n, c, h, w = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(-1, c)
        y = self.lin(rows.contiguous())
        return y.view(n, h, w, -1).permute(0, 3, 1, 2)


class ConvTapsQ(torch.nn.Conv2d):
    """`Conv2dQ` (register.py:79) for the plain 3x3 convolutions of the channels-last backbone / neck (and, when
    built with a stride, for strided 1x1 convolutions): the same three phases as LinearQ, the int8 phase running
    `bevops_conv_tile_int8_fused` -- fp16 activation quantised inside the kernel's operand load, int8 weights in
    the taps-major layout, de-quantising epilogue with shift / identity / ReLU.  The channels-last data path
    (`bevformer._conv_nhwc`) reads `qmode` / `int8_nhwc`; in the float and calibrate phases it runs this module's
    weights through its ordinary fp16 path (and `collect` sees the input)."""

    def __init__(self, conv, calibrator, site):
        k = conv.kernel_size[0]
        assert conv.kernel_size == (k, k) and k in (1, 3) and conv.groups == 1 and conv.padding == (k // 2, k // 2) \
            and conv.stride[0] == conv.stride[1] and conv.dilation == (1, 1)
        super().__init__(conv.in_channels, conv.out_channels, k, conv.stride, k // 2, bias=conv.bias is not None)
        self.weight, self.bias = conv.weight, conv.bias
        self.cal, self.site, self.qmode = calibrator, site, "float"
        self.scale_in = self.scale_w = None
        self.register_buffer("weight_q", None, persistent=False)
        self.bias_f32 = None
        # prequant: quantise the fp16 input ONCE (one pass over it) and run the int8 implicit GEMM on the int8 copy,
        # instead of quantising inside the operand load -- there every input pixel is re-read and RE-QUANTISED once
        # per tap (nine times for a 3x3), which is what made the fused form lose to the fp16 kernel in round 3
        self.prequant = False

    def calibrate(self):
        self.qmode = "calibrate"
        return self

    def collect(self, x):
        self.cal.collect(self.site, x)

    def freeze(self, weight_calibrator=None):
        self.scale_in = float(self.cal.scale(self.site)) if self.cal.has(self.site) else 1.0
        wc = (weight_calibrator or MinMaxCalibrator)()
        wc.collect("w", self.weight.detach())
        self.scale_w = float(wc.scale("w"))
        self.weight_q = _Base.quantize(self.weight.detach().permute(0, 2, 3, 1), self.scale_w).contiguous()   # taps-major
        self.bias_f32 = None if self.bias is None else self.bias.detach().float().contiguous()
        self.qmode = "int8"
        return self

    def int8_nhwc(self, x, residual=None, relu=False):
        from . import functions as _f
        if self.prequant and residual is None:
            from .functions import int8_chain as C
            q = _f.quantize_rows(x.permute(0, 2, 3, 1), self.scale_in)      # [n, h, w, c]: the channels-last bytes as they lie
            return C.conv_int8_chain_nhwc(q.permute(0, 3, 1, 2), self.scale_in, self.weight_q, self.scale_w, self.bias_f32,
                                          relu, self.stride[0], torch.float16)
        return _f.conv_int8_nhwc(x, self.scale_in, self.weight_q, self.scale_w, self.bias_f32, relu, residual,
                                 self.stride[0])

    def fake_quant_reference(self, x):
        xq = torch.clamp(torch.round(x.float() / self.scale_in), -127, 127) * self.scale_in
        wq = self.weight_q.permute(0, 3, 1, 2).float() * self.scale_w
        return torch.nn.functional.conv2d(xq, wq, None if self.bias is None else self.bias.float(), self.stride,
                                          self.padding)

    def forward(self, x):
        if self.qmode == "int8" and x.is_cuda and x.dtype == torch.float16:
            return self.int8_nhwc(x.contiguous(memory_format=torch.channels_last))
        if self.qmode == "calibrate":
            self.collect(x)
        return super().forward(x)


def quantize_dense_layers(model, calibrator, select=lambda name, mod: True):
    """Swap every nn.Linear of `model` accepted by `select(name, module)` (K % 16 == 0, N % 4 == 0)
    for a LinearQ sharing its parameters and calibrator.  Returns the list of swapped modules; call
    `.calibrate()` on them, run calibration frames, then `.freeze()`."""
    swapped = []
    for name, mod in list(model.named_modules()):
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}" if name else child_name
            if type(child) is torch.nn.Linear and child.in_features % 16 == 0 and child.out_features % 4 == 0 \
                    and select(full, child):
                q = LinearQ.from_linear(child, calibrator, "linear:" + full)
                setattr(mod, child_name, q)
                swapped.append(q)
    return swapped


def quantize_backbone_convs(model, calibrator, select=lambda name, mod: True, conv3x3=False):
    """Swap the 1x1 convolutions of the backbone / neck (bottleneck conv1, conv3, downsample, FPN laterals;
    `Conv2dQ` of the reference, det2trt/models/utils/register.py:79, configs/bevformer/plugin/
    bevformer_base_trt_p2_q.py) for Conv2dQ sharing their parameters: in the channels-last data path they
    are the LinearQ GEMM over the [N*H*W, C] rows with shift / identity / ReLU in its epilogue (a stride goes into
    the int8 GEMM's row addressing).  `conv3x3=True` additionally turns the plain 3x3 convolutions with Cin % 64 == 0
    (bottleneck conv2 of the stages without DCN, FPN output convolutions) into ConvTapsQ (int8 implicit GEMM) -- off
    by default: the implicit GEMM re-reads and RE-QUANTISES an input pixel once per tap, and on one box the INT8
    frame was 6 % slower with them than with the fp16 convolution kernel (18.5 vs 17.5 ms).  The 7x7 stem and the
    DCNv2 pack's offset convolution stay in the model's dtype.  Returns the swapped modules (`.calibrate()`,
    calibration frames, `.freeze()`)."""
    swapped = []
    for name, mod in list(model.named_modules()):
        if not name.startswith(("backbone", "neck")):
            continue
        for child_name, child in list(mod.named_children()):
            full = f"{name}.{child_name}"
            if type(child) is not torch.nn.Conv2d or child.groups != 1 or not select(full, child):
                continue
            q = None
            if child.kernel_size == (1, 1) and child.in_channels % 16 == 0 and child.out_channels % 4 == 0:
                q = Conv2dQ(child, calibrator, "conv:" + full)
            elif conv3x3 and child.kernel_size == (3, 3) and child.padding == (1, 1) and child.dilation == (1, 1) \
                    and child.in_channels % 64 == 0 and child_name != "conv_offset":
                # (the DCNv2 pack's offset convolution feeds sampling positions and stays in fp16)
                q = ConvTapsQ(child, calibrator, "conv:" + full)
            if q is not None:
                q = q.to(child.weight.device, child.weight.dtype)
                setattr(mod, child_name, q)
                swapped.append(q)
    return swapped


class Int8ChainBackbone:
    """The backbone + FPN laterals of the INT8 engine as an int8 ACTIVATION CHAIN (what TensorRT builds from the
    reference's `Conv2dQ` backbone, configs/bevformer/plugin/bevformer_base_trt_p2_q.py, when it keeps the tensors
    between the layers in int8): the stem's pooled output is quantised once; from there every 1x1 / 3x3 / DCNv2
    layer of every bottleneck reads int8 and writes int8 with its consumer's calibrated input scale -- the identity
    rows included -- until the FPN lateral convolutions de-quantise into the fp16 neck.  One byte per element in and
    out of every layer instead of two; no quantise / de-quantise passes.

    Build (like a TensorRT PTQ build, three steps):
        chain = Int8ChainBackbone(model, calibrator)   # swaps the 1x1 convolutions for Conv2dQ, arms the taps
        ... calibration frames through the fp16 model ...
        chain.freeze()                                 # scales + int8 weights; model.extract_feat now runs the chain

    Layer arithmetic: `functions/int8_chain.py` (int8 x int8 -> int32 on the matrix cores, requantising epilogues;
    the DCNv2 block is the INT8 plugin's arithmetic on channels-last int8 tensors)."""

    def __init__(self, model, calibrator, weight_calibrator=None):
        self.model, self.cal, self.ready = model, calibrator, False
        self.wcal = weight_calibrator or MinMaxCalibrator
        self.convs = quantize_backbone_convs(model, calibrator)
        for m in self.convs:
            m.calibrate()
        for si, stage in enumerate(model.backbone.stages):
            for bi, blk in enumerate(stage):
                blk.chain_cal, blk.chain_site = calibrator, f"chain:{si}.{bi}"
                if hasattr(blk.conv2, "conv_offset"):
                    blk.conv2.chain_cal, blk.conv2.chain_site = calibrator, f"chain:{si}.{bi}"
        model.int8_chain = self

    # ---- build
    def _wq(self, w):
        wc = self.wcal()
        wc.collect("w", w.detach())
        s = float(wc.scale("w"))
        return _Base.quantize(w.detach(), s), s

    def _scale(self, name):
        if not self.cal.has(name):
            if not any(k.startswith("chain:") for k in self.cal._stats):
                return 1.0          # a rank without cameras fed the backbone empty batches only: placeholder, never used
            raise RuntimeError(f"int8 chain: no calibration statistics for '{name}' -- calibrate through the "
                               "channels-last chain path (the NCHW path does not visit the chain's sites)")
        return float(self.cal.scale(name))

    def freeze(self):
        m = self.model
        for c in self.convs:
            c.freeze()
        for stage in m.backbone.stages:
            for blk in stage:
                blk.chain_cal = None
                if hasattr(blk.conv2, "conv_offset"):
                    blk.conv2.chain_cal = None
        dev = m.backbone.stem.weight.device
        plan = []
        stages = m.backbone.stages
        lat_of = {}                     # stage index -> lateral convolution reading its output
        for l, si in zip(m.neck.lateral, m.backbone.out_indices):
            lat_of[si] = l
        for si, stage in enumerate(stages):
            blocks = []
            for bi, blk in enumerate(stage):
                site = f"chain:{si}.{bi}"
                e = {"s_x": blk.conv1.lin.scale_in, "s_1": self._scale(site + ".t1"), "s_2": blk.conv3.lin.scale_in,
                     "c1": blk.conv1, "c3": blk.conv3, "down": blk.downsample, "s_idt": None}
                if blk.downsample is not None:
                    e["s_idt"] = self._scale(site + ".idt")
                c2 = blk.conv2
                if hasattr(c2, "conv_offset"):       # DCNv2 pack
                    # the chain's offset convolution is the 3x3, one-deform-group form: 18 offsets + 9 mask logits,
                    # padded to 32 output channels (the channels-last INT8 entry reads exactly that layout)
                    if c2.conv_offset.out_channels != 27 or getattr(c2, "deform_groups", 1) != 1:
                        raise NotImplementedError("int8 chain: DCNv2 packs other than 3x3 / deform_groups=1")
                    wq, sw = self._wq(c2.weight)
                    ow = torch.zeros((32,) + tuple(c2.conv_offset.weight.shape[1:]), dtype=torch.float32, device=dev)
                    ow[:27] = c2.conv_offset.weight.detach().float()
                    amax = ow.abs().flatten(1).amax(1).clamp(min=1e-12)        # per output channel (zero rows: any scale)
                    osc = (amax / 127.0)
                    oq = torch.clamp(torch.round(ow / osc.view(-1, 1, 1, 1)), -127, 127).to(torch.int8)
                    ob = torch.zeros(32, dtype=torch.float32, device=dev)
                    ob[:27] = c2.conv_offset.bias.detach().float()
                    e["dcn"] = dict(wq=wq.contiguous(), sw=sw, bias=c2.bias.detach().float().contiguous(),
                                    oq=oq.permute(0, 2, 3, 1).contiguous(), osc=osc.contiguous(), ob=ob,
                                    s_off=self._scale(site + ".offset"), s_mask=self._scale(site + ".mask"),
                                    stride=c2.stride)
                else:
                    wq, sw = self._wq(c2.weight)
                    e["conv"] = dict(wq=wq.permute(0, 2, 3, 1).contiguous(), sw=sw,
                                     bias=c2.bias.detach().float().contiguous(), stride=c2.stride[0])
                blocks.append(e)
            plan.append(blocks)
        # output scale of a block = input scale of what reads it: the next block, the next stage, or the lateral
        for si, blocks in enumerate(plan):
            for bi, e in enumerate(blocks):
                if bi + 1 < len(blocks):
                    e["s_out"] = blocks[bi + 1]["s_x"]
                elif si + 1 < len(plan):
                    e["s_out"] = plan[si + 1][0]["s_x"]
                else:
                    e["s_out"] = lat_of[si].lin.scale_in
        self.plan, self.lat_of = plan, lat_of
        self.s_stem = plan[0][0]["s_x"]
        self.ready = True
        return self

    # ---- run
    @staticmethod
    def _conv1x1(x, s_x, conv, relu, out_dtype, s_out, residual=None, s_res=1.0):
        """x int8 channels-last -> conv (a Conv2dQ, frozen) as the int8 GEMM over its rows; a stride goes into the
        implicit GEMM's row addressing."""
        from .functions import int8_chain as C
        lin = conv.lin
        if conv.stride[0] > 1:
            assert residual is None
            w = lin.weight_q.view(conv.out_channels, 1, 1, conv.in_channels)
            return C.conv_int8_chain_nhwc(x, s_x, w, lin.scale_w, lin.bias_f32, relu, conv.stride[0], out_dtype, s_out)
        n, c, h, w_ = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(-1, c)
        res = None if residual is None else residual.permute(0, 2, 3, 1).reshape(-1, residual.shape[1])
        y = C.linear_int8_chain(rows, s_x, lin.weight_q, lin.scale_w, lin.bias_f32, res, s_res, relu, out_dtype, s_out)
        return y.view(n, h, w_, -1).permute(0, 3, 1, 2)

    @torch.no_grad()
    def __call__(self, img):
        """img [cams, 3, H, W] fp16 -> the FPN's outputs (fp16, channels-last), as model.neck.forward_nhwc gives."""
        import torch.nn.functional as F
        from .functions import int8_chain as C
        m = self.model
        ops = m.ops
        bb = m.backbone
        from .functions.conv import STEM_FUSED, stem_conv_pool
        if (STEM_FUSED["enabled"] and img.is_contiguous() and img.shape[-1] % 2 == 0
                and tuple(bb.stem.weight.shape) == (64, 3, 7, 7) and bb.stem.stride == (2, 2) and bb.stem.padding == (3, 3)):
            x = stem_conv_pool(img, bb.stem.weight, bb.stem.bias, self.s_stem)       # 7x7 stem + pool: one kernel, int8 out
        else:
            x = img.contiguous(memory_format=torch.channels_last)
            y = F.conv2d(x, bb.stem.weight, None, bb.stem.stride, bb.stem.padding)   # 7x7 stem: library convolution
            if not y.is_contiguous(memory_format=torch.channels_last):
                y = y.contiguous(memory_format=torch.channels_last)
            x = C.bias_relu_maxpool_nhwc_int8(y, bb.stem.bias, self.s_stem)
        i8 = torch.int8
        lats = []
        for si, blocks in enumerate(self.plan):
            for e in blocks:
                if e["down"] is not None:
                    idt, s_idt = self._conv1x1(x, e["s_x"], e["down"], False, i8, e["s_idt"]), e["s_idt"]
                else:
                    idt, s_idt = x, e["s_x"]
                t = self._conv1x1(x, e["s_x"], e["c1"], True, i8, e["s_1"])
                if "dcn" in e:
                    d = e["dcn"]
                    om = C.conv_int8_chain_nhwc(t, e["s_1"], d["oq"], d["osc"], d["ob"], False, d["stride"],
                                                torch.float16)
                    t = C.modulated_deformable_conv2d_int8_nhwc(t, e["s_1"], om, d["s_off"], d["s_mask"], d["wq"],
                                                                d["sw"], d["bias"], e["s_2"], True, d["stride"], 1, 1,
                                                                1, 1)
                else:
                    c = e["conv"]
                    t = C.conv_int8_chain_nhwc(t, e["s_1"], c["wq"], c["sw"], c["bias"], True, c["stride"], i8,
                                               e["s_2"])
                x = self._conv1x1(t, e["s_2"], e["c3"], True, i8, e["s_out"], idt, s_idt)
            if si in self.lat_of:
                lats.append(self._conv1x1(x, blocks[-1]["s_out"], self.lat_of[si], False, torch.float16, 1.0))
        return m.neck.topdown_nhwc(lats, ops)


def engine_dense_select(name, mod):
    """Which nn.Linear layers of the re-hosted BEVFormer the INT8 engine runs as LinearQ: the encoder's dense layers
    except (a) TSA's sampling_offsets / attention_weights, whose fp16 form is the split projection (two K = 256 GEMMs
    on the un-concatenated operands, 40 us) where the int8 form needs the [nq, 512] concatenation copy first (50 us
    + 2 x 17 us), and (b) SCA's value_proj, which in fp16 writes the sampler's planes itself.  The decoder (900
    queries: every layer is launch-bound, INT8 buys no time) stays fp16 -- the layer-precision choice a TensorRT
    builder makes by timing; tools/int8_attribution.py has the error side of it."""
    if not name.startswith("encoder."):
        return False
    return not name.endswith(("tsa.sampling_offsets", "tsa.attention_weights", "sca.value_proj"))


def build_int8_engine(B, name, dev, frames, calibrator="entropy", chain=True, dense_select=None, decoder_int8=False,
                      sca_int8=False, calibration_cache=None, block_norm_fused=None):
    """The PTQ build of the re-hosted model that bench.py times (`B` = the bevformer module, `frames` = an iterable
    of (image, can_bus, lidar2img) calibration frames of one scene): int8 activation chain through the backbone
    (Int8ChainBackbone; chain=False: Conv2dQ layers with fp16 tensors between them, the round-3 build), encoder
    dense layers as LinearQ, TSA's MSDA on the INT8 plugin, everything else on the fp16 operators.
    sca_int8=True: the SCA site too runs the INT8 plugin (quantise value / offsets / weights, bevops_msda_forward in
    int8, masked camera sum on the de-quantised result) as the reference's INT8 engines do
    (configs/bevformer/plugin/bevformer_base_trt_p2_q.py) -- instead of the fp16 projected sampler, which is faster
    than every int8 form of that site on MI355X; bench.py reports both builds.
    calibration_cache (a path; `*_device` calibrators only): a file that does not exist is written after calibrating
    from `frames`; one that exists is loaded INSTEAD of calibrating -- no frame is run, `frames` may be empty -- and
    gives the same scales.  Besides the states it holds the MSDA sites' batch sizes, which `site_filter` reads.
    block_norm_fused: the encoder blocks of the returned model with their LayerNorm in the epilogue of the block's last
    int8 GEMM, the FFN's hidden tensor int8 (bevformer._INT8_LN_FUSED; True / False for this model, None = the switch's
    value, off unless BEVOPS_INT8_LN_FUSED=1).
    Returns (model, qops, note)."""
    dtype = torch.float16
    if calibration_cache is not None:
        cal_type = get_calibrator(calibrator) if isinstance(calibrator, str) else type(calibrator)
        if not issubclass(cal_type, _DeviceCalibrator):
            raise ValueError("calibration_cache needs a device calibrator (minmax_device, percentile_device, "
                             "entropy_device)")
    qops = Int8PluginOps(calibrator, channels_last=True, fused_sca=not sca_int8, engine=True)
    qops.int8_ln_fused = None if block_norm_fused is None else bool(block_norm_fused)
    if sca_int8:
        qops._pass = tuple(n for n in qops._pass if not n.startswith("spatial_cross_attention"))
    model = B.BEVFormer(name, ops=qops, seed=0, backbone_layout="nhwc").to(dev, dtype)
    qops.attach(model)
    sel = dense_select or ((lambda n, m: n.startswith(("encoder.", "decoder."))) if decoder_int8 else engine_dense_select)
    q = quantize_dense_layers(model, qops.cal, sel)
    ch = None
    if chain:
        ch = Int8ChainBackbone(model, qops.cal)
        if os.environ.get("BEVOPS_INT8_FPN", "1") != "0":
            # the FPN's 3x3 output convolutions as int8 implicit GEMMs on a pre-quantised copy of their fp16 input
            # (Conv2dQ of the reference's INT8 config; 2x the matrix rate of the fp16 kernel on the frame's largest
            # convolution, 6 x 256 x 116 x 200)
            taps = [m for m in quantize_backbone_convs(model, qops.cal, lambda n, m: n.startswith("neck."), conv3x3=True)
                    if isinstance(m, ConvTapsQ)]
            for m in taps:
                m.prequant = True
            q += taps
    else:
        q += quantize_backbone_convs(model, qops.cal)
    for m in q:
        m.calibrate()
    n = 0
    if calibration_cache is not None and os.path.exists(calibration_cache):
        extra = qops.cal.load_calibration(calibration_cache, dev)
        qops._site_bs = {k: int(v) for k, v in extra["site_bs"].items()}
        n = int(extra["calibration_frames"])
    else:
        r = B.FrameRunner(model, dev, dtype)
        for img, can, l2i in frames:
            r.step(img, can, l2i, "calib")
            n += 1
        if calibration_cache is not None:
            qops.cal.save_calibration(calibration_cache, {"site_bs": qops._site_bs, "calibration_frames": n})
    scales = qops.freeze()
    for m in q:
        m.freeze()
    if ch is not None:
        ch.freeze()
    if not decoder_int8:
        qops.site_filter = lambda site: qops.site_batch(site) != 1      # the decoder's MSDA (batch 1) stays fp16
    note = {"int8_plugin_sites": sum(1 for k in scales if k.endswith(".out") and k.startswith("msda")
                                     and (decoder_int8 or qops.site_batch(k[:-4]) != 1)),
            "int8_dense_layers": len(q), "int8_backbone_layers": (len(ch.convs) + sum(len(b) for b in ch.plan)) if ch else 0,
            "activation_chain": bool(ch), "calibration_frames": n, "sca_site": "int8 plugin" if sca_int8 else "fp16 projected sampler"}
    return model, qops, note


def _calibrated(cal, cache, dev, run, extra):
    """The statistics of a PTQ build in `cal`: an existing calibration cache `cache` is loaded INSTEAD of running frames;
    otherwise run() calibrates (-> the number of frames n) and, given a path, the statistics are saved there with
    extra(n).  -> the number of frames run (0 when the cache was loaded)."""
    from .int8_plan import load_calibration, save_calibration
    if cache is not None and os.path.exists(cache):
        load_calibration(cal, cache, dev if isinstance(cal, _DeviceCalibrator) else None)
        return 0
    n = run()
    if cache is not None:
        save_calibration(cal, cache, extra(n))
    return n


BEVDET_BEV_HALF_BUILDS = ("fp16", "int8")
BEVDET_DEPTHNET_DCN_BUILDS = (None, "int8")


def build_int8_bevdet(D, dev, frames, calibrator="entropy", bev_half="fp16", calibration_cache=None, cfg=None,
                      depthnet_dcn=None):
    """The PTQ build of the re-hosted BEVDet-R50 (BASELINE config 5; `D` = the bevdet module, or a bevdet.BEVDet
    instance whose weights to quantise; `frames` = an iterable of (image, ranks...) calibration inputs): ResNet-50 + FPN
    laterals as the int8 activation chain, bev_pool_v2 on its INT8 plugin flavour.  bev_half="fp16" (the default): the
    small BEV encoder / head convolutions stay fp16.  bev_half="int8": everything behind the image neck runs the int8
    plan of bevdet_int8.py (design/bevdet_int8.md) -- depth_net, the softmax + split and the pooling leaving as int8,
    every BasicBlock, the two bilinear up-samplers, neck, heads; its sites are calibrated during the same frames, on
    the fp16 kernels of BEVDet(bev_half="hip") from each frame's fp16 image features.  calibration_cache (bev_half="int8"):
    a path -- an existing cache is loaded INSTEAD of running frames, otherwise the collected statistics of every site
    (image chain, pooling and BEV half) are saved there (the format of save_calibration / load_calibration).
    Returns (model, qops, note); with bev_half="int8" the model is a bevdet_int8.Int8BEVDet (forward,
    forward_calibrated, bev_half_calibrated, get_candidates, get_bboxes, prepare_bev_half: BEVDetRunner captures it
    unchanged).
    A BEVDepth model (cfg["view_transformer"] == "bevdepth"; `cfg`: the configuration to ask a module `D` for, forwarded
    only when given) is built with bev_half="int8" only: the DepthNet's int8 plan of bevdepth_int8.py in front of the same
    BEV half (design/bevdepth_int8.md), frames = (image, ranks_bev, ranks_depth, ranks_feat, interval_starts,
    interval_lengths, mlp_input), the model a bevdepth_int8.Int8BEVDepth.  The default bev_half="fp16" build of a BEVDepth
    model is not built: NotImplementedError.
    depthnet_dcn: what to do with the DCN layer of a BEVDepth model's DepthNet (use_dcn=True, BEVDEPTH_R50_DCN).  None
    (the default): such a model is refused, NotImplementedError, before any frame runs.  "int8" (with bev_half="int8"):
    the layer joins the plan as two int8 layers -- the pack's offset convolution with fp16 out (the offsets are never
    quantised) and the int8 grouped deformable convolution deform_conv2d_q_nhwc with its own site "dn.dcn"
    (design/bevdepth_dcn_int8.md); note["depthnet_dcn"] = "int8".  "int8" on a model without the layer, or any other
    value: ValueError."""
    if bev_half not in BEVDET_BEV_HALF_BUILDS:
        raise ValueError(f"bev_half = {bev_half!r}: one of {BEVDET_BEV_HALF_BUILDS}")
    if depthnet_dcn not in BEVDET_DEPTHNET_DCN_BUILDS:
        raise ValueError(f"depthnet_dcn = {depthnet_dcn!r}: one of {BEVDET_DEPTHNET_DCN_BUILDS}")
    if calibration_cache is not None and bev_half != "int8":
        raise ValueError("build_int8_bevdet: calibration_cache goes with bev_half='int8'")
    src = D if isinstance(D, torch.nn.Module) else None
    model_cfg = (getattr(src, "cfg", None) if src is not None else cfg) or {}
    if model_cfg.get("view_transformer") == "bevstereo" or (model_cfg.get("depthnet_cfg") or {}).get("stereo", False):
        raise NotImplementedError("build_int8_bevdet: the BEVStereo model (DepthNet(stereo=True): the temporal-stereo cost "
                                  "volume) has no INT8 build (design/bevstereo.md)")
    depthnet = model_cfg.get("view_transformer") == "bevdepth"
    has_dcn = bool(depthnet and ((model_cfg.get("depthnet_cfg") or {}).get("use_dcn", False)
                                 or getattr(getattr(getattr(src, "view", None), "depth_net", None), "use_dcn", False)))
    if has_dcn and depthnet_dcn is None:
        raise NotImplementedError("build_int8_bevdet: the DepthNet's DCN layer (use_dcn=True) is built in INT8 on request "
                                  "only: pass depthnet_dcn=\"int8\" with bev_half=\"int8\" (design/bevdepth_dcn_int8.md), or "
                                  "build the model with use_dcn=False (BEVDEPTH_R50)")
    if depthnet_dcn is not None and not has_dcn:
        raise ValueError(f"build_int8_bevdet: depthnet_dcn = {depthnet_dcn!r}, but the model's DepthNet has no DCN layer "
                         "(a BEVDepth model with depthnet_cfg use_dcn=True, BEVDEPTH_R50_DCN)")
    if depthnet and bev_half != "int8":
        raise NotImplementedError("build_int8_bevdet: the bev_half='fp16' build of a BEVDepth model is not built (its "
                                  "DepthNet has an int8 plan only in front of the int8 BEV half); pass bev_half=\"int8\" "
                                  "(design/bevdepth_int8.md)")
    if src is not None:
        from . import bevdet as D
    kw = {}
    if src is not None and depthnet:
        kw["cfg"] = src.cfg
    elif src is None and cfg is not None:
        kw["cfg"] = cfg
    qops = Int8PluginOps(calibrator, channels_last=True)
    model = D.BEVDet(ops=qops, seed=0, **kw).to(dev, torch.float16)
    if src is not None:
        model.load_state_dict(src.state_dict())
    model.view.ops = qops
    ch = Int8ChainBackbone(model, qops.cal)
    if bev_half == "int8":
        return _build_int8_bevdet_bev_half(model, qops, ch, dev, frames, calibration_cache, depthnet, depthnet_dcn)
    n = 0
    for f in frames:
        qops.begin_frame()
        model(*f)
        n += 1
    scales = qops.freeze()
    ch.freeze()
    model.register_forward_pre_hook(lambda m, args: qops.begin_frame())
    note = {"int8_plugin_sites": sum(1 for k in scales if k.startswith("bev_pool") and k.endswith(".out")),
            "int8_backbone_layers": len(ch.convs) + sum(len(b) for b in ch.plan), "activation_chain": True,
            "calibration_frames": n}
    return model, qops, note


def _build_int8_bevdet_bev_half(model, qops, ch, dev, frames, calibration_cache, depthnet=False, depthnet_dcn=None):
    """build_int8_bevdet(bev_half="int8") behind the construction of the image chain: the calibration frames (or the
    cache), the freeze, the Int8BEVDet (depthnet: the Int8BEVDepth) around the model."""
    from . import bevdet_int8 as _bi
    if depthnet:
        from . import bevdepth_int8 as _plan
    else:
        _plan = _bi
    cal = qops.cal

    def run():
        inner, seen, n = model.image_features, {}, 0

        def image_features(image):        # (keeps each frame's fp16 image features for the BEV half's calibration)
            seen["x"] = inner(image)
            return seen["x"]

        model.image_features = image_features
        try:
            for f in frames:
                qops.begin_frame()
                model(*f)
                _plan.calibrate_frame(model, seen.pop("x"), f[1:], cal)
                n += 1
        finally:
            del model.image_features
        return n

    n = _calibrated(cal, calibration_cache, dev, run,
                    lambda n: {"model": "bevdepth" if depthnet else "bevdet", "bev_half": "int8", "frames": n})
    scales = qops.freeze()
    ch.freeze()
    model.register_forward_pre_hook(lambda m, args: qops.begin_frame())
    q = (_plan.Int8BEVDepth if depthnet else _bi.Int8BEVDet)(
        model, _bi.scales_from(cal, _plan.build_plan(model).sites, "build_int8_bevdet"))
    note = {"int8_plugin_sites": sum(1 for k in scales if k.startswith("bev_pool") and k.endswith(".out")),
            "int8_backbone_layers": len(ch.convs) + sum(len(b) for b in ch.plan), "activation_chain": True,
            "calibration_frames": n, "bev_half": "int8", "int8_bev_half_layers": q.num_int8_layers,
            "bev_half_scale_sites": len(q.plan.sites)}
    if depthnet:
        front = q.plan.layers[:q.plan.tail]
        note["depthnet_int8_layers"] = sum(1 for l in front if l.op in ("conv", "dcn"))
        note["depthnet_scale_sites"] = len([s for s in q.plan.sites if s.startswith(_bi.SITE_PREFIX + "dn.")])
    if depthnet_dcn is not None:
        note["depthnet_dcn"] = depthnet_dcn
    return q, qops, note


def build_int8_yolox(Y, dev, images, calibrator="entropy", calibration_cache=None, cfg=None, ops=None):
    """The PTQ build of the re-hosted YOLOX (`Y` = the yolox module, or a yolox.YOLOX instance whose weights to
    quantise; `images` = an iterable of fp16 [B, 3, H, W] calibration images): every convolution of the backbone, the
    PAFPN and the head on bevops_conv_slice_s8, every tensor between two layers int8 with one scale per buffer
    (yolox_int8.py, design/yolox_int8.md).  The calibration runs the fp16 fast path and collects every scale group's
    writes under one site; `calibrator` names any of CALIBRATORS.  calibration_cache: a path -- an existing cache is
    loaded INSTEAD of running frames, otherwise the collected statistics are saved there (the calibration-cache
    format of save_calibration / load_calibration).  Returns (model, note): model has forward / get_bboxes / prepare
    like YOLOX, and YOLOXRunner captures it unchanged."""
    from . import yolox_int8 as _yi
    fp = Y if isinstance(Y, torch.nn.Module) else Y.YOLOX(cfg)
    fp = fp.to(dev, torch.float16)
    plan = _yi.build_plan(fp)
    _, num_groups = plan.groups()
    cal = get_calibrator(calibrator)()
    n = _calibrated(cal, calibration_cache, dev, lambda: _yi.calibrate(fp, images, cal, ops),
                    lambda n: {"model": "yolox", "scale_groups": num_groups, "frames": n})
    model = _yi.Int8YOLOX(fp, _yi.group_scales_from(cal, num_groups), ops)
    note = {"int8_layers": model.num_int8_layers, "scale_groups": num_groups, "calibration_frames": n}
    return model, note


def build_int8_centernet(C, dev, images, calibrator="entropy", calibration_cache=None, cfg=None, ops=None, neck="int8"):
    """The PTQ build of the re-hosted CenterNet-R18-DCNv2 (`C` = the centernet module, or a centernet.CenterNet instance
    whose weights to quantise -- a checkpoint loaded through checkpoint.load_centernet_state_dict; `images` = an
    iterable of fp16 [B, 3, H, W] calibration images): the stem's pooled output int8, every BasicBlock convolution on
    bevops_conv_slice_s8(_ex) with the identity in front of the ReLU, the head as two int8 launches, every tensor between
    two layers int8 with one scale per tensor (centernet_int8.py, design/centernet_int8.md).  neck="int8": the DCNv2 packs
    on the int8 channels-last block and the up-sampling layers on bevops_deconv4x4s2_s8 (the reference's implicit INT8
    build); neck="fp16": the neck stays the fp16 CTResNetNeck (the reference's explicit-quantisation config).  The
    calibration runs the fp16 fast path and collects one site per tensor; `calibrator` names any of CALIBRATORS.
    calibration_cache: a path -- an existing cache is loaded INSTEAD of running frames, otherwise the collected
    statistics are saved there (the format of save_calibration / load_calibration; one cache serves both neck modes).
    Returns (model, note): model has forward / get_bboxes / prepare / cfg like CenterNet, and CenterNetRunner captures it
    unchanged."""
    from . import centernet_int8 as _ci
    fp = C if isinstance(C, torch.nn.Module) else C.CenterNet(cfg)
    fp = fp.to(dev, torch.float16)
    cal = get_calibrator(calibrator)()
    n = _calibrated(cal, calibration_cache, dev, lambda: _ci.calibrate(fp, images, cal, ops),
                    lambda n: {"model": "centernet", "sites": len(_ci.all_sites(fp)), "frames": n})
    model = _ci.Int8CenterNet(fp, _ci.scales_from(cal, _ci.build_plan(fp, neck).sites, "build_int8_centernet"), ops, neck)
    note = {"int8_layers": model.num_int8_layers, "scale_sites": len(model.plan.sites), "calibration_frames": n,
            "neck": model.neck_note}
    return model, note
