"""What the INT8 detector builds share (centernet_int8.py, bevdet_int8.py with bevdepth_int8.py on top, yolox_int8.py):
the plan vocabulary, the statements of a plan convolution, the calibration cache and the model base class.  This module
imports none of the model modules.  design/model.md, "The INT8 plan".

* `Layer`, `Plan`: a list of layers on NAMED tensors.  A tensor is "q" (int8, one scale) or "f16"; a layer with
  into = (buffer, first channel) writes a channel slice of `buffer`, and every slice of a buffer is in the buffer's scale
  group: one calibration site (prefix + group) and one scale for all its writers and its reader.
* `basic_block_layers`: the downsample / conv1 / conv2 walk of a BasicBlock.
* `conv_statement` / `conv_call`: ONE fp32 statement and ONE int8 call of a plan convolution; `into_slice`: where a
  layer with `into` writes, for the statement and for the run.
* `fake_quant`, `scales_from`, `float_operands`, `save_calibration` / `load_calibration`.
* `Int8Model`: scale validation, `scale()`, `num_int8_layers`, the stamped operand cache, the capture guards.
  (yolox_int8.py keeps its own Ref / Step plan and takes the helpers and the base class only.)"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .functions.multi_scale_deformable_attn import _TensorCache
from .functions.yolox_ops import nhwc_empty


def fake_quant(t, scale):
    """Quantise and dequantise: clamp(rne(t * (1 / scale)), -127, 127) * scale with the kernels' fp32 reciprocal."""
    inv = (torch.ones((), dtype=torch.float32) / torch.tensor(scale, dtype=torch.float32)).item()
    return torch.clamp(torch.round(t * inv), -127, 127) * scale


# ---- the plan

class Layer:
    """op: the model's operator name ("conv" is the shared one); src / dst / res: tensor names; into = (buffer, first
    channel): dst is that channel slice of `buffer`; extra: further int8 tensors the layer writes; factor: an up-sampler's;
    dilation, image_bias (the name of an fp16 [n, Cout] tensor added in place of the bias): a convolution's."""

    def __init__(self, op, key, src, dst, res=None, act="none", stride=1, into=None, extra=(), factor=1, dilation=1,
                 image_bias=None):
        self.op, self.key, self.src, self.dst, self.res, self.act, self.stride = op, key, src, dst, res, act, stride
        self.into, self.extra, self.factor, self.dilation, self.image_bias = into, extra, factor, dilation, image_bias


class Plan:
    """prefix: of the calibration sites; int8_ops: the ops that count as int8 layers."""

    def __init__(self, prefix, int8_ops):
        self.prefix, self.int8_ops = prefix, tuple(int8_ops)
        self.layers, self.tensors, self.group, self.buffers = [], {}, {}, {}   # tensors: name -> "q" | "f16", in write order

    def add(self, layer, kind="q"):
        self.layers.append(layer)
        for name in layer.extra + (layer.dst,):
            self.tensors[name] = kind if name == layer.dst else "q"
            self.group[name] = layer.into[0] if (layer.into is not None and name == layer.dst) else name
        return layer.dst

    def readable(self, buffer):
        """The int8 buffer as a tensor a layer reads: its group is itself."""
        self.tensors[buffer], self.group[buffer] = "q", buffer
        return buffer

    @property
    def int8_layers(self):
        return sum(1 for l in self.layers if l.op in self.int8_ops)

    def site(self, tensor):
        return self.prefix + self.group[tensor]

    @property
    def sites(self):
        out = []
        for n, kind in self.tensors.items():
            if kind == "q" and self.site(n) not in out:
                out.append(self.site(n))
        return out


def basic_block_layers(P, blk, name, x, kind="q", into=None):
    """A BasicBlock on the plan P from the tensor x: the downsample (a stage's first block) -> name.idt, conv1 + ReLU ->
    name.t1, conv2 + identity + ReLU with the identity IN FRONT of the ReLU -> name.out (`kind`, `into`: of that last
    tensor).  -> name.out."""
    s = blk.conv1.stride[0]
    idt = x
    if blk.downsample is not None:
        idt = P.add(Layer("conv", name + ".down", x, name + ".idt", stride=s))
    t = P.add(Layer("conv", name + ".conv1", x, name + ".t1", act="relu", stride=s))
    return P.add(Layer("conv", name + ".conv2", t, name + ".out", res=idt, act="relu", into=into), kind)


def basic_block_conv(blk, which):
    """The convolution behind the key name.{down, conv1, conv2} of `basic_block_layers`."""
    return {"down": blk.downsample, "conv1": blk.conv1, "conv2": blk.conv2}[which]


# ---- a plan convolution: its fp32 statement, its int8 call, its place in a buffer

def conv_statement(l, x, operands, res=None, image_bias=None):
    """The fp32 statement of the convolution layer l on x (NCHW fp32 holding q * scale): the dequantised taps-major
    weight, pad (k / 2) * dilation, the per-image bias in place of the bias, the identity in front of the activation."""
    w, ws, b = operands
    wf = (w.float() * ws[:, None, None, None]).permute(0, 3, 1, 2)
    v = F.conv2d(x, wf, b if image_bias is None else None, l.stride, (w.shape[1] // 2) * l.dilation, l.dilation)
    if image_bias is not None:
        v = v + image_bias[:, :, None, None]
    if res is not None:
        v = v + res
    return F.relu(v) if l.act == "relu" else v


def conv_call(ops, l, x, scale_x, operands, res, scale_res, out, scale_out, image_bias=None):
    """The int8 call of the convolution layer l: conv_slice_q_taps' argument list.  scale_out None: fp16 out."""
    w, ws, b = operands
    kw = {}
    if l.dilation != 1 or image_bias is not None:
        kw = dict(dilation=l.dilation, image_bias=image_bias)
    return ops.conv_slice_q_taps(x, scale_x, w, ws, b if image_bias is None else None, l.act, res,
                                 1.0 if res is None else scale_res, l.stride, out, scale_out,
                                 torch.float16 if scale_out is None else torch.int8, res_first=res is not None, **kw)


def stored(plan, name, v, scales, round_f16):
    """What the tensor `name` holds of the statement's fp32 value v: an int8 tensor the fake quantisation with its site's
    scale; an fp16 tensor v rounded to binary16 -- when round_f16 (bevdet_int8, bevdepth_int8: where the kernels round;
    centernet_int8 states its fp16 tensors without that rounding).  scales None: v, nothing is quantised or rounded."""
    if scales is None:
        return v
    if plan.tensors[name] == "q":
        return fake_quant(v, scales[plan.site(name)])
    return v.half().float() if round_f16 else v


def into_slice(plan, l, live, width, alloc):
    """The channel slice [c0, c0 + width) of l.into's buffer among the tensors `live`; alloc(channels) makes the buffer
    when the layer is its first writer (the statement: zeros like its value; the run: nhwc_empty)."""
    buf, c0 = l.into
    if buf not in live:
        live[buf] = alloc(plan.buffers[buf])
    return live[buf][:, c0:c0 + width]


def place(plan, l, live, v):
    """The statement's side of `into`: the value v of l.dst copied into its slice of the buffer.  -> v."""
    if l.into is not None:
        into_slice(plan, l, live, v.shape[1], lambda C: v.new_zeros((v.shape[0], C) + tuple(v.shape[2:]))).copy_(v)
    return v


def out_slice(plan, l, live, src, width, dtype):
    """The run's side of `into`: the slice the layer l writes from its input `src` (None without `into`); the buffer is a
    channels-last tensor of the layer's output size -- src's over the stride, times the up-sampler's factor."""
    if l.into is None:
        return None
    n, _, h, w = src.shape
    f = l.factor
    return into_slice(plan, l, live, width, lambda C: nhwc_empty(n, C, (h - 1) // l.stride * f + f, (w - 1) // l.stride * f + f,
                                                                 src.device, dtype))


def float_operands(sources):
    """{key: (weight [Cout, Cin, k, k], bias or None)} -> the un-quantised operands in the layout of the quantised ones:
    taps-major fp32 weights, unit scales, a zero bias where there is none."""
    return {k: (w.detach().float().permute(0, 2, 3, 1), torch.ones(w.shape[0], device=w.device),
                torch.zeros(w.shape[0], device=w.device) if b is None else b.detach().float()) for k, (w, b) in sources.items()}


# ---- calibration: the cache and the scales

def _save_host_calibration(cal, path, extra):
    """A host calibrator's statistics in the calibration-cache format of the device calibrators
    (quantization.write_calibration_cache): histogram calibrators fill `range` and `hist`, min-max fills `amax`."""
    import numpy as np
    from . import quantization as _q
    names = list(cal._stats)
    n = len(names)
    fields = {k: np.zeros(n, dtype=np.float32) for k in ("range", "amax")}
    fields.update({k: np.zeros(n, dtype=np.uint64) for k in ("count", "nonfinite")})
    fields["batches"] = np.zeros(n, dtype=np.uint32)
    fields["hist"] = np.zeros((n, _q._NUM_BINS), dtype=np.uint64)
    for i, name in enumerate(names):
        st = cal._stats[name]
        if isinstance(st, dict):
            fields["range"][i] = fields["amax"][i] = st["range"]
            fields["hist"][i] = st["hist"].numpy().astype(np.uint64)
            fields["count"][i] = int(fields["hist"][i].sum())
        else:
            fields["range"][i] = fields["amax"][i] = st
    _q.write_calibration_cache(path, names, fields, extra)


def _load_host_calibration(cal, path):
    from . import quantization as _q
    names, fields, extra = _q.read_calibration_cache(path)
    cal._stats = {}
    for i, name in enumerate(names):
        if isinstance(cal, _q._Histogram):
            cal._stats[name] = {"hist": torch.from_numpy(fields["hist"][i].astype("float64")), "range": float(fields["range"][i])}
        else:
            cal._stats[name] = float(fields["amax"][i])
    return extra


def save_calibration(cal, path, extra=None):
    if hasattr(cal, "save_calibration"):
        cal.save_calibration(path, extra)
    else:
        _save_host_calibration(cal, path, extra)


def load_calibration(cal, path, device=None):
    if hasattr(cal, "load_calibration"):
        return cal.load_calibration(path, device)
    return _load_host_calibration(cal, path)


def scales_from(cal, sites, who="the INT8 build"):
    """{site: scale} of the calibrator `cal` for `sites`, as fp32 numbers (what the kernels receive); who: names the
    builder in the message."""
    missing = [s for s in sites if not cal.has(s)]
    if missing:
        raise ValueError(f"{who}: no calibration data for the sites {missing}")
    return {s: float(torch.tensor(cal.scale(s), dtype=torch.float32)) for s in sites}


# ---- the model

class Int8Model(nn.Module):
    """The base of the INT8 models around an fp16 model `fp` (kept: its parameters are this module's, and a weight reload
    rebuilds the int8 operands).  A model gives `self.plan`, calls `_set_scales`, and fills the hooks:

      _quantize()          the operand table from fp's weights                         (required)
      _stamped()           the tensors whose change makes the table stale             (fp's parameters)
      _packs(table, build) further packed images of the table: build them, or say whether all are cached   (none)
      PREPARE, OPERAND     the name of the method that builds the operands, and what the guard's message calls them"""

    PREPARE = "prepare"
    OPERAND = "quantised"

    def __init__(self, fp):
        super().__init__()
        self.fp = fp
        self.cfg = fp.cfg

    def _set_scales(self, scales, sites, what="scale"):
        who = type(self).__name__
        missing = [s for s in sites if s not in scales]
        if missing:
            raise ValueError(f"{who}: no scale for the sites {missing}")
        self.scales = {s: float(scales[s]) for s in sites}
        if not all(0.0 < v < float("inf") for v in self.scales.values()):
            raise ValueError(f"{who}: every {what} is positive and finite")
        self.eval()

    @property
    def num_int8_layers(self):
        return self.plan.int8_layers

    def scale(self, tensor):
        return self.scales[self.plan.site(tensor)]

    # ---- the hooks
    def _quantize(self):
        raise NotImplementedError

    def _stamped(self):
        return self.fp.parameters()

    def _packs(self, table, build):
        return True

    # ---- the cached operands
    def operands(self, build=True):
        """The quantised operands on the device of the weights; cached, stamped with the version of every tensor of
        `_stamped()` and rebuilt when one changes.  build=False: None when missing or stale."""
        stamp = tuple(_TensorCache._stamp(p) for p in self._stamped())
        hit = self.__dict__.get("_operands")
        if hit is not None and hit[0] == stamp and self._packs(hit[1], build=False):
            return hit[1]
        if not build:
            return None
        table = self._quantize()
        self.__dict__["_operands"] = (stamp, table)
        self._packs(table, build=True)
        return table

    def _outside_capture(self):
        """The head of PREPARE: building operands allocates, so it must run OUTSIDE stream capture.  -> a parameter."""
        p = next(self.fp.parameters())
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{type(self).__name__}.{self.PREPARE}() allocates: call it before the capture begins")
        return p

    def _ready(self, like, what="fp16 CUDA tensors"):
        """The operand table for a forward on `like`, built first when missing or stale -- unless the stream is
        capturing: then a missing operand raises before any launch."""
        who = type(self).__name__
        if not (like.is_cuda and like.dtype == torch.float16):
            raise ValueError(f"{who}: {what} (the int8 path has no plain fallback)")
        if self.operands(build=False) is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{who}: a {self.OPERAND} operand is missing or stale and the stream is capturing; "
                                   f"call {self.PREPARE}() (or the model once, eagerly) before the capture")
            getattr(self, self.PREPARE)()
        return self.operands(build=False)
