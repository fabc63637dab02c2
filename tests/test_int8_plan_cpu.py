"""CPU-only: the INT8 detector builds keep their plans, their quantised operands and their launches
(bevformer_tensorrt_amd/int8_plan.py and the four model modules on top of it).

Every digest below was taken from the commit BEFORE int8_plan.py existed (each model module with its own Layer, Plan,
scales_from and operand cache), by this file's own functions: they read the plans through the fields and names that
commit had (a field it lacked reads as the present default), so one description serves both sides.

* PLAN: every layer or step with all its fields, the tensors or buffers in order, sites or groups, buffers, tail;
* OPERANDS: every entry of every `quantize_operands` table -- int8 weights, fp32 scales, fp32 biases (elementwise
  arithmetic on seeded weights: the same bytes on every host);
* CALLS: one `run` on operators that compute nothing (tests/util_*_int8.py: ShapeOps behind ScaleRecorder, every entry
  logged underneath): operator name, every scalar argument -- the scales included --, operand shapes and dtypes.

and the structure the module is there for: one Layer, one Plan, one scales_from, one operand-cache stamp."""
import hashlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bevformer_tensorrt_amd")

PLAN_DIGESTS = {
    "centernet.int8": "35fb86492e549bd4aa9627a7fd6032f7e3f1ce66f865c2a7f510ff40eb405817",
    "centernet.fp16": "b14ba751d19163a67206ff0a045df9674434b5e66c27c64f97f3a1d090279e12",
    "bevdet": "63699d7d27d78589bd929db82b48e9993365e23ca7c01486ce3984a81cdc96bb",
    "bevdepth": "2770f34bf8f30d7c986fdf35d6d3f716a40190004ded2aeb56de94c3394dc9af",
    "yolox_s": "d112ae845ebf9de24f67f50636416c81d0bbf133bae0248739abd3e713983792",
}
OPERAND_DIGESTS = {
    "centernet.int8": "f59557fe79678e0613ed787527340e33ffd19a71da1bf3a33482f6c0a9462e67",
    "centernet.fp16": "338f2bd628885118f37bd5ba4a4d8fd8e3444f876a4f1ea85b0577953f53d90f",
    "bevdet": "9223c50a94679b51986e0f959bd754bee561fe1528521cb8a607ed41e6d6fe97",
    "bevdepth": "d61ef0ed8e8af69af43676db4676252f0bf028756d513037341c7325a602e067",
    "yolox_s": "1f69ca5f9376a74bbb0e6a16ad1e9951e01765b1c5b2ebd672f7b7b9b8ab5682",
}
CALL_DIGESTS = {
    "centernet.int8": "adad9d0f8dd1e9525311e5c86082a6924a69983abaed015f7ee41f0c6427fcb1",
    "centernet.fp16": "b952ff087247b89f48ea4e595613b9ef8ded2811721cf364ec7f67cea3de980f",
    "bevdet": "0b0654813882ff2a73d18ae35fe52707db905859507fe8e20175ed751c784610",
    "bevdepth": "4ac4ee35895b7cbb48b860008ca8520e1d6c398ffb741dcecc35e85e1f70cd7b",
}

LAYER_FIELDS = (("op", None), ("key", None), ("src", None), ("dst", None), ("res", None), ("act", "none"), ("stride", 1),
                ("into", None), ("extra", ()), ("factor", 1), ("dilation", 1), ("image_bias", None))
STEP_FIELDS = ("op", "src", "dst", "key", "res", "act", "stride", "ks")


def _sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


# ---------------------------------------------------------------------------------------------- the models
_MODELS = {}


def fp_model(name):
    if name not in _MODELS:
        if name.startswith("centernet"):
            from bevformer_tensorrt_amd.centernet import CenterNet
            _MODELS[name] = CenterNet(seed=0)
        elif name == "bevdet":
            from bevformer_tensorrt_amd.bevdet import BEVDet
            _MODELS[name] = BEVDet(seed=0)
        elif name == "bevdepth":
            from bevformer_tensorrt_amd.bevdet import BEVDEPTH_R50, BEVDet
            _MODELS[name] = BEVDet(cfg=BEVDEPTH_R50, seed=0)
        else:
            from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
            _MODELS[name] = YOLOX(YOLOX_S, seed=0)
    return _MODELS[name]


def module_of(name):
    import importlib
    return importlib.import_module("bevformer_tensorrt_amd." + {"centernet.int8": "centernet_int8", "centernet.fp16": "centernet_int8",
                                                                "bevdet": "bevdet_int8", "bevdepth": "bevdepth_int8",
                                                                "yolox_s": "yolox_int8"}[name])


def plan_of(name):
    M, fp = module_of(name), fp_model(name)
    return M.build_plan(fp, name.split(".")[1]) if name.startswith("centernet") else M.build_plan(fp)


# ---------------------------------------------------------------------------------------------- descriptions
def describe_plan(name):
    plan, fp = plan_of(name), fp_model(name)
    lines = []
    if name == "yolox_s":
        names = {m: n for n, m in fp.named_modules()}
        ref = lambda r: None if r is None else (r.buf, r.c0, r.C, r.div)
        for s in plan.steps:
            row = {f: getattr(s, f) for f in STEP_FIELDS}
            row.update(src=ref(s.src), dst=ref(s.dst), res=ref(s.res), key=names.get(s.key, s.key))
            lines.append(repr(sorted(row.items())))
        lines.append("bufs " + repr(plan.bufs))
        lines.append("groups " + repr(plan.groups()))
        lines.append("outputs " + repr([ref(r) for r in plan.outputs]))
    else:
        for l in plan.layers:
            lines.append(repr([(f, getattr(l, f, default)) for f, default in LAYER_FIELDS]))
        lines.append("tensors " + repr(list(plan.tensors.items())))
        lines.append("sites " + repr(plan.sites))
        lines.append("buffers " + repr(sorted(getattr(plan, "buffers", {}).items())))
        lines.append("tail " + repr(getattr(plan, "tail", None)))
    return "\n".join(lines)


def _entry_bytes(h, v):
    if isinstance(v, torch.Tensor):
        t = v.detach().cpu().contiguous()
        h.update(repr((str(t.dtype), tuple(t.shape))).encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    elif isinstance(v, float):
        h.update(torch.tensor(v, dtype=torch.float32).numpy().tobytes())
    elif isinstance(v, dict):
        for k in sorted(v):
            h.update(repr(k).encode())
            _entry_bytes(h, v[k])
    elif isinstance(v, (tuple, list)):
        for x in v:
            _entry_bytes(h, x)
    else:
        h.update(repr(v).encode())


def describe_operands(name):
    M, fp = module_of(name), fp_model(name)
    table = M.quantize_operands(fp) if name == "yolox_s" else M.quantize_operands(fp, plan_of(name))
    names = {m: n for n, m in fp.named_modules()}
    rows = sorted(((repr(names.get(k, k)), v) for k, v in table.items()), key=lambda kv: kv[0])
    h = hashlib.sha256()
    for k, v in rows:
        h.update(k.encode())
        _entry_bytes(h, v)
    return h.hexdigest()


class CallLog:
    """Logs every entry called on it -- its name and its arguments as the recorder above it hands them on: tensors as
    (shape, dtype), everything else by value -- and forwards to `inner`."""

    def __init__(self, inner):
        self.inner, self.lines = inner, []

    @staticmethod
    def _show(v):
        if isinstance(v, torch.Tensor):
            return ("tensor", tuple(v.shape), str(v.dtype))
        if isinstance(v, (tuple, list)):
            return tuple(CallLog._show(x) for x in v)
        if isinstance(v, float):
            return repr(float(v))
        return repr(v)

    def __getattr__(self, name):
        entry = getattr(self.inner, name)

        def call(*args, **kwargs):
            self.lines.append(repr((name, tuple(self._show(a) for a in args), sorted((k, self._show(v)) for k, v in kwargs.items()))))
            return entry(*args, **kwargs)
        return call


def formula_scales(sites):
    return {s: 0.02 + 0.001 * i for i, s in enumerate(sites)}


def describe_calls(name, monkeypatch):
    M, fp, plan = module_of(name), fp_model(name), plan_of(name)
    scales = formula_scales(plan.sites)
    if name.startswith("centernet"):
        import util_centernet_int8 as U
        neck = name.split(".")[1]
        shape = U.ShapeOps(fp)
        monkeypatch.setattr(fp.neck, "forward_nhwc", shape.neck_fp16)
        model = M.Int8CenterNet(fp, scales, neck=neck)
        log = CallLog(shape)
        model.run(torch.zeros(1, 3, 64, 96, dtype=torch.float16), model.operands(), U.ScaleRecorder(log))
    else:
        import util_bevdepth_int8 as UD
        import util_bevdet_int8 as UB
        U = UD if name == "bevdepth" else UB
        model = (M.Int8BEVDepth if name == "bevdepth" else M.Int8BEVDet)(fp, scales)
        log = CallLog(U.ShapeOps())
        rec = U.ScaleRecorder(log)
        x = torch.zeros(6, 16, 44, 256, dtype=torch.float16).permute(0, 3, 1, 2)
        pool = lambda d, f, s: rec.bev_pool_v2_int8(d, f, None, None, None, None, None, *s, 128, 128)
        kw = dict(mlp_input=torch.zeros(6, 27)) if name == "bevdepth" else {}
        model.run(x, pool, model.operands(), rec, **kw)
    return "\n".join(log.lines)


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", sorted(PLAN_DIGESTS))
def test_plan_digest(name):
    got = _sha(describe_plan(name))
    print("plan", name, got)
    assert got == PLAN_DIGESTS[name]


@pytest.mark.parametrize("name", sorted(OPERAND_DIGESTS))
def test_operand_digest(name):
    got = describe_operands(name)
    print("operands", name, got)
    assert got == OPERAND_DIGESTS[name]


@pytest.mark.parametrize("name", sorted(CALL_DIGESTS))
def test_call_sequence_digest(name, monkeypatch):
    got = _sha(describe_calls(name, monkeypatch))
    print("calls", name, got)
    assert got == CALL_DIGESTS[name]


def _sources():
    return {f: open(os.path.join(PKG, f)).read() for f in sorted(os.listdir(PKG)) if f.endswith(".py")}


def test_one_layer_one_plan_one_scales_from_one_stamp():
    src = _sources()
    count = lambda pattern: {f: len(re.findall(pattern, t, re.M)) for f, t in src.items() if re.search(pattern, t, re.M)}
    assert count(r"^class Layer\b") == {"int8_plan.py": 1}
    assert count(r"^class DLayer\b") == {}
    assert count(r"^def scales_from\b") == {"int8_plan.py": 1}
    # yolox_int8 keeps its own Ref / Step plan (buffers with channel slices, union-find groups)
    assert count(r"^class Plan\b") == {"int8_plan.py": 1, "yolox_int8.py": 1}
    int8 = ("int8_plan.py", "yolox_int8.py", "centernet_int8.py", "bevdet_int8.py", "bevdepth_int8.py")
    assert {f: src[f].count("_TensorCache._stamp(") for f in int8} == {f: int(f == "int8_plan.py") for f in int8}


def test_the_shared_module_imports_no_model_and_the_models_not_each_other():
    import subprocess
    import sys
    code = ("import sys\n"
            "import bevformer_tensorrt_amd.int8_plan\n"
            "models = ('yolox', 'centernet', 'bevdet', 'bevdepth')\n"
            "for m in models:\n"
            "    for n in (m, m + '_int8'):\n"
            "        assert 'bevformer_tensorrt_amd.' + n not in sys.modules, n\n"
            "import bevformer_tensorrt_amd.centernet_int8, bevformer_tensorrt_amd.bevdet_int8\n"
            "assert 'bevformer_tensorrt_amd.yolox_int8' not in sys.modules\n"
            "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_the_names_the_tests_and_tools_use_stay_where_they_were():
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd import bevdet_int8 as BI
    from bevformer_tensorrt_amd import centernet_int8 as CI
    from bevformer_tensorrt_amd import int8_plan as IP
    from bevformer_tensorrt_amd import yolox_int8 as YI
    for M in (CI, BI, DI, YI):
        assert M.save_calibration is IP.save_calibration and M.load_calibration is IP.load_calibration
        for n in ("build_plan", "quantize_operands", "calibrate" if M in (CI, YI) else "calibrate_frame"):
            assert callable(getattr(M, n)), (M.__name__, n)
    for M in (CI, BI, DI):
        assert M.scales_from is IP.scales_from and M.Layer is IP.Layer and M.Plan is IP.Plan and callable(M.emulate)
    assert CI.SITE_PREFIX == "centernet." and BI.SITE_PREFIX == DI.SITE_PREFIX == "bevdet."
    assert callable(BI.pool_statement) and callable(DI.gates_statement) and callable(CI.all_sites)
    assert all(callable(getattr(YI, n)) for n in ("run_plan", "split_outputs", "group_site", "group_scales_from"))
    for cls in (CI.Int8CenterNet, BI.Int8BEVDet, DI.Int8BEVDepth, YI.Int8YOLOX):
        assert issubclass(cls, IP.Int8Model)
    assert issubclass(DI.Int8BEVDepth, BI.Int8BEVDet)
