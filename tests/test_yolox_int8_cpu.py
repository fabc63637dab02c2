"""CPU-only: the plan of the INT8 build of YOLOX (bevformer_tensorrt_amd/yolox_int8.py): the scale-group union, the
quantised operand table and the calibration cache round trip."""
import numpy as np
import pytest
import torch

from bevformer_tensorrt_amd import quantization as Q
from bevformer_tensorrt_amd import yolox as Y
from bevformer_tensorrt_amd import yolox_int8 as YI


@pytest.fixture(scope="module")
def model():
    return Y.YOLOX(Y.YOLOX_S)


@pytest.fixture(scope="module")
def plan(model):
    return YI.build_plan(model)


def _conv_writing(plan, buf, c0):
    return [s for s in plan.steps if s.op == "conv" and s.dst.buf == buf and s.dst.c0 == c0]


def test_plan_restates_the_fast_path(model, plan):
    convs = [s for s in plan.steps if s.op == "conv"]
    n_act = sum(1 for m in model.modules() if isinstance(m, Y.ConvAct))
    # every ConvAct once, except the six first tower convolutions that run stacked (3 launches), plus 3 packed predictors
    assert len(convs) == n_act - 6 + 3 + 3 == 74
    assert [s.op for s in plan.steps].count("up") == 2 and [s.op for s in plan.steps].count("pool") == 1
    assert plan.steps[0].op == "focus" and plan.bufs[plan.steps[0].dst.buf] == (32, 2, "q")
    assert [plan.bufs[r.buf] for r in plan.outputs] == [(88, 8, "f16"), (88, 16, "f16"), (88, 32, "f16")]
    # a buffer is written completely before it is read, no channel twice
    written = {}
    for s in plan.steps:
        for r in (s.src, s.res):
            if r is not None:
                have = written.get(r.buf, set())
                assert set(range(r.c0, r.c0 + r.C)) <= have, "read before written"
        chans = set(range(s.dst.c0, s.dst.c0 + s.dst.C))
        if s.res is None or (s.res.buf, s.res.c0) != (s.dst.buf, s.dst.c0):
            assert not (chans & written.get(s.dst.buf, set())), "written twice"
        written.setdefault(s.dst.buf, set()).update(chans)
    for b, (C, _, _) in enumerate(plan.bufs):
        assert written[b] == set(range(C))


def test_scale_group_union_on_yolox_s(model, plan):
    gid, n = plan.groups()
    # 62 buffers: 3 fp16 predictor outputs without a group, 59 int8 buffers, 2 unions (one per up-sampler)
    assert len(plan.bufs) == 62 and sum(g is None for g in gid) == 3 and n == 57
    assert sorted(set(g for g in gid if g is not None)) == list(range(n))
    ups = [s for s in plan.steps if s.op == "up"]
    neck, c = model.neck, model.neck.in_channels
    for i, s in enumerate(ups):
        assert s.src.buf != s.dst.buf and gid[s.src.buf] == gid[s.dst.buf]
        # the source is a reduce layer's output in the second half of a bottom-up buffer [down | high]; the
        # destination is the first half of a top-down buffer [up(high) | c]: both buffers whole in ONE group
        width = c[1 - i]
        assert (s.src.c0, s.src.C, s.dst.c0, s.dst.C) == (width, width, 0, width)
        assert plan.bufs[s.src.buf][0] == plan.bufs[s.dst.buf][0] == 2 * width
        red = _conv_writing(plan, s.src.buf, width)
        down = _conv_writing(plan, s.src.buf, 0)
        assert len(red) == 1 and red[0].key is neck.reduce_layers[i]
        assert len(down) == 1 and down[0].key is neck.downsamples[1 - i]
        members = [b for b in range(len(plan.bufs)) if gid[b] == gid[s.src.buf]]
        assert sorted(members) == sorted((s.src.buf, s.dst.buf))
    assert gid[ups[0].src.buf] != gid[ups[1].src.buf]
    # SPP: conv1's quarter and the three pooled quarters are ONE buffer, hence one group
    pool = next(s for s in plan.steps if s.op == "pool")
    assert pool.src.buf == pool.dst.buf and (pool.src.c0, pool.dst.c0, pool.dst.C) == (0, pool.src.C, 3 * pool.src.C)
    # every other group is one buffer
    sizes = np.bincount([g for g in gid if g is not None])
    assert sorted(sizes.tolist()) == [1] * 55 + [2, 2]


def test_yolox_x_plan_counts():
    p = YI.build_plan(Y.YOLOX(Y.YOLOX_X))
    assert sum(1 for s in p.steps if s.op == "conv") == 146 and p.groups()[1] == 129
    # the padded widths: 80 -> 96 channels, never 128
    assert {p.bufs[s.dst.buf][0] for s in p.steps if s.op == "conv" and s.dst.div == 2} == {96}


def test_quantised_operand_table(model, plan):
    table = YI.quantize_operands(model)
    for s in plan.steps:
        if s.op != "conv":
            continue
        w, ws, b = table[s.key]
        assert w.dtype == torch.int8 and ws.dtype == b.dtype == torch.float32
        assert w.shape[0] == s.dst.C == ws.numel() == b.numel() and w.shape[3] == s.src.C
    head, feat = model.bbox_head, model.bbox_head.feat
    w, ws, b = table[("first", 1)]
    a = YI._Y.quantize_weight_taps(head.cls_convs[1][0].weight, head.cls_convs[1][0].bias)
    r = YI._Y.quantize_weight_taps(head.reg_convs[1][0].weight, head.reg_convs[1][0].bias)
    assert torch.equal(w, torch.cat([a[0], r[0]])) and torch.equal(ws, torch.cat([a[1], r[1]]))
    w, ws, b = table[("pred", 0)]
    assert tuple(w.shape) == (88, 1, 1, 2 * feat) and table["slices"] == [(0, 80), (80, 84), (84, 85)]
    assert not w[:80, ..., feat:].any() and not w[80:85, ..., :feat].any()            # block-diagonal
    assert not w[85:].any() and bool((ws[85:] == 1).all()) and not b[85:].any()      # pad rows: scale 1, zero weights
    assert int(w[:85].abs().amax(dim=(1, 2, 3)).min()) == 127


@pytest.mark.parametrize("name", ["minmax", "entropy", "percentile"])
def test_calibration_cache_round_trip_without_a_frame(tmp_path, name, plan):
    """Statistics collected under the group sites, saved, reloaded into a fresh calibrator: equal scales, and
    build_int8_yolox builds from the cache with an EMPTY image list."""
    _, n = plan.groups()
    cal = Q.get_calibrator(name)()
    g = torch.Generator().manual_seed(3)
    for i in range(n):
        for part in range(2):                 # two slices of one group under one site: the joint statistic
            cal.collect(YI.group_site(i), torch.randn((4, 16, 8, 8), generator=g) * (0.5 + i) * (1 + part))
    path = str(tmp_path / f"yolox_{name}.npz")
    YI.save_calibration(cal, path, {"frames": 2})
    fresh = Q.get_calibrator(name)()
    assert YI.load_calibration(fresh, path) == {"frames": 2}
    assert fresh.scales() == cal.scales() and len(cal.scales()) == n
    names, fields, _ = Q.read_calibration_cache(path)                 # the format of the device calibrators' cache
    assert names == [YI.group_site(i) for i in range(n)] and fields["hist"].shape == (n, 2048)
    want = YI.group_scales_from(cal, n)
    model, note = Q.build_int8_yolox(Y.YOLOX(Y.YOLOX_S), "cpu", [], calibrator=name, calibration_cache=path)
    assert model.group_scales == want and all(s > 0 for s in want)
    assert note == {"int8_layers": 74, "scale_groups": 57, "calibration_frames": 0}
    with pytest.raises(ValueError, match="no calibration data"):
        YI.group_scales_from(Q.get_calibrator(name)(), n)


def _unquantised_table(fp):
    """The plan's operand table with the fp32 weights themselves (scale 1): what `quantize_operands` pads and merges,
    without the rounding."""
    taps = lambda w: w.detach().float().permute(0, 2, 3, 1).contiguous()    # noqa: E731
    table, head = {}, fp.bbox_head
    for m in fp.modules():
        if isinstance(m, Y.ConvAct):
            w, b = YI._Y.pad_channels(m.weight.float(), m.bias.float(), groups_in=m.groups_in)
            table[m] = (taps(w), torch.ones(w.shape[0]), b)
    for l in range(len(head.cls_convs)):
        a, r = head.cls_convs[l][0], head.reg_convs[l][0]
        table[("first", l)] = (taps(torch.cat([a.weight, r.weight], 0)), torch.ones(2 * head.feat),
                               torch.cat([a.bias, r.bias], 0).detach().float())
        w, b, slices = Y.merge_yolox_predictors(*((c[l].weight, c[l].bias) for c in (head.conv_cls, head.conv_reg,
                                                                                    head.conv_obj)))
        table[("pred", l)] = (taps(w), torch.ones(w.shape[0]), b.float())
        table["slices"] = slices
    return table


@pytest.mark.parametrize("cfg,size", [("YOLOX_S", (64, 96)), ("YOLOX_X", (32, 64))])
def test_the_plan_without_quantisation_is_the_plain_model(cfg, size):
    """The plan run in fp32 torch ops with nothing quantised (mode "emulate", no scales, the fp32 weights) is the plain
    model: slices, identities, pools, up-sampling, stacked towers and packed predictors are the model's.  Only the fp32
    summation order differs (padded and merged convolutions): 1e-4 of each output's largest value."""
    fp = Y.YOLOX(getattr(Y, cfg))
    image = torch.randn((2, 3) + size, generator=torch.Generator().manual_seed(5))
    plan = YI.build_plan(fp)
    seen = {}
    packed = YI.run_plan(plan, image, "emulate", None, _unquantised_table(fp),
                         collect=lambda g, t: seen.__setitem__(g, seen.get(g, 0) + 1))
    got = YI.split_outputs(packed, [(0, 80), (80, 84), (84, 85)])
    ref = fp(image)
    assert len(got) == len(ref) == 9
    for a, b in zip(got, ref):
        assert tuple(a.shape) == tuple(b.shape)
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    # every group was collected; the two unions from two convolution writers each plus their own
    gid, n = plan.groups()
    assert sorted(seen) == list(range(n))
    up = next(s for s in plan.steps if s.op == "up")
    assert seen[gid[up.src.buf]] == 3                  # reduce layer, down-sample, the backbone's output


def test_int8_model_object_on_the_cpu(model, plan):
    _, n = plan.groups()
    with pytest.raises(ValueError, match="57 scale groups"):
        YI.Int8YOLOX(model, [1.0] * (n - 1))
    with pytest.raises(ValueError, match="positive and finite"):
        YI.Int8YOLOX(model, [1.0] * (n - 1) + [float("inf")])
    q = YI.Int8YOLOX(model, [0.5] * n)
    assert q.num_int8_layers == 74 and q.cfg is model.cfg and next(q.parameters()) is next(model.parameters())
    with pytest.raises(ValueError, match="fp16 CUDA image"):       # no quiet fall-back to eager PyTorch
        q(torch.zeros((1, 3, 64, 64)))
    # a weight reload rebuilds the quantised operands
    t0 = q.operands()
    assert q.operands() is t0 and q.operands(build=False) is t0
    w = model.backbone.stem.conv.weight
    with torch.no_grad():
        w.mul_(2.0)
    assert q.operands(build=False) is None
    t1 = q.operands()
    assert t1 is not t0 and torch.equal(t1[model.backbone.stem.conv][1], t0[model.backbone.stem.conv][1] * 2)
    with torch.no_grad():
        w.mul_(0.5)
