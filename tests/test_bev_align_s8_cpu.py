"""CPU-only: every status of bevops_bev_align_stack_s8 in the documented order (the entry answers before any device
call), `bev_align_stack_q_plain` on a case computed by hand, and the INT8 build of a temporal model without a GPU: the
refusal of the default bev_half, the plan's counts and the calibration cache's round trip of the new sites."""
import ctypes

import pytest
import torch


def test_every_status_in_the_documented_order():
    from bevformer_tensorrt_amd.utils import load_library
    lib = load_library()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(**kw):
        a = dict(curr=p, cp=16, hist=p, hp=16, out=p, op=32, meta=p, B=0, H=2, W=3, C=16, T=1)
        a.update(kw)
        return lib.bevops_bev_align_stack_s8(a["curr"], a["cp"], a["hist"], a["hp"], a["out"], a["op"], a["meta"], a["B"],
                                             a["H"], a["W"], a["C"], a["T"], None)

    assert call() == 0                                                        # B == 0: success without a launch
    for bad in (dict(curr=None), dict(hist=None), dict(out=None), dict(meta=None), dict(B=-1), dict(H=0), dict(W=-2),
                dict(C=0), dict(T=0), dict(cp=0), dict(hp=8), dict(op=16), dict(T=2, op=32), dict(cp=24), dict(hp=40),
                dict(op=40), dict(curr=p + 8), dict(hist=p + 2), dict(out=p + 8), dict(meta=p + 4)):
        assert call(**bad) == 2, bad
    for unsupported in (dict(C=8), dict(C=24, cp=32, hp=32, op=48), dict(T=16, op=272), dict(H=0x10000), dict(W=0x10000),
                        dict(B=1 << 9, H=1 << 9, W=1 << 9),                                  # curr reaches 2^31 bytes
                        dict(B=1 << 9, H=1 << 9, W=1 << 8, T=3, op=64),                      # curr does not; the ring and out do
                        dict(B=1 << 9, H=1 << 9, W=1 << 8)):                                 # the ring's 2 slots of 2^30, and out
        assert call(**unsupported) == 3, unsupported
    assert call(B=1, C=8) == 3                                                               # with B > 0 too, no launch
    # the order: BAD_PARAM wins over NOT_SUPPORTED, a pitch below the channels over its alignment
    assert call(C=8, curr=None) == 2 and call(C=24, cp=32, hp=32, op=48, meta=p + 4) == 2
    assert call(T=16, op=256) == 2 and call(C=24, cp=16) == 2 and call(H=0x10000, out=p + 8) == 2
    assert lib.bevops_query(b"bevops_bev_align_stack_s8")


def test_q_plain_statement_by_hand():
    """A 3 x 3 map, one channel pair, shift (0.5, 0.5) and shift (-0.5, 0): weights 1 / 4 and 1 / 2.
    p = [[1, 2, 3], [4, 5, 8], [-7, -8, 100]]:
      (0.5, 0.5): pixel (0, 0) = (1 + 2 + 4 + 5) / 4 = 3; (0, 1) = (2 + 3 + 5 + 8) / 4 = 4.5 -> 4 (tie to even);
                  (1, 0) = (4 + 5 - 7 - 8) / 4 = -1.5 -> -2 (tie to even); (1, 1) = (5 + 8 - 8 + 100) / 4 = 26.25 -> 26;
                  column 2 has its right corners outside: (0, 2) = (3 + 8) / 4 = 2.75 -> 3, (1, 2) = (8 + 100) / 4 = 27,
                  row 2 its lower corners: (2, 0) = (-7 - 8) / 4 = -3.75 -> -4, (2, 1) = 92 / 4 = 23, (2, 2) = 25.
      (-0.5, 0):  x0 = -1 outside for column 0: (r, 0) = p[r][0] / 2 -> 0.5 -> 0, 2, -3.5 -> -4; column 1 = (p0 + p1) / 2 ->
                  1.5 -> 2, 4.5 -> 4, -7.5 -> -8; column 2 = (p1 + p2) / 2 -> 2.5 -> 2, 6.5 -> 6, 46.
    The second channel holds -p: ties mirror (-4.5 -> -4, 1.5 -> 2); +-127 clamps (-128 in the map stays -127)."""
    from bevformer_tensorrt_amd.functions import bev_align_stack, bev_align_stack_q_plain, pack_bev_align_meta
    p = torch.tensor([[1, 2, 3], [4, 5, 8], [-7, -8, 100]], dtype=torch.int8)
    curr = torch.tensor([[9, -9]], dtype=torch.int8).view(1, 2, 1, 1).expand(1, 2, 3, 3).contiguous()
    hist = torch.zeros(3, 1, 2, 3, 3, dtype=torch.int8)
    hist[1, 0, 0], hist[1, 0, 1] = p, -p
    hist[2, 0, 0] = -128
    tf = torch.tensor([[1, 0, 0.5, 0, 1, 0.5], [1, 0, -0.5, 0, 1, 0]]).view(1, 2, 2, 3)
    meta = pack_bev_align_meta(tf, [1, 1], [1, 1], 0)
    ring = hist.clone()
    got = bev_align_stack_q_plain(curr, ring, meta, 2)
    a = torch.tensor([[3, 4, 3], [-2, 26, 27], [-4, 23, 25]], dtype=torch.int8)
    b = torch.tensor([[0, 2, 2], [2, 4, 6], [-4, -8, 46]], dtype=torch.int8)
    assert got.dtype == torch.int8 and got.shape == (1, 6, 3, 3)
    assert torch.equal(got[0, :2], curr[0]) and torch.equal(ring[0], curr) and torch.equal(ring[1:], hist[1:])
    assert torch.equal(got[0, 2], a) and torch.equal(got[0, 3], -a) and torch.equal(got[0, 4], b) and torch.equal(got[0, 5], -b)
    # the clamp, an invalid slice, and the operator's route for int8 tensors that are not on a GPU
    meta = pack_bev_align_meta(torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 2).view(1, 2, 2, 3), [2, 1], [1, 0], 0)
    got = bev_align_stack(curr, hist.clone(), meta, 2)
    assert bool((got[0, 2] == -127).all()) and not bool(got[0, 3].any()) and torch.equal(got[0, 4:], curr[0])


def test_default_bev_half_refuses_a_temporal_model():
    from bevformer_tensorrt_amd.bevdet import BEVDet, BEVDET4D_R50
    from bevformer_tensorrt_amd.quantization import build_int8_bevdet
    with pytest.raises(NotImplementedError, match="temporal"):
        build_int8_bevdet(BEVDet(BEVDET4D_R50, seed=0), torch.device("cpu"), [])


@pytest.mark.parametrize("base,num_adj,pre", [("BEVDET_R50", 1, True), ("BEVDET_R50", 2, False), ("BEVDEPTH_R50", 1, True)])
def test_plan_counts_and_cache_round_trip(base, num_adj, pre, tmp_path):
    """Against the plan of the same model without `temporal`: pre_process adds four convolutions and the sites of their
    three inner tensors; the alignment adds one layer; this frame's map and the stacked buffer are ONE site, which takes
    the place of the pooled map's without pre_process.  BEVDET4D_R50: 33 layers, 28 int8, 30 sites."""
    from bevformer_tensorrt_amd import bevdepth_int8 as DI, bevdet as D, bevdet_int8 as BI
    from bevformer_tensorrt_amd.quantization import MinMaxCalibrator
    mod = DI if base == "BEVDEPTH_R50" else BI
    cfg = getattr(D, base)
    still = mod.build_plan(D.BEVDet(cfg, seed=0))
    fp = D.BEVDet(dict(cfg, temporal=dict(num_adj=num_adj, pre_process=pre)), seed=0)
    plan = mod.build_plan(fp)
    assert len(plan.layers) == len(still.layers) + 1 + 4 * pre and plan.int8_layers == still.int8_layers + 4 * pre
    assert len(plan.sites) == len(still.sites) + (4 if pre else 0) and len(set(plan.sites)) == len(plan.sites)
    if base == "BEVDET_R50" and pre:
        assert (len(plan.layers), plan.int8_layers, len(plan.sites)) == (33, 28, 30)
    k = [l.op for l in plan.layers].index("align")
    align, first = plan.layers[k], plan.layers[k + 1]
    assert align.src == ("pre.b1.out" if pre else "bev") and align.dst == first.src == "stack" and first.key == "s0.b0.down"
    assert plan.site(align.src) == plan.site("stack") == "bevdet.stack" and ("bevdet.bev" in plan.sites) == pre
    table = mod.quantize_operands(fp, plan)
    assert tuple(table["s0.b0.conv1"][0].shape) == (128, 3, 3, (num_adj + 1) * 64)
    assert pre == ("pre.b1.conv2" in table) and (not pre or tuple(table["pre.b1.conv2"][0].shape) == (64, 3, 3, 64))
    cal = MinMaxCalibrator()
    for i, s in enumerate(plan.sites):
        cal.collect(s, torch.full((8,), float(i + 1)))
    path = str(tmp_path / "temporal.calib")
    BI.save_calibration(cal, path, {"model": "bevdet", "bev_half": "int8", "frames": 1})
    again = MinMaxCalibrator()
    BI.load_calibration(again, path)
    scales = BI.scales_from(again, plan.sites)
    assert scales == BI.scales_from(cal, plan.sites) and "bevdet.stack" in scales
    model = mod.Int8BEVDepth(fp, scales) if mod is DI else BI.Int8BEVDet(fp, scales)
    ring = model.new_history(2, "cpu")
    assert model.num_adj == num_adj and ring.dtype == torch.int8 and tuple(ring.shape) == (num_adj + 1, 2, 64, 128, 128)
    assert ring[0].is_contiguous(memory_format=torch.channels_last) and not bool(ring.any())
