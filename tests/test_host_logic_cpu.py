"""Host-side logic of the operator layer that needs no GPU: dispatch defaults."""
def test_dense_dispatch_default_without_measurement():
    """functions/linear.py: the choice made when a problem cannot be measured (inside stream capture, or
    BEVOPS_DENSE_TUNE=0): the persistent tall-skinny GEMM for 256-column layers with K >= 256, the library entry
    otherwise; the candidate table names every implementation the measured dispatch picks from."""
    from bevformer_tensorrt_amd.functions import linear as L
    assert L._dense_default(256, 256, True) == "tsgemm"
    assert L._dense_default(256, 1024, False) == "tsgemm"
    assert L._dense_default(256, 64, False) == "blaslt"        # short K: one step per tile, the persistent kernel loses
    assert L._dense_default(512, 256, False) == "blaslt"
    assert L._dense_default(256, 200, False) == "blaslt"       # outside tsgemm's K % 64 domain
    assert set(L._DENSE) == {"tsgemm", "tile", "small", "blaslt", "torch"}
    # rule mode (DETERMINISTIC: camera-sharded runs; NOT what BEVOPS_DENSE_TUNE=0 selects -- that is the default above):
    # a function of the problem alone, on the hand-written kernels only; few rows -> the no-pipeline GEMM
    assert L._dense_deterministic(256, 256, 40000) == "tsgemm"
    assert L._dense_deterministic(192, 256, 40000) == "tile"
    assert L._dense_deterministic(256, 256, 900) == "small"
    assert L._dense_deterministic(512, 256, 900) == "small"
    # ... but not for many-tile problems the shipped table measured 2-3 x slower on it (advisor, round 4)
    assert L._dense_deterministic(2048, 512, 2250) == "tsgemm"
    assert L._dense_deterministic(512, 1024, 4224) == "tsgemm"
    assert L._dense_deterministic(2048, 512, 1056) == "tsgemm"
    assert L._dense_deterministic(256, 200, 900) == "tile"      # outside small_gemm's K % 64 domain
    # shipped table: keys are the problem without the device name
    assert L._problem(("cuda:0", 34800, 256, 1024, True, True, False)) == "34800,256,1024,1,1,0"


def test_own_kernel_dispatch_and_reproducible_table_choices():
    """Round 6: (a) functions/linear.py: OWN_KERNELS -- what the model runs behind its backbone -- takes the fastest
    HAND-WRITTEN candidate of the shipped table's own measurements, never a library one, and the DETERMINISTIC rule for
    a problem the table has not seen; (b) the shipped table never sends a convolution to the library (MIOpen's split
    reduction is not run-to-run reproducible) where the hand-written implicit GEMM is within 5 % of it."""
    import json
    import os
    from bevformer_tensorrt_amd.functions import linear as L
    own = ("tile", "tsgemm", "small")
    measured = L._table()["measured_dense"]
    assert len(measured) > 50
    for prob, times in measured.items():
        m, n, k = (int(v) for v in prob.split(",")[:3])
        key = ("cuda:0", m, n, k) + tuple(bool(int(v)) for v in prob.split(",")[3:])
        got = L._dense_own(key, n, k, m)
        cand = {c: t for c, t in times.items() if c in own}
        assert got in own
        if cand:
            assert times[got] == min(cand.values()), (prob, got, times)
    assert L._dense_own(("cuda:0", 40000, 256, 256, False, True, False), 256, 256, 40000) == "tsgemm"     # library: 13.9 us
    assert L._dense_own(("cuda:0", 40000, 512, 256, True, True, False), 512, 256, 40000) == "tile"
    assert L._dense_own(("cuda:0", 12345, 256, 256, False, True, False), 256, 256, 12345) == "tsgemm"      # unseen: the rule
    assert L._dense_own(("cuda:0", 12345, 192, 256, False, True, False), 192, 256, 12345) == "tile"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = json.load(open(os.path.join(root, "bevformer_tensorrt_amd", "dispatch_gfx950.json")))
    for prob, times in table["measured_us"]["conv"].items():
        if "tile" in times and times["tile"] <= 1.05 * times["library"]:
            assert table["conv"][prob] == "tile", prob
    # the six-camera stride-2 FPN convolution of the base model: the one launch that made the default frame irreproducible
    assert table["conv"]["6,29,50,256,256,3,2,0,0"] == "tile"


def test_frame_runner_hands_every_frame_its_own_calibration():
    """lidar2img is a per-frame input (the reference feeds it to the engine on every frame,
    tools/bevformer/evaluate_trt.py:99,131-132, and its loop builds a fresh tensor per frame, evaluate_pth.py:93 --
    which routinely lands on the address the previous one freed, with version 0): FrameRunner.step keeps no cache of
    it.  The forward of frame k must see frame k's 96 values whether they arrive in a fresh tensor, in the same tensor
    object edited in place, or unchanged -- and it gets no precomputed projection (the model evaluates it per frame)."""
    import numpy as np
    import torch
    from bevformer_tensorrt_amd import bevformer as B

    class Stub(torch.nn.Module):
        bev_h = bev_w = 4
        cfg = {"image": (32, 32)}
        ops = None
        def forward(self, image, prev_bev, use, can_bus, l2i, cams, gather, shift=None, proj=None):
            self.seen = (l2i.clone(), proj, can_bus.clone(), shift.clone())
            return prev_bev, torch.zeros(1), torch.zeros(1)

    def fresh(v):                       # the reference loop's pattern: a new tensor every frame
        return torch.from_numpy(np.full((1, 6, 4, 4), v, dtype=np.float32))

    m = Stub()
    r = B.FrameRunner(m, torch.device("cpu"), torch.float32)
    img, can = torch.zeros(1, 6, 3, 32, 32), torch.zeros(18)
    for k, v in enumerate([1.0, 2.0, 3.0, 3.0, 4.0]):
        t = fresh(v)
        r.step(img, can, t, "scene")
        assert m.seen[0].shape == (1, 6, 4, 4) and bool((m.seen[0] == v).all()), (k, v)
        assert m.seen[1] is None
        del t
    same = fresh(5.0)
    r.step(img, can, same, "scene")
    same.mul_(2.0)                                            # in-place edit of the SAME object
    same[0, 2, 1, 3] = -7.5
    r.step(img, can, same, "other scene")
    assert torch.equal(m.seen[0], same)
    # the other small inputs share the upload: can_bus deltas and the host-evaluated shift are still what they were
    can2 = torch.zeros(18); can2[0], can2[1], can2[-2], can2[-1] = 0.8, -0.3, 0.31, 1.7
    r.step(img, can2, same, "other scene")
    assert torch.equal(m.seen[0], same)
    from bevformer_tensorrt_amd import geometry as G
    assert torch.equal(m.seen[3], G.bev_shift(m.seen[2].clone(), 4, 4, (102.4 / 4, 102.4 / 4)))


def test_deterministic_dispatch_flag_is_per_thread():
    import threading
    from bevformer_tensorrt_amd.functions import linear as L
    L.DETERMINISTIC["enabled"] = True
    seen = []
    t = threading.Thread(target=lambda: seen.append(L.DETERMINISTIC["enabled"]))
    t.start(); t.join()
    try:
        assert seen == [False] and L.DETERMINISTIC["enabled"] is True
    finally:
        L.DETERMINISTIC["enabled"] = False
