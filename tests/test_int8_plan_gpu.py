"""The INT8 detector builds keep their bits on the GPU (bevformer_tensorrt_amd/int8_plan.py and the four model modules
on top of it): one frame per model by the recipe of tests/test_bevdepth_int8_gpu.py's `int8_bevdet_frame` -- scales from a
formula (no calibration run: nothing but the plan's own kernels decides the bits), the second of two forwards -- against
the sha-256 a build of the commit BEFORE int8_plan.py existed gave on an MI355X in the same visit.  (Int8BEVDet on the
default model: PARENT_INT8_BEVDET_DIGEST in tests/test_bevdepth_int8_gpu.py.)

`scale_list_digest` pins the calibrated scales of the `built` fixtures of tests/test_yolox_int8_gpu.py and
tests/test_centernet_int8_gpu.py (the calibrate-or-cache path of the builders).  The fixtures of
tests/test_bevdet_int8_gpu.py and tests/test_bevdepth_int8_gpu.py are not pinned: two runs of that earlier commit gave
two different scale lists for each of them."""
import pytest
import torch

import test_bevdepth_gpu as TD

pytestmark = pytest.mark.gpu

PARENT_DIGESTS = {
    "centernet.int8": "da9d0304bf310329e43fef98370f69b4d81c5193319c78a473eb652723e7202c",
    "centernet.fp16": "2af965dd211118ab47f22c81120b1420eb86e1366029cd0f2bd5bc720272947e",
    "yolox_s": "f147fbad95e97c9d22cb8add91bd5de38836f6695d5386c76b706dc11e138d05",
    "bevdepth": "b6f55738ecbc53c39c91102651799b1acaa06530bf352f5f2170490565e21d8e",
}


def scale_list_digest(*scales):
    """sha-256 of the sorted (site, scale) lists of one or more {site: scale} tables (a built model's calibrated scales)."""
    import hashlib
    h = hashlib.sha256()
    for table in scales:
        h.update(repr(sorted((k, float(v)) for k, v in table.items())).encode())
    return h.hexdigest()


def _formula(sites):
    return {s: 0.02 + 0.001 * i for i, s in enumerate(sites)}


def centernet_frame(neck):
    from bevformer_tensorrt_amd import centernet_int8 as CI
    from bevformer_tensorrt_amd.centernet import CenterNet
    fp = CenterNet(seed=0).cuda().half()
    model = CI.Int8CenterNet(fp, _formula(CI.build_plan(fp, neck).sites), neck=neck)
    assert model.neck == neck
    img = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(3)).cuda().half()
    model(img)
    return model(img)


def yolox_frame():
    import bevformer_tensorrt_amd.functions as fn
    from bevformer_tensorrt_amd import yolox_int8 as YI
    from bevformer_tensorrt_amd.yolox import YOLOX, YOLOX_S
    fp = YOLOX(YOLOX_S, seed=0, ops=fn).cuda().half()
    n = YI.build_plan(fp).groups()[1]
    model = YI.Int8YOLOX(fp, [0.02 + 0.001 * i for i in range(n)])
    img = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda().half()
    model(img)
    return model(img)


def bevdepth_frame():
    from bevformer_tensorrt_amd import bevdepth_int8 as DI
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    fp = TD._build("hip", torch.float16)
    scales = _formula(DI.build_plan(fp).sites)
    scales["bevdet.depth"] = 1.0 / 127.0
    model = DI.Int8BEVDepth(fp, scales)
    calib = fp.view.calibration_matrices(*jittered_rig(fp.view, 5)).cuda()
    img = torch.randn(1, 6, 3, 256, 704, generator=torch.Generator().manual_seed(3)).cuda().half()
    model.forward_calibrated(img, calib)
    return model.forward_calibrated(img, calib)


FRAMES = {"centernet.int8": lambda: centernet_frame("int8"), "centernet.fp16": lambda: centernet_frame("fp16"),
          "yolox_s": yolox_frame, "bevdepth": bevdepth_frame}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_the_frame_keeps_the_parent_commits_bits(name):
    outs = FRAMES[name]()
    torch.cuda.synchronize()
    got = TD.frame_digest(outs)
    print("frame", name, got)
    assert any(float(o.float().abs().max()) > 0 for o in outs)
    assert got == PARENT_DIGESTS[name]
