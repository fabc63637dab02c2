"""BEVDet's camera front end, the parts that need no GPU: the numpy restatement of PIL's resize against the golden
canvases the reference's own pipeline produced (tests/golden/make_image_prepare_golden.py) and against live PIL, the
host plan builder of the C ABI against the restatement's tables (exactly equal), the augmentation / post-transform
helpers against the reference's values bit for bit, the argument checks that return before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
import util_image_prepare as U

R50 = (900, 1600, 704, 396, 0, 140, 704, 396)


@pytest.fixture(scope="module")
def gold():
    return golden("image_prepare")


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def _geometry(gold, name):
    g = [int(v) for v in gold[f"{name}_geometry"]]
    return (g[0], g[1]), tuple(g[2:6]), bool(g[6]), g[7]      # resize_dims, crop, flip, rotate


@pytest.mark.parametrize("name", list(U.CASES))
def test_restatement_equals_golden_canvases(gold, name):
    dims, crop, flip, rotate = _geometry(gold, name)
    assert rotate == 0
    for kind in ("noise", "checker"):
        raw, want = gold[f"{name}_{kind}_raw"], gold[f"{name}_{kind}_canvas"]
        assert raw.shape[1:3] == U.CASES[name][0] and raw.dtype == want.dtype == np.uint8
        for i in range(len(raw)):
            assert np.array_equal(U.prepare(raw[i], dims, crop, flip), want[i]), (name, kind, i)
        if kind == "checker":
            assert (want == 0).any() and (want == 255).any()


def test_restatement_equals_live_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    sizes = [(900, 1600, 704, 396), (37, 53, 23, 16), (40, 64, 96, 60), (20, 30, 45, 33), (50, 90, 1, 1), (50, 90, 3, 2)]
    sizes += [tuple(int(v) for v in rng.integers(1, 80, 4)) for _ in range(40)]
    for k, (h, w, W, H) in enumerate(sizes):
        img = U.noise(k, 1, h, w)[0] if k % 3 else U.checkerboard(1, h, w, 3)[0]
        want = np.array(Image.fromarray(img).resize((W, H)))
        assert np.array_equal(U.resize(img, W, H), want), (h, w, W, H)


def _plan(lib, geom):
    size = lib.bevops_image_resize_plan_size(*geom)
    assert size > 0 and size % 4 == 0, geom
    buf = np.full(size // 4, -1, np.int32)
    assert lib.bevops_image_resize_plan_build(*geom, buf.ctypes.data, size) == 0, geom
    return buf


def _check_plan(lib, geom):
    H0, W0, rW, rH, x0, y0, x1, y1 = geom
    buf = _plan(lib, geom)
    kx, bx, ksx = U.coeffs(W0, rW)
    ky, by, ksy = U.coeffs(H0, rH)
    assert buf[1:11].tolist() == [H0, W0, rW, rH, x0, y0, x1, y1, ksx, ksy]
    fW, fH = x1 - x0, y1 - y0
    assert len(buf) == 16 + fW * (2 + ksx) + fH * (2 + ksy)
    p = 16
    for n, b, k, ks, lo in ((fW, bx, kx, ksx, x0), (fH, by, ky, ksy, y0)):
        assert np.array_equal(buf[p:p + 2 * n].reshape(n, 2), b[lo:lo + n]), geom
        p += 2 * n
        assert np.array_equal(buf[p:p + n * ks].reshape(n, ks), k[lo:lo + n]), geom
        p += n * ks


def test_plan_build_equals_restatement_fixture_and_r50_geometries(gold, lib):
    for name in U.CASES:
        dims, crop, _, _ = _geometry(gold, name)
        _check_plan(lib, U.CASES[name][0] + dims + crop)
    _check_plan(lib, R50)


def test_plan_build_equals_restatement_every_output_size_from_37(lib):
    for out in range(1, 41):
        _check_plan(lib, (37, 37, out, out, 0, 0, out, out))


def test_python_plan_tables(lib):
    import bevformer_tensorrt_amd as bev
    plan = bev.image_resize_plan(90, 160, (76, 42), (3, 13, 73, 37), "cpu")
    assert plan is bev.image_resize_plan(90, 160, (76, 42), (3, 13, 73, 37), "cpu")        # cached
    bx, kx, by, ky = plan.tables()
    k, b, _ = U.coeffs(160, 76)
    assert np.array_equal(bx.numpy(), b[3:73]) and np.array_equal(kx.numpy(), k[3:73])
    k, b, _ = U.coeffs(90, 42)
    assert np.array_equal(by.numpy(), b[13:37]) and np.array_equal(ky.numpy(), k[13:37])
    assert plan.out_size == (24, 70)
    with pytest.raises(bev.utils.lib.BevopsError):
        bev.image_resize_plan(90, 160, (76, 42), (3, 13, 77, 37), "cpu")                    # crop leaves the image


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def test_augmentation_and_post_transform_bit_for_bit(gold):
    import bevformer_tensorrt_amd as bev
    for name, ((H, W), cfg, flip, scale, _) in U.CASES.items():
        resize, dims, crop, fl, rot = bev.bevdet_test_augmentation(H, W, cfg, flip=flip, scale=scale)
        gdims, gcrop, gflip, grot = _geometry(gold, name)
        assert np.float64(resize).tobytes() == gold[f"{name}_resize"].tobytes()
        assert (tuple(dims), tuple(crop), bool(fl), rot) == (gdims, gcrop, gflip, grot)
        post_rot, post_tran = bev.bevdet_post_transform(resize, crop, fl)
        assert post_rot.dtype == post_tran.dtype == torch.float32
        assert np.array_equal(_bits(post_rot.numpy()), _bits(gold[f"{name}_post_rot"])), name
        assert np.array_equal(_bits(post_tran.numpy()), _bits(gold[f"{name}_post_tran"])), name
    from bevformer_tensorrt_amd.bevdet import DATA_CONFIG_R50
    assert DATA_CONFIG_R50 == U.DATA_CONFIG_R50
    for tag, flip in (("r50", None), ("r50_flip", True)):
        resize, dims, crop, fl, rot = bev.bevdet_test_augmentation(900, 1600, DATA_CONFIG_R50, flip=flip)
        assert (resize, dims, crop, fl, rot) == (0.44, (704, 396), (0, 140, 704, 396), bool(flip), 0)
        post_rot, post_tran = bev.bevdet_post_transform(resize, crop, fl)
        assert np.array_equal(_bits(post_rot.numpy()), _bits(gold[f"{tag}_post_rot"]))
        assert np.array_equal(_bits(post_tran.numpy()), _bits(gold[f"{tag}_post_tran"]))
    post_rot, post_tran = bev.bevdet_post_transform(0.44, (0, 140, 704, 396), False)
    assert torch.equal(post_rot, torch.diag(torch.tensor([0.44, 0.44, 1.0])))
    assert torch.equal(post_tran, torch.tensor([0.0, -140.0, 0.0]))


def test_status_codes_without_a_device(lib):
    size = lib.bevops_image_resize_plan_size(*R50)
    assert size == 4 * (16 + 704 * (2 + 11) + 256 * (2 + 11))
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    m = (ctypes.c_double * 3)(*U.MEAN)
    s = (ctypes.c_double * 3)(*U.STD)
    F16 = 1

    def call(images=p, plan=p, nbytes=size, dtype=F16, out=p, canvas=None, N=6, geom=R50, rotate=0, mean=m, std=s):
        return lib.bevops_image_resize_crop_normalize(images, plan, nbytes, dtype, out, canvas, N, *geom, rotate, mean, std,
                                                      1, 0, 1, None)
    assert call(images=None) == 2 and call(plan=None) == 2 and call(out=None) == 2        # null pointers
    assert call(mean=None) == 2 and call(std=None) == 2
    assert call(N=0) == 2 and call(N=-1) == 2
    assert call(nbytes=size - 4) == 2 and call(nbytes=size + 4) == 2 and call(nbytes=0) == 2   # a plan of another size
    assert call(rotate=5) == 3
    assert call(dtype=2) == 3                                                              # int8 output
    assert call(std=(ctypes.c_double * 3)(1.0, 0.0, 1.0)) == 2
    assert call(geom=(900, 1600, 704, 396, 0, 140, 704, 397)) == 3                         # the crop leaves the image
    assert call(geom=(900, 1600, 704, 396, -1, 140, 703, 396)) == 3
    assert call(geom=(900, 1600, 704, 396, 10, 140, 10, 396)) == 2                         # empty crop
    assert call(geom=(900, 0, 704, 396, 0, 140, 704, 396)) == 2
    far = (4000, 4000, 40, 40, 0, 0, 40, 40)                                               # ratio 100: one tile's window
    assert call(geom=far) == 3                                                             # is 48 MB, not 64 KiB
    assert lib.bevops_image_resize_plan_size(*far) == 0
    assert lib.bevops_image_resize_plan_size(900, 1600, 704, 396, 0, 140, 704, 397) == 0
    assert lib.bevops_image_resize_plan_size(900, 1600, 0, 396, 0, 0, 1, 1) == 0
    host = np.zeros(size // 4, np.int32)
    assert lib.bevops_image_resize_plan_build(*R50, None, size) == 2
    assert lib.bevops_image_resize_plan_build(*R50, host.ctypes.data, size - 4) == 2
    assert lib.bevops_image_resize_plan_build(*far, host.ctypes.data, size) == 3
    assert lib.bevops_image_resize_plan_build(900, 1600, 704, 396, 0, 140, 704, 397, host.ctypes.data, size) == 3
    assert not host.any()                                                                  # nothing was written
    # the documented domain: every per-axis ratio from 1/4 to 4, whatever the size
    for geom in ((4000, 4000, 1000, 1000, 0, 0, 1000, 1000), (1000, 1000, 4000, 4000, 0, 0, 4000, 4000),
                 (2160, 3840, 960, 540, 100, 100, 900, 500)):
        assert lib.bevops_image_resize_plan_size(*geom) > 0


def test_exported_and_not_registered():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd import functions as F
    for name in ("bevdet_test_augmentation", "bevdet_post_transform", "image_resize_plan", "image_resize_crop_normalize"):
        assert getattr(bev, name) is getattr(F, name) and name in F.__all__
        assert name not in bev.TRT_FUNCTIONS
    with pytest.raises(AssertionError):
        bev.image_resize_crop_normalize(torch.zeros(1, 4, 4, 3, dtype=torch.uint8),
                                        bev.image_resize_plan(4, 4, (4, 4), (0, 0, 4, 4), "cpu"))
