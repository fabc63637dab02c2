"""bevops_lss_voxel_prepare_batched on the device through the C ABI: bit-equality with the one-sample entry at B = 1,
the fixture recorded from the reference's own methods at B > 1, the exact composition of B one-sample calls, the
smallest shapes at the digit, tile and wave boundaries, the guarded arena, capture and replay, and the pooling of a batch
of grids (bev_pool_v2_indirect(batch=B))."""
import numpy as np
import pytest
import torch

from util_arena import POISONS, Arena
from util_lss import fixture as fixture_one
from util_lss_batched import cells_of, check_arrays, compose, digest, fixture, grid9, tiny_view, view_for

pytestmark = pytest.mark.gpu

_G, _CASES = fixture()
_G1, _CASES1 = fixture_one()
DEV = "cuda"


def _filled(nbytes, fill):
    return torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device=DEV)


def _abi(vt, calib, batched=True, want_coor=True, fill=0x55, alloc=None):
    """The batched entry (or, batched=False with a 1-D calib, the one-sample entry) with every output and the workspace
    (exactly the queried size) pre-filled with `fill` -> (rb, rd, rf, st, ln, counts, coor) as the kernels left them."""
    import ctypes
    from bevformer_tensorrt_amd.utils import lib as L
    handle = L.load_library()
    alloc = alloc or (lambda nbytes, name: _filled(nbytes, fill))
    frustum = vt.frustum.to(DEV, torch.float32).contiguous()
    calib = calib.to(DEV).contiguous()
    B = calib.shape[0] if batched else 1
    n = (calib.shape[-1] - 9) // 24
    d, h, w, _ = frustum.shape
    num_points = B * n * d * h * w
    cap = min(num_points, B * cells_of(vt))
    i32 = lambda k, name: alloc(k * 4, name).view(torch.int32)
    rb, rd, rf = i32(num_points, "ranks_bev"), i32(num_points, "ranks_depth"), i32(num_points, "ranks_feat")
    st, ln, counts = i32(cap, "interval_starts"), i32(cap, "interval_lengths"), i32(2, "counts")
    coor = alloc(num_points * 12, "coor").view(torch.float32) if want_coor else None
    if batched:
        need = handle.bevops_lss_voxel_prepare_batched_workspace_size(B, n, d, h, w)
        entry = handle.bevops_lss_voxel_prepare_batched
    else:
        need = handle.bevops_lss_voxel_prepare_workspace_size(n, d, h, w)
        entry = handle.bevops_lss_voxel_prepare
    assert need > 0
    ws = alloc(need, "workspace")
    assert ws.numel() == need and ws.data_ptr() % 16 == 0
    status = entry(frustum.data_ptr(), calib.data_ptr(), ctypes.cast(grid9(vt), ctypes.c_void_p), rb.data_ptr(),
                   rd.data_ptr(), rf.data_ptr(), st.data_ptr(), ln.data_ptr(), counts.data_ptr(),
                   coor.data_ptr() if want_coor else None, B, n, d, h, w, ws.data_ptr(), need, L.current_stream_ptr(torch.device(DEV)))
    assert status == 0, status
    torch.cuda.synchronize()
    return rb, rd, rf, st, ln, counts, coor


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8).flatten(),
                                                                     b.contiguous().view(torch.uint8).flatten())


def _np(out):
    return [None if t is None else t.cpu().numpy() for t in out]


def _trim(out):
    """(rb, rd, rf, st, ln) cut at the counts, after asserting zeros behind them; None when nothing is kept"""
    rb, rd, rf, st, ln, counts = _np(out[:6])
    n_pts, n_int = counts.tolist()
    for a, k in ((rb, n_pts), (rd, n_pts), (rf, n_pts), (st, n_int), (ln, n_int)):
        assert 0 <= k <= a.size and not a[k:].any(), "entries at and behind the count are zero"
    if n_int == 0:
        assert n_pts == 0
        return None
    return rb[:n_pts], rd[:n_pts], rf[:n_pts], st[:n_int], ln[:n_int]


def _composition(vt, calib):
    """the batched arrays built from B calls of the ONE-SAMPLE entry"""
    d, h, w, _ = vt.frustum.shape
    n = (calib.shape[1] - 9) // 24
    singles = [_abi(vt, calib[b], batched=False) for b in range(calib.shape[0])]
    arrays = compose([_trim(s) for s in singles], cells_of(vt), n, d * h * w, h * w)
    coor = torch.cat([s[6] for s in singles])
    return arrays, coor


def _check_against_composition(vt, calib, got=None):
    got = got or _abi(vt, calib)
    want, coor = _composition(vt, calib)
    trimmed = _trim(got)
    n_pts, n_int = got[5].tolist()
    assert (n_pts, n_int) == (want[0].size, want[3].size)
    if trimmed is not None:
        for a, b in zip(trimmed, want):
            assert np.array_equal(a, b)
    assert _same_bits(got[6], coor)
    return got


def _check_against_statement(vt, calib, got):
    want = vt.prepare_stable(vt.lidar_coor_plain(calib.cpu()))
    trimmed = _trim(got)
    if trimmed is None:
        assert all(r is None for r in want)
        return
    for a, b in zip(trimmed, want):
        assert np.array_equal(a, b.numpy())
    assert np.array_equal(got[6].cpu().numpy().view(np.int32).reshape(-1), vt.lidar_coor_plain(calib.cpu()).numpy().view(np.int32).reshape(-1))


@pytest.mark.parametrize("case", _CASES1)
def test_batch_one_equals_the_one_sample_entry(case):
    vt = view_for(_G1, case)
    calib = torch.from_numpy(_G1[case + ".calib"])
    old = _abi(vt, calib, batched=False)
    new = _abi(vt, calib.view(1, -1))
    for a, b in zip(old, new):
        assert _same_bits(a, b)


@pytest.mark.parametrize("case", _CASES)
def test_fixture_case(case):
    vt = view_for(_G, case)
    calib = torch.from_numpy(_G[case + ".calib"])
    got = _abi(vt, calib)
    assert digest(got[6].cpu().numpy()) == str(_G[case + ".coor_sha256"])
    assert np.array_equal(got[5].cpu().numpy(), _G[case + ".counts"])
    check_arrays(_G, case, *_trim(got))
    _check_against_statement(vt, calib, got)
    _check_against_composition(vt, calib, got)      # (the empty middle sample of `empty_middle` included)
    if case == "four_r50":
        assert 4 * cells_of(vt) == 65536            # the sort's third digit


def _rigs(vt, B, n_cams, seed=0):
    from bevformer_tensorrt_amd.bevdet import jittered_rig
    rigs = [jittered_rig(vt, 40 + seed + b, n_cams=n_cams) for b in range(B)]
    cat = lambda i: torch.cat([r[i] for r in rigs], 0)
    return vt.calibration_matrices_batched(cat(0), None, cat(2), cat(3), cat(4), cat(5))


SMALL = [  # (d, h, w), cameras, B, (nx, ny, nz): B * cells on both sides of a digit boundary at B = 2, other B beside
    ((3, 2, 5), 1, 2, (127, 1, 1)), ((3, 2, 5), 2, 2, (128, 1, 1)), ((3, 2, 5), 1, 2, (129, 1, 1)),
    ((3, 2, 5), 2, 2, (151, 217, 1)), ((3, 2, 5), 1, 2, (128, 256, 1)), ((3, 2, 5), 2, 2, (331, 99, 1)),
    ((3, 2, 5), 2, 3, (16, 16, 2)), ((3, 2, 5), 1, 5, (51, 1, 1)), ((3, 2, 5), 2, 5, (13, 5, 1)),
    # 1 023 / 1 024 / 1 025 points per sample: the sample boundary before, on and behind a tile edge and inside a wave
    ((3, 11, 31), 1, 2, (16, 16, 1)), ((4, 16, 16), 1, 2, (16, 16, 1)), ((5, 5, 41), 1, 2, (16, 16, 1)),
]


@pytest.mark.parametrize("dhw,n_cams,B,cells", SMALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_smallest_shapes(dhw, n_cams, B, cells):
    vt = tiny_view(*dhw, cells)
    assert cells_of(vt) == cells[0] * cells[1] * cells[2]
    calib = _rigs(vt, B, n_cams)
    got = _check_against_composition(vt, calib)
    _check_against_statement(vt, calib, got)
    n_pts = int(got[5][0])
    assert 0 < n_pts                                  # the geometry keeps something
    if dhw != (3, 2, 5):
        assert B * n_cams * dhw[0] * dhw[1] * dhw[2] in (2046, 2048, 2050)


def test_all_points_of_a_sample_in_one_cell():
    vt = tiny_view(3, 2, 5, (1, 1, 1), span=1000.0, z=(-100.0, 100.0))
    calib = _rigs(vt, 3, 2)
    got = _check_against_composition(vt, calib)
    _check_against_statement(vt, calib, got)
    rb, rd, rf, st, ln = _trim(got)
    assert st.tolist() == [0, 60, 120] and ln.tolist() == [60, 60, 60] and np.array_equal(rd, np.arange(180))
    assert np.array_equal(rb, np.repeat(np.arange(3), 60))


@pytest.mark.parametrize("case", ["empty_middle", "tiny"])
def test_guarded_arena_under_both_poisons(case):
    if case == "tiny":
        vt = tiny_view(3, 11, 31, (16, 16, 1))
        calib = _rigs(vt, 2, 1)
    else:
        vt = view_for(_G, case)
        calib = torch.from_numpy(_G[case + ".calib"])
    results = []
    for poison in POISONS:
        arena = Arena(192 * 1024 * 1024, poison)
        got = _abi(vt, calib, alloc=lambda nbytes, name: arena.carve(nbytes, 16, name, scratch=name == "workspace"))
        arena.check()
        _trim(got)                                    # zeros behind the counts
        results.append([t.clone() for t in got])
        del arena
    for a, b in zip(*results):
        assert _same_bits(a, b)
    _check_against_composition(vt, calib, results[0])


def test_capture_once_replay_three_calibrations():
    from bevformer_tensorrt_amd import functions as F
    vt = tiny_view(5, 5, 41, (16, 16, 2))
    frustum = vt.frustum.to(DEV)
    hosts = [_rigs(vt, 3, 2, seed=10 * k) for k in range(3)]
    calib = torch.zeros_like(hosts[0], device=DEV)
    args = (frustum, calib, vt.grid_lower_bound, vt.grid_interval, vt.grid_size)
    want = []
    for hst in hosts:
        calib.copy_(hst)
        want.append([t.clone() for t in F.lss_voxel_prepare_batched(*args)] + [F.lss_lidar_coor_batched(*args).clone()])
    assert len({tuple(w[5].tolist()) for w in want}) == 3
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.lss_voxel_prepare_batched(*args)
        F.lss_lidar_coor_batched(*args)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = list(F.lss_voxel_prepare_batched(*args)) + [F.lss_lidar_coor_batched(*args)]
    for k in (0, 1, 2, 1, 0):
        calib.copy_(hosts[k])
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, want[k]):
            assert _same_bits(a, b), k
    # the wrapper's trimmed form and its shapes
    calib.copy_(hosts[0])
    trimmed = F.lss_voxel_prepare_batched(*args, padded=False)
    n_pts, n_int = want[0][5].tolist()
    assert trimmed[0].numel() == n_pts and trimmed[3].numel() == n_int
    assert tuple(want[0][6].shape) == (3, 2, 5, 5, 41, 3) and want[0][3].numel() == min(3 * 2 * 1025, 3 * 512)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.int8])
def test_pooling_a_batch_of_grids(dtype):
    """bev_pool_v2_indirect(batch=B) on the batched arrays == the per-sample calls on per-sample arrays, stacked."""
    from bevformer_tensorrt_amd import functions as F
    case = "empty_middle"
    vt = view_for(_G, case)
    calib = torch.from_numpy(_G[case + ".calib"]).to(DEV)
    B, n, (d, h, w) = calib.shape[0], 6, vt.frustum.shape[:3]
    args = lambda c: (vt.frustum.to(DEV), c, vt.grid_lower_bound, vt.grid_interval, vt.grid_size)
    gen = torch.Generator().manual_seed(5)
    if dtype == torch.int8:
        depth = torch.randint(0, 127, (B * n, d, h, w), generator=gen, dtype=torch.int8).to(DEV)
        feat = torch.randint(-127, 127, (B * n, h, w, 64), generator=gen, dtype=torch.int8).to(DEV)
        kw = dict(scales=(1 / 127.0, 0.05, 0.11))
    else:
        depth = torch.rand(B * n, d, h, w, generator=gen).softmax(1).to(dtype).to(DEV)
        feat = torch.randn(B * n, h, w, 64, generator=gen).to(dtype).to(DEV)
        kw = {}
    rb, rd, rf, st, ln, counts = F.lss_voxel_prepare_batched(*args(calib))
    got = F.bev_pool_v2_indirect(depth, feat, rd, rf, rb, st, ln, counts, 128, 128, batch=B, **kw)
    assert tuple(got.shape) == (B, 128, 128, 64)
    want = []
    for b in range(B):
        rb1, rd1, rf1, st1, ln1, c1 = F.lss_voxel_prepare(*args(calib[b]))
        want.append(F.bev_pool_v2_indirect(depth[b * n:(b + 1) * n], feat[b * n:(b + 1) * n], rd1, rf1, rb1, st1, ln1, c1,
                                           128, 128, **kw))
    want = torch.cat(want)
    assert _same_bits(got, want)
    assert not got[1].float().any() and got[0].float().abs().sum() > 0 and got[2].float().abs().sum() > 0
