"""bevops_stereo_cost_volume_f16 / bevops_stereo_grid (csrc/stereo_cost.hip) through the C ABI in the guarded arena of
tests/util_arena.py, under both poisons, guards intact, equal bits under both, every byte of the output buffer outside
the output slice compared, pad columns exact zeros -- against the float64 statement of tests/util_stereo.py within the
bounds design/bevstereo.md section 4 derives.  prev, curr and out are pitched channel slices of wider buffers.

The kernel's pixel tile is 4 consecutive pixels of the flattened [n, Hc, Wc] index (one pixel per wave of a 256-thread
block): (1, 3, 4, ...) has rows of exactly one tile, the odd shapes and (2, 4, 70, ...) rows that cross tiles and a last
block with idle waves."""
import functools

import pytest
import torch

import util_stereo as U
from conftest import golden
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 24 << 20
# (n, Hc, Wc, C, D): one pixel; odd sizes; a channel chunk past 256 with a tail; maximal D with rows crossing the 4-pixel
# tile; rows of exactly one tile
SHAPES = [(1, 1, 1, 8, 1), (2, 5, 7, 8, 6), (1, 9, 33, 264, 59), (2, 4, 70, 256, 128), (1, 3, 4, 16, 5)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
PAD_IN, PAD_OUT, OFF = 16, 24, 8        # slack channels of the wide buffers; the slices start 8 channels in


@pytest.fixture(scope="module")
def lib():
    from bevformer_tensorrt_amd.utils import load_library
    return load_library()


def dpad_of(D):
    return (D + 7) // 8 * 8


def run(lib, arena, prev, curr, D, bias, grid=None, geom=None, status=0):
    """One call on arena buffers; prev, curr [n, C, Hc, Wc] CPU tensors of fp16-exact values, grid [n, D, Hc, Wc, 2] fp32
    or geom = (consts [n, 40], xs, ys, ds) -> the output slice [n, D, Hc, Wc] on the CPU (fp16).  Checks the guards, the
    slack columns of the output buffer and the pad columns."""
    from bevformer_tensorrt_amd.utils import lib as L
    n, C, H, W = curr.shape
    dp = dpad_of(D)

    def wide(t, name):
        buf = arena.empty((n, C + PAD_IN, H, W), torch.float16, 16, name, channels_last=True)
        buf[:, OFF:OFF + C].copy_(t.half())
        return buf, buf[:, OFF:OFF + C]

    pbuf, pd = wide(prev, "prev")
    cbuf, cd = wide(curr, "curr")
    obuf = arena.empty((n, dp + PAD_OUT, H, W), torch.float16, 16, "output", channels_last=True)
    before = obuf.permute(0, 2, 3, 1).contiguous().view(torch.int16).clone()
    od = obuf[:, OFF:OFF + dp]
    ptrs = [None] * 5
    if grid is not None:
        ptrs[0] = arena.place(grid.float().contiguous(), 8, "grid").data_ptr()
    else:
        keep = [arena.place(t.float().contiguous(), 4, f"geom{i}") for i, t in enumerate(geom)]
        ptrs[1:] = [t.data_ptr() for t in keep]
    stream = L.current_stream_ptr(torch.device("cuda"))
    st = lib.bevops_stereo_cost_volume_f16(pd.data_ptr(), C + PAD_IN, cd.data_ptr(), C + PAD_IN, *ptrs, od.data_ptr(),
                                           dp + PAD_OUT, n, H, W, C, D, dp, float(bias), stream)
    assert st == status
    arena.check()
    after = obuf.permute(0, 2, 3, 1).contiguous().view(torch.int16)
    outside = torch.ones(dp + PAD_OUT, dtype=torch.bool, device="cuda")
    outside[OFF:OFF + dp] = False
    assert torch.equal(after[..., outside], before[..., outside]), "bytes outside the output slice were written"
    out = od.float().cpu()
    assert bool((out[:, D:] == 0).all()) and not bool(torch.signbit(out[:, D:]).any()), "pad columns are exact zeros"
    return od[:, :D].cpu().contiguous()


def run_both(lib, *args, **kw):
    a, b = (run(lib, Arena(CAPACITY, p), *args, **kw) for p in POISONS)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    return a


def check(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = (err - bound).max().item()
    print(f"{what}: max error {err.max().item():.3e}, max (error - bound) {worst:.3e}, max bound {bound.max().item():.3e}")
    assert bool((err <= bound).all()), (what, err.max().item())


def quarter_targets(n, D, H, W, gen):
    """Sample positions on the quarter-pixel lattice from one pixel outside the image to one pixel outside."""
    tx = torch.randint(-4, 4 * W + 1, (n, D, H, W), generator=gen).float() / 4
    ty = torch.randint(-4, 4 * H + 1, (n, D, H, W), generator=gen).float() / 4
    if W == 1:
        tx = torch.zeros_like(tx)
    if H == 1:
        ty = torch.zeros_like(ty)
    return tx, ty


@functools.lru_cache(maxsize=None)
def lattice_case(shape):
    n, H, W, C, D = shape
    g = torch.Generator().manual_seed(11 + sum(shape))
    prev, curr = U.dyadic((n, C, H, W), g), U.dyadic((n, C, H, W), g)
    grid = U.lattice_grid(*quarter_targets(n, D, H, W, g), H, W)
    ix, iy = U.source_pos(grid, H, W)
    assert bool(((ix * 4) == torch.round(ix * 4)).all() and ((iy * 4) == torch.round(iy * 4)).all())    # on the lattice
    return prev, curr, grid, {b: U.ref_cost_volume(prev, curr, grid, b) for b in (0.0, 5.0)}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_quarter_pixel_lattice_dyadic_features(lib, shape):
    """Costs are exact integers over 2^7: the output against the float64 softmax of those exact costs."""
    prev, curr, grid, want = lattice_case(shape)
    for bias in (0.0, 5.0):
        ref = want[bias]
        assert bool((ref["cost"] * 128 == torch.round(ref["cost"] * 128)).all())
        got = run_both(lib, prev, curr, shape[4], bias, grid=grid)
        check(got, ref["prob"], U.softmax_bound(ref["prob"]), f"lattice {shape} bias {bias}")
    if shape[4] > 1 and shape[1] * shape[2] > 1:
        gate = want[5.0]["gate"]
        assert 0.05 < gate.float().mean().item() < 0.95          # the bias is live on part of the volume


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_prev_equals_curr_with_an_identity_grid(lib, shape):
    n, H, W, C, D = shape
    g = torch.Generator().manual_seed(5)
    feat = U.relu_like((n, C, H, W), g)
    # align_corners=True: pixel w sits at 2 w / (W - 1) - 1.  fp32 reaches it within a few ulps of the grid value, not always exactly; every
    # hypothesis of a pixel has the SAME position, hence the same cost and the same gate: an exactly uniform softmax
    gx = torch.linspace(-1, 1, W) if W > 1 else torch.zeros(1)
    gy = torch.linspace(-1, 1, H) if H > 1 else torch.zeros(1)
    grid = torch.stack([gx.view(1, 1, 1, W).expand(n, D, H, W), gy.view(1, 1, H, 1).expand(n, D, H, W)], -1).contiguous()
    ix, iy = U.source_pos(grid, H, W)
    assert (ix - torch.arange(W).float()).abs().max() <= 2.0 ** -16 and \
        (iy - torch.arange(H).float().view(H, 1)).abs().max() <= 2.0 ** -16
    for bias in (0.0, 5.0):             # gate == 0 where the feature is zero: the same bias at every depth of the pixel
        got = run_both(lib, feat, feat, D, bias, grid=grid)
        want = torch.tensor(1.0 / D).half()
        assert bool((got == want).all()), (got.float() - want.float()).abs().max().item()


def test_gate_channel_is_the_first_of_the_last_group(lib):
    n, H, W, C, D = 2, 5, 7, 16, 6
    g = torch.Generator().manual_seed(9)
    prev = (0.25 + U.relu_like((n, C, H, W), g)).half().float()      # strictly positive (and fp16-exact): gate == 0 only where the warp is zero
    curr = U.relu_like((n, C, H, W), g)
    tx, ty = quarter_targets(n, D, H, W, g)
    tx[:, ::2] = -3.0                                   # every other hypothesis fully outside
    grid = U.lattice_grid(tx, ty, H, W)
    base = U.ref_cost_volume(prev, curr, grid, 5.0)
    inside = ~base["gate"]
    assert bool(base["gate"][:, ::2].all()) and inside[:, 1::2].float().mean().item() > 0.5
    check(run_both(lib, prev, curr, D, 5.0, grid=grid), base["prob"], U.general_bound(base["prob"], base["mag"]), "gate base")
    for ch, fires in ((C - 4, True), (C - 3, False), (0, False), (C - 1, False), (C - 8, False)):
        p = prev.clone()
        p[:, ch] = 0
        ref = U.ref_cost_volume(p, curr, grid, 5.0)
        assert bool(ref["gate"].all()) == fires and (fires or torch.equal(ref["gate"], base["gate"]))
        got = run_both(lib, p, curr, D, 5.0, grid=grid)
        check(got, ref["prob"], U.general_bound(ref["prob"], ref["mag"]), f"channel {ch} zeroed")
        if fires:       # the bias at every depth: a softmax does not see it -- the result of bias = 0 on the same input
            none = U.ref_cost_volume(p, curr, grid, 0.0)
            assert (none["prob"] - ref["prob"]).abs().max().item() < 1e-12
            assert (ref["prob"] - base["prob"]).abs().max().item() > 0.05


def test_positions_outside_the_image(lib):
    n, H, W, C, D = 1, 4, 6, 8, 8
    g = torch.Generator().manual_seed(13)
    prev, curr = (0.25 + U.relu_like((n, C, H, W), g)).half().float(), U.relu_like((n, C, H, W), g)
    tx, ty = quarter_targets(n, D, H, W, g)
    grid = U.lattice_grid(tx.clamp(0, W - 1), ty.clamp(0, H - 1), H, W)
    outside = [(-2.0, -2.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.0, -float("inf")), (1e30, -1e30), (-1.5, 3.0)]
    for d, (gx, gy) in enumerate(outside):
        grid[:, d, ..., 0], grid[:, d, ..., 1] = gx, gy
    ref = U.ref_cost_volume(prev, curr, grid, 5.0)
    assert bool(ref["gate"][:, :len(outside)].all()) and not bool(ref["gate"][:, len(outside):].any())
    want_cost = curr.double().abs().sum(1)[:, None] + 5.0                     # a zero warp plus the bias
    assert (ref["cost"][:, :len(outside)] - want_cost).abs().max().item() < 1e-12
    got = run_both(lib, prev, curr, D, 5.0, grid=grid)
    assert bool(torch.isfinite(got).all())
    check(got, ref["prob"], U.general_bound(ref["prob"], ref["mag"]), "outside")
    grid[:] = -2.0                      # everything outside: the uniform distribution
    got = run_both(lib, prev, curr, D, 5.0, grid=grid)
    assert bool((got == torch.tensor(1.0 / D).half()).all())


def test_one_hot_prev_localises_the_four_corners(lib):
    """prev is 1 in ONE channel of ONE pixel, curr is zero, bias 0: the cost of a hypothesis is the bilinear weight its
    sample gives that pixel -- max(0, 1 - |sx - x|) max(0, 1 - |sy - y|), stated independently of the corner logic."""
    n, H, W, C, D = 1, 5, 6, 16, 6
    py, px, ch = 2, 3, 5
    prev, curr = torch.zeros(n, C, H, W), torch.zeros(n, C, H, W)
    prev[0, ch, py, px] = 1.0
    # the pixel as north-west, north-east, south-west and south-east corner, dead on, and out of reach
    offs = [(0.25, 0.25), (-0.75, 0.25), (0.25, -0.75), (-0.75, -0.75), (0.0, 0.0), (1.0, 0.5)]
    tx = torch.stack([torch.full((H, W), px + dx) for dx, _ in offs]).view(1, D, H, W)
    ty = torch.stack([torch.full((H, W), py + dy) for _, dy in offs]).view(1, D, H, W)
    grid = U.lattice_grid(tx, ty, H, W)
    ix, iy = U.source_pos(grid, H, W)
    assert torch.equal(ix, tx) and torch.equal(iy, ty)
    w = torch.tensor([max(0.0, 1 - abs(dx)) * max(0.0, 1 - abs(dy)) for dx, dy in offs], dtype=torch.float64)
    assert w.tolist() == [0.5625, 0.1875, 0.1875, 0.0625, 1.0, 0.0]
    want = torch.softmax(-w, 0).view(1, D, 1, 1).expand(n, D, H, W)
    got = run_both(lib, prev, curr, D, 0.0, grid=grid)
    check(got, want, U.softmax_bound(want), "one-hot")
    ref = U.ref_cost_volume(prev, curr, grid, 0.0)
    assert (ref["prob"] - want).abs().max().item() < 1e-15


def _geometry(n, H, W, D, seed):
    """A plausible rig at the map's size: consts [n, 40] and the frustum tables of create_frustum(downsample=4)."""
    from bevformer_tensorrt_amd.bevdet import LSSViewTransformer, jittered_rig
    from bevformer_tensorrt_amd.functions import stereo_calibration, stereo_frustum_tables
    size = (4 * H, 4 * W)
    cfg = dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 1.0 + D, 1.0])
    view = LSSViewTransformer(grid_config=cfg, input_size=size, downsample=4, in_channels=32, out_channels=16, ops=object())
    _, _, K, pr, pt, _ = jittered_rig(view, seed, n_cams=n)
    pt[0, :, 0] *= size[1] / 704.0
    g = torch.Generator().manual_seed(seed)
    k2s = torch.eye(4).repeat(1, n, 1, 1)
    k2s[0, :, :3, 3] = (torch.rand(n, 3, generator=g) - 0.5) * torch.tensor([0.8, 0.1, 2.5])
    if n > 1:       # the last camera yawed and moved back: part of its volume outside the image, part behind the camera
        k2s[0, -1, 0, 0], k2s[0, -1, 0, 2], k2s[0, -1, 2, 0], k2s[0, -1, 2, 2] = 0.825, 0.565, -0.565, 0.825
        k2s[0, -1, 2, 3] = -1.5
    return (stereo_calibration(k2s, K, pr, pt),) + tuple(stereo_frustum_tables(view.frustum))


def device_grid(lib, geom, n, D, H, W, status=0):
    from bevformer_tensorrt_amd.utils import lib as L
    arena = Arena(CAPACITY, POISONS[0])
    keep = [arena.place(t.float().contiguous(), 4, f"geom{i}") for i, t in enumerate(geom)]
    out = arena.empty((n, D, H, W, 2), torch.float32, 8, "grid")
    st = lib.bevops_stereo_grid(*[t.data_ptr() for t in keep], out.data_ptr(), n, D, H, W,
                                L.current_stream_ptr(torch.device("cuda")))
    assert st == status
    arena.check()
    return out.cpu()


@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS[:4])
def test_computed_grid_equals_the_explicit_grid_bit_for_bit(lib, shape):
    n, H, W, C, D = shape
    geom = _geometry(n, H, W, D, 3)
    grid = device_grid(lib, geom, n, D, H, W)
    g = torch.Generator().manual_seed(17)
    prev, curr = U.relu_like((n, C, H, W), g), U.relu_like((n, C, H, W), g)
    a = run_both(lib, prev, curr, D, 5.0, geom=geom)
    b = run_both(lib, prev, curr, D, 5.0, grid=grid)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    if n > 1 and H * W > 1:
        inside = (grid.abs() <= 1).all(-1)
        assert 0.02 < inside.float().mean().item() < 0.98 and bool((grid == -2).any())


def test_stereo_grid_against_the_fixture(lib):
    """bevops_stereo_grid against the grid the reference's gen_grid computed (tests/golden/bevstereo.npz).  The fp32
    order is matched -- every product, sum and quotient rounded on its own, the 3 x 3 products summed in ascending k --
    so the comparison is bit for bit; `near_plane` (float64 z within 1e-4 of the 1e-3 plane) holds no position in the
    fixture, the mask is applied all the same."""
    from bevformer_tensorrt_amd.functions import stereo_calibration, stereo_frustum_tables
    G = golden("bevstereo")
    t = lambda k: torch.from_numpy(G[k])
    consts = stereo_calibration(t("k2s_sensor"), t("intrins"), t("post_rots"), t("post_trans"))
    got = device_grid(lib, (consts,) + tuple(stereo_frustum_tables(t("cv_frustum"))), 2, 6, 8, 12)
    want, keep = t("grid"), ~t("near_plane")
    assert keep.float().mean().item() >= 0.99
    diff = (got - want)[keep].abs().max().item()
    print(f"bevops_stereo_grid vs gen_grid: max |difference| {diff:.3e} (the reference's own fp32 error {float(G['grid_err']):.3e})")
    assert torch.equal(got[keep].view(torch.int32), want[keep].view(torch.int32))


@functools.lru_cache(maxsize=None)
def gaussian_case(shape):
    n, H, W, C, D = shape
    g = torch.Generator().manual_seed(23 + sum(shape))
    prev, curr = U.relu_like((n, C, H, W), g, 0.7), U.relu_like((n, C, H, W), g, 0.7)
    base = torch.stack(torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")[::-1], -1)
    grid = (base.view(1, 1, H, W, 2) + 0.35 * torch.randn(n, D, H, W, 2, generator=g)).float()
    return prev, curr, grid, U.ref_cost_volume(prev, curr, grid, 5.0)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gaussian_grids_and_features(lib, shape):
    prev, curr, grid, ref = gaussian_case(shape)
    got = run_both(lib, prev, curr, shape[4], 5.0, grid=grid)
    chunks = (shape[3] + 255) // 256
    check(got, ref["prob"], U.general_bound(ref["prob"], ref["mag"], chunks), f"gaussian {shape}")
    if shape[0] * shape[1] * shape[2] * shape[4] >= 200:
        assert 0.05 < ref["gate"].float().mean().item() < 0.95


def test_a_nan_reaches_only_the_pixels_whose_samples_touch_it(lib):
    shape = SHAPES[1]
    prev, curr, grid, ref = gaussian_case(shape)
    n, H, W, C, D = shape
    prev = prev.clone()
    py, px = 2, 3
    prev[0, 1, py, px] = float("nan")
    hit = torch.zeros(n, H, W, dtype=torch.bool)
    for valid, yi, xi in ref["touched"]:        # a corner inside the image is read whatever its weight
        t = valid & (yi == py) & (xi == px)
        t[1:] = False
        hit |= t.any(1)
    assert 0 < int(hit.sum()) < n * H * W
    got = run_both(lib, prev, curr, D, 5.0, grid=grid)
    nan = torch.isnan(got)
    assert torch.equal(nan.all(1), hit) and torch.equal(nan.any(1), hit)          # the whole softmax of such a pixel
    clean = ~hit[:, None].expand_as(got)
    err = (got.double() - ref["prob"]).abs()
    assert bool((err <= U.general_bound(ref["prob"], ref["mag"]))[clean].all())


def test_wrapper_and_graph_replay(lib):
    from bevformer_tensorrt_amd.functions import stereo_cost_volume, stereo_grid
    n, H, W, C, D = SHAPES[1]
    prev, curr, grid, ref = gaussian_case(SHAPES[1])
    dev = lambda t: t.half().cuda().contiguous(memory_format=torch.channels_last)
    p, c, gd = dev(prev), dev(curr), grid.cuda()
    eager = stereo_cost_volume(p, c, gd, D, 5.0)
    assert eager.shape == (n, 8, H, W) and eager.is_contiguous(memory_format=torch.channels_last)
    check(eager[:, :D].cpu(), ref["prob"], U.general_bound(ref["prob"], ref["mag"]), "wrapper")
    first = stereo_cost_volume(None, c, gd, D, 5.0, dpad=32)
    assert first.shape == (n, 32, H, W) and not bool(first.any())
    geom = tuple(t.cuda() for t in _geometry(n, H, W, D, 3))
    static = torch.empty_like(eager)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        stereo_cost_volume(p, c, geom[0], D, 5.0, frustum_tables=geom[1:], out=static)
    torch.cuda.current_stream().wait_stream(stream)
    want = static.clone()
    assert torch.equal(want, stereo_cost_volume(p, c, stereo_grid(geom[0], geom[1:]), D, 5.0))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stereo_cost_volume(p, c, geom[0], D, 5.0, frustum_tables=geom[1:], out=static)
    for _ in range(2):
        static.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static.view(torch.int16), want.view(torch.int16))
