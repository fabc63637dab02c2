"""The three entries of csrc/lss_depthnet.hip through the C ABI in the guarded arena of tests/util_arena.py, under both
poisons: bevops_se_gate2_nhwc and bevops_global_avgpool_nhwc bit for bit against their numpy statements,
bevops_lss_camera_gate against float64 inside derived bounds."""
import functools

import numpy as np
import pytest
import torch

import util_exact_dense as X
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 12 << 20


def _lib():
    from bevformer_tensorrt_amd.utils import lib as L
    return L, L.load_library(), L.current_stream_ptr(torch.device("cuda"))


def _slice(arena, values, pitch, c0, name):
    """values [rows, C] fp16 as channels c0 .. c0 + C of a poisoned [rows, pitch] buffer -> (buffer, view)."""
    rows, C = values.shape
    buf = arena.empty((rows, pitch), torch.float16, 16, name)
    view = buf[:, c0:c0 + C]
    view.copy_(torch.from_numpy(np.array(values)))
    return buf, view


def _outside_untouched(buf, before, c0, C):
    after = buf.cpu().numpy()
    mask = np.zeros(after.shape, bool)
    mask[:, c0:c0 + C] = True
    m8 = np.repeat(mask, 2, axis=-1)
    assert np.array_equal(after.view(np.uint8)[~m8], before[~m8]), "bytes outside the output slice were written"
    return after[:, c0:c0 + C].copy()


# ---------------------------------------------------------------------------------------------- se_gate2
def se_gate2_call(arena, x, gates, n, hw, xlay, alay, blay):
    L, h, st = _lib()
    c = x.shape[1]
    _, xv = _slice(arena, x, c + xlay[0], xlay[1], "x")
    gd = arena.place(torch.from_numpy(gates), 16, "gates")
    abuf = arena.empty((n * hw, c + alay[0]), torch.float16, 16, "out_a")
    bbuf = arena.empty((n * hw, c + blay[0]), torch.float16, 16, "out_b")
    av, bv = abuf[:, alay[1]:alay[1] + c], bbuf[:, blay[1]:blay[1] + c]
    a0, b0 = abuf.cpu().numpy().view(np.uint8).copy(), bbuf.cpu().numpy().view(np.uint8).copy()
    x0 = xv.cpu().numpy().copy()
    rc = h.bevops_se_gate2_nhwc(xv.data_ptr(), c + xlay[0], gd.data_ptr(), av.data_ptr(), c + alay[0], bv.data_ptr(),
                                c + blay[0], n, hw, c, st)
    assert rc == L.SUCCESS
    arena.check()
    assert np.array_equal(xv.cpu().numpy().view(np.int16), x0.view(np.int16))
    return (_outside_untouched(abuf, a0, alay[1], c).view(np.int16), _outside_untouched(bbuf, b0, blay[1], c).view(np.int16))


@pytest.mark.parametrize("c", [8, 72, 256])
@pytest.mark.parametrize("n,hw", [(1, 1), (5, 7), (2, 704)], ids=["1", "35", "1408"])
def test_se_gate2_bits(n, hw, c):
    """float32 product, binary16 rounding; out_a is slice [16, 16 + c) of a buffer of pitch c + 40, x a slice of pitch
    c + 24 at channel 8, out_b dense.  Subnormal and overflowing products included."""
    r = X._rng("se_gate2", n, hw, c)
    x = r.standard_normal((n * hw, c)).astype(np.float16)
    x.reshape(-1)[:4] = np.array([65504.0, -65504.0, 6e-8, 0.0], np.float16)[:min(4, x.size)]
    gates = r.random((2, n, c)).astype(np.float32)
    gates[0, 0, :2] = [1.0, 2.0 ** -12]
    want = [(x.astype(np.float32).reshape(n, hw, c) * gates[b][:, None, :]).astype(np.float16).reshape(n * hw, c)
            for b in (0, 1)]
    got = [se_gate2_call(Arena(CAPACITY, p), x, gates, n, hw, (24, 8), (40, 16), (0, 0)) for p in POISONS]
    for b in (0, 1):
        assert np.array_equal(got[0][b], got[1][b])
        bad = np.argwhere(got[0][b] != want[b].view(np.int16))
        assert len(bad) == 0, f"branch {b}: {len(bad)} of {want[b].size} differ, first at {tuple(bad[0])}"
    assert not np.array_equal(want[0], want[1])


# ---------------------------------------------------------------------------------------------- global average pool
def avgpool_call(arena, x, n, hw, xlay, out_pitch):
    L, h, st = _lib()
    c = x.shape[1]
    _, xv = _slice(arena, x, c + xlay[0], xlay[1], "x")
    obuf = arena.empty((n, out_pitch), torch.float16, 2, "out")
    o0 = obuf.cpu().numpy().view(np.uint8).copy()
    rc = h.bevops_global_avgpool_nhwc(xv.data_ptr(), c + xlay[0], obuf.data_ptr(), out_pitch, n, hw, c, st)
    assert rc == L.SUCCESS
    arena.check()
    return _outside_untouched(obuf, o0, 0, c)


@pytest.mark.parametrize("c", [8, 72, 256])
@pytest.mark.parametrize("n,hw", [(3, 1), (3, 35), (2, 704)], ids=["1", "35", "704"])
def test_global_avgpool_bits_on_integers(n, hw, c):
    """Integers in [-64, 64]: every partial sum is an integer below 2^24, exact in any order, so the result is the
    correctly rounded quotient twice over: fp16(fp32(sum / hw))."""
    r = X._rng("avgpool", n, hw, c)
    x = r.integers(-64, 65, size=(n * hw, c)).astype(np.float16)
    s = x.astype(np.float64).reshape(n, hw, c).sum(axis=1)
    want = (s.astype(np.float32) / np.float32(hw)).astype(np.float16)
    got = [avgpool_call(Arena(CAPACITY, p), x, n, hw, (24, 8), c + 5) for p in POISONS]
    assert np.array_equal(got[0].view(np.int16), got[1].view(np.int16))
    assert np.array_equal(got[0].view(np.int16), want.view(np.int16)), np.argwhere(got[0] != want)[:8]
    assert want.any()


@pytest.mark.parametrize("hw,c", [(35, 72), (704, 256)])
def test_global_avgpool_gaussian_bound_and_repeatability(hw, c):
    """|got - mean64| <= hw 2^-24 mean|x| (fp32 accumulation: at most hw roundings of partial sums that stay below
    sum |x|; the division adds 2^-24 |mean|, covered) + one binary16 step (half a unit in the last place, 2^-11 |mean|,
    and half a subnormal step)."""
    n = 2
    r = X._rng("avgpool gaussian", hw, c)
    x = (r.standard_normal((n * hw, c)) + 0.25).astype(np.float16)
    x64 = x.astype(np.float64).reshape(n, hw, c)
    mean, mabs = x64.mean(axis=1), np.abs(x64).mean(axis=1)
    bound = hw * 2.0 ** -24 * mabs + 2.0 ** -11 * np.abs(mean) + 2.0 ** -25
    a = avgpool_call(Arena(CAPACITY, 0xFF), x, n, hw, (0, 0), c)
    b = avgpool_call(Arena(CAPACITY, 0x55), x, n, hw, (0, 0), c)
    assert np.array_equal(a.view(np.int16), b.view(np.int16)), "two calls differ"
    err = np.abs(a.astype(np.float64) - mean)
    print(f"avgpool gaussian hw {hw} c {c}: max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------- camera gate
def branch_words(mid):
    return mid * (3 * mid + 31)


def gate64(v, packed, mid, dtype=np.float64):
    """The documented statement on the packed block, evaluated in `dtype` with numpy's own summation:
    -> (pre-sigmoid values [2, n, mid], gates)."""
    v = v.astype(dtype)
    pre = []
    for br in (0, 1):
        q = packed[br * branch_words(mid):(br + 1) * branch_words(mid)].astype(dtype)
        at = 0
        h = v
        for li, kdim in enumerate((27, mid, mid, mid)):
            w, b = q[at:at + kdim * mid].reshape(kdim, mid), q[at + kdim * mid:at + kdim * mid + mid]
            at += kdim * mid + mid
            h = h @ w + b
            if li in (0, 2):
                h = np.maximum(h, 0)
        assert at == branch_words(mid)
        pre.append(h)
    pre = np.stack(pre)
    with np.errstate(over="ignore"):
        return pre, (1 / (1 + np.exp(-pre))).astype(dtype)


def gate_call(arena, v, in_pitch, packed, mid):
    L, h, st = _lib()
    n = v.shape[0]
    rows = np.full((n, in_pitch), 12345.0, np.float32)
    rows[:, :27] = v
    vd = arena.place(torch.from_numpy(rows.reshape(-1)[:(n - 1) * in_pitch + 27].copy()), 4, "mlp_input")
    pd = arena.place(torch.from_numpy(np.array(packed)), 4, "packed")
    assert L.load_library().bevops_lss_camera_gate_packed_size(mid) == packed.nbytes
    gd = arena.empty((2, n, mid), torch.float32, 4, "gates")
    rc = h.bevops_lss_camera_gate(vd.data_ptr(), in_pitch, pd.data_ptr(), gd.data_ptr(), n, mid, st)
    assert rc == L.SUCCESS
    arena.check()
    return gd.cpu().numpy()


def gate_both(v, in_pitch, packed, mid):
    got = [gate_call(Arena(CAPACITY, p), v, in_pitch, packed, mid) for p in POISONS]
    assert np.array_equal(got[0].view(np.int32), got[1].view(np.int32))
    return got[0]


def sparse_signs(r, kdim, mid, nnz, scale):
    """[kdim, mid] with nnz entries of +-scale per output column."""
    w = np.zeros((kdim, mid))
    for j in range(mid):
        w[r.choice(kdim, size=min(nnz, kdim), replace=False), j] = r.choice([-1.0, 1.0], size=min(nnz, kdim)) * scale
    return w


@functools.lru_cache(maxsize=None)
def dyadic_block(mid):
    """Parameters on which every dot product is exact in fp32 in ANY order: three +-1 entries per output and layer
    (the last layer +-2^-11, so that the gate's argument spreads over about +-20), biases half-integers: the values of
    layer l are half-integers (multiples of 2^-12 behind the last layer) below 2600 * 3^l + ..., whose sums of
    magnitudes stay below 2^24 units.  gate64 in float64 is then the exact argument."""
    r = X._rng("camera gate dyadic", mid)
    parts = []
    for _ in (0, 1):
        for li, kdim in enumerate((27, mid, mid, mid)):
            parts.append(sparse_signs(r, kdim, mid, 3, 2.0 ** -11 if li == 3 else 1.0).reshape(-1))
            parts.append(r.integers(-64, 65, size=mid) * (2.0 ** -12 if li == 3 else 0.5))
    packed = np.concatenate(parts).astype(np.float32)
    assert packed.size == 2 * branch_words(mid)
    packed.setflags(write=False)
    return packed


def dyadic_inputs(r, n):
    v = r.integers(-5200, 5201, size=(n, 27)) * 0.5
    v[:, 0] = 1266.5
    return v.astype(np.float32)


def sigmoid_bound(g64):
    """tests/test_conv_slice_gpu.py's bound for the fp32 evaluation of 1 / (1 + exp(-s)) with the hardware exponential
    and reciprocal on an exact argument: under 128 * 2^-24 = 2^-17 relative; plus half an fp32 subnormal step."""
    return 2.0 ** -17 * np.abs(g64) + 2.0 ** -150


@pytest.mark.parametrize("mid", [32, 96, 256])
@pytest.mark.parametrize("n", [1, 6, 7])
def test_camera_gate_on_dyadic_parameters(n, mid):
    packed = dyadic_block(mid)
    v = dyadic_inputs(X._rng("camera gate dyadic in", n, mid), n)
    # exactness of every layer in fp32, in any order: the sums of magnitudes, in units of the layer's step
    mag = np.abs(v.astype(np.float64))
    for br in (0, 1):
        q = np.abs(packed[br * branch_words(mid):(br + 1) * branch_words(mid)].astype(np.float64))
        at, h = 0, mag
        for li, kdim in enumerate((27, mid, mid, mid)):
            h = h @ q[at:at + kdim * mid].reshape(kdim, mid) + q[at + kdim * mid:at + kdim * mid + mid]
            at += kdim * mid + mid
            assert h.max() / (2.0 ** -12 if li == 3 else 0.5) < 2.0 ** 24
    pre, want = gate64(v, packed, mid)
    X.f32_exact(pre, "the gate's argument")
    assert np.abs(pre).max() > 8 and (np.abs(pre) < 4).mean() > 0.1
    got = gate_both(v, 27 if n != 6 else 51, packed, mid).astype(np.float64)
    err, bound = np.abs(got - want), sigmoid_bound(want)
    print(f"camera gate dyadic n {n} mid {mid}: max err / bound {np.max(err / bound):.4f}")
    assert np.all(err <= bound), f"{int((err > bound).sum())} gates beyond the bound, worst {np.max(err / bound):.3f}"


@functools.lru_cache(maxsize=None)
def gaussian_block(mid):
    r = X._rng("camera gate gaussian", mid)
    parts = []
    for _ in (0, 1):
        for li, kdim in enumerate((27, mid, mid, mid)):
            scale = np.full(kdim, 1.0 / np.sqrt(kdim))
            if li == 0:
                scale = scale / gaussian_spread()            # fc1 with the BatchNorm folded in: 1 / std per input
            parts.append((r.standard_normal((kdim, mid)) * scale[:, None]).reshape(-1))
            parts.append(r.standard_normal(mid) * 0.5)
    packed = np.concatenate(parts).astype(np.float32)
    packed.setflags(write=False)
    return packed


def gaussian_spread():
    """The size of the 27 inputs: intrinsics (focal lengths and principal points around 1000), post-augmentation and
    extrinsic entries of order 1, a few translations of order 100."""
    s = np.ones(27)
    s[:4] = 1000.0
    s[12:15] = 100.0
    return s


def gaussian_inputs(r, n):
    return (r.standard_normal((n, 27)) * gaussian_spread() * 0.2 + gaussian_spread()).astype(np.float32)


@pytest.mark.parametrize("mid", [32, 96, 256])
@pytest.mark.parametrize("n", [1, 6, 7])
def test_camera_gate_on_gaussian_parameters(n, mid):
    """The yardstick is the error of torch's fp32 CPU statement against float64 ON THE SAME OPERANDS (the packed block):
    the kernel may be at most 4 x that maximum -- its summation order (one ascending fma chain) differs."""
    packed = gaussian_block(mid)
    v = gaussian_inputs(X._rng("camera gate gaussian in", n, mid), n)
    _, want = gate64(v, packed, mid)
    pt = torch.from_numpy(packed.copy())
    ref = []
    for br in (0, 1):
        q, at, h = pt[br * branch_words(mid):(br + 1) * branch_words(mid)], 0, torch.from_numpy(v)
        for li, kdim in enumerate((27, mid, mid, mid)):
            h = torch.nn.functional.linear(h, q[at:at + kdim * mid].reshape(kdim, mid).t().contiguous(),
                                           q[at + kdim * mid:at + kdim * mid + mid])
            at += kdim * mid + mid
            if li in (0, 2):
                h = torch.relu(h)
        ref.append(torch.sigmoid(h))
    ref = torch.stack(ref).numpy()
    yard = np.abs(ref.astype(np.float64) - want).max()
    got = gate_both(v, 27, packed, mid)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"camera gate gaussian n {n} mid {mid}: kernel max err {err:.3e}, torch fp32 CPU max err {yard:.3e}, "
          f"ratio {err / yard:.2f}")
    assert want.std() > 0.05
    assert err <= 4.0 * yard


def test_camera_gate_sees_a_focal_length_change_below_the_binary16_step():
    """1266.4 and 1266.0 are both 1266 in binary16; in fp32 they give different gates, each right."""
    mid, n = 96, 2
    packed = gaussian_block(mid)
    v = gaussian_inputs(X._rng("camera gate focal"), n)
    v[1] = v[0]
    v[0, 0], v[1, 0] = 1266.4, 1266.0
    assert np.float16(v[0, 0]) == np.float16(v[1, 0])
    got = gate_both(v, 27, packed, mid)
    _, want = gate64(v, packed, mid)
    assert not np.array_equal(got[:, 0], got[:, 1])
    moved = np.abs(want[:, 0] - want[:, 1])
    big = moved > 64 * 2.0 ** -24                               # gates the change moves by more than the fp32 error
    assert big.mean() > 0.5
    assert np.all(np.sign(got[:, 0] - got[:, 1])[big] == np.sign(want[:, 0] - want[:, 1])[big])


# ---------------------------------------------------------------------------------------------- the Python side
def test_wrappers_equal_the_c_calls():
    import types

    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions import yolox_ops as Y
    n, H, W, c = 2, 5, 7, 72
    r = X._rng("lss_depthnet wrappers")
    x = r.standard_normal((n * H * W, c)).astype(np.float16)
    gates = r.random((2, n, c)).astype(np.float32)
    wa, wb = se_gate2_call(Arena(CAPACITY, 0x55), x, gates, n, H * W, (0, 0), (0, 0), (0, 0))
    xt = Y.nhwc_empty(n, c, H, W, "cuda")
    xt.copy_(torch.from_numpy(x).cuda().view(n, H, W, c).permute(0, 3, 1, 2))
    buf = Y.nhwc_empty(n, c + 40, H, W, "cuda")
    buf.fill_(float("nan"))
    a, b = bev.se_gate2_nhwc(xt, torch.from_numpy(gates).cuda(), out_a=buf[:, 16:16 + c])
    assert a.data_ptr() == buf[:, 16:16 + c].data_ptr()
    assert np.array_equal(a.permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy().view(np.int16), wa)
    assert np.array_equal(b.permute(0, 2, 3, 1).reshape(-1, c).cpu().numpy().view(np.int16), wb)
    assert torch.isnan(buf[:, :16]).all() and torch.isnan(buf[:, 16 + c:]).all()
    pooled = bev.global_avgpool_nhwc(xt)
    want = avgpool_call(Arena(CAPACITY, 0x55), x, n, H * W, (0, 0), c)
    assert np.array_equal(pooled.cpu().numpy().view(np.int16), want.view(np.int16))
    assert torch.equal(pooled, bev.global_avgpool_nhwc(xt))
    # the gate through pack_camera_gate's cache; never packed under capture
    mid = 32
    g = torch.Generator().manual_seed(3)

    def lin(o, i):
        m = torch.nn.Linear(i, o)
        m.weight.data = torch.randn((o, i), generator=g) / i ** 0.5
        return m.cuda()

    bn = torch.nn.BatchNorm1d(27)
    bn.running_mean.data = torch.randn((27,), generator=g)
    bn.running_var.data = torch.rand((27,), generator=g) + 0.5
    bn = bn.cuda().eval()
    mods = [types.SimpleNamespace(fc1=lin(mid, 27), fc2=lin(mid, mid)) for _ in range(2)]
    ses = [types.SimpleNamespace(conv_reduce=lin(mid, mid), conv_expand=lin(mid, mid)) for _ in range(2)]
    v = torch.randn((6, 27), generator=g).cuda()
    scratch = torch.zeros(8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1.0)
        with pytest.raises(RuntimeError, match="capturing"):
            bev.camera_gate_packed(bn, mods[0], ses[0], mods[1], ses[1])
    del graph
    packed = bev.camera_gate_packed(bn, mods[0], ses[0], mods[1], ses[1])
    got = bev.lss_camera_gate(v, packed, mid)
    with torch.no_grad():
        h = bn(v)
        want = torch.stack([torch.sigmoid(s.conv_expand(torch.relu(s.conv_reduce(m.fc2(torch.relu(m.fc1(h)))))))
                            for m, s in zip(mods, ses)])
    assert got.shape == (2, 6, mid) and torch.allclose(got, want, atol=1e-5, rtol=0)
