"""bevops_conv3d_slice_f16 (csrc/conv3d_slice.hip) through the C entry, every operand in the guarded arena of
tests/util_arena.py under the NaN poison; every byte of the output buffer outside the output slice is compared.

Lattice: x = integers in [-8, 8] / 2, w = integers in [-8, 8] / 4, bias and identity integers in [-64, 64] / 8.  A product
is a multiple of 2^-3 of at most 8 and K <= 27 * 96, so every partial sum is a multiple of 2^-3 below 2^15: under 2^24
units, exact in fp32 in any order.  The output must be the float64 result rounded once to fp16, bit for bit.

Gaussian operands: |out - ref| <= g S + 2^-11 (|ref| + g S) + 2^-25 with g = (27 Cin + 2) 2^-24 (one fp32 rounding per
product-accumulate of K = 27 Cin terms, bias and identity) and S = sum |x w| + |bias| + |res| per output, in float64:
accumulation error, one fp16 rounding of the perturbed value, half a subnormal step.  Derived, not measured."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util_arena import Arena

pytestmark = pytest.mark.gpu

LAST = {}      # what the last launch() call left: the output slice view and the entry's arguments (the replay test)


def conv64(x, w, stride):
    """float64 statement: x [B, Z, Y, X, Ci], w [Co, kz, ky, kx, Ci] -> [B, Zo, Yo, Xo, Co]."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).permute(0, 4, 1, 2, 3)
    return F.conv3d(t(x), t(w), None, stride, w.shape[1] // 2).permute(0, 2, 3, 4, 1).numpy()


def ref64(x, w, bias, res, stride, act):
    v = conv64(x, w, stride) + (0 if bias is None else np.float64(bias)) + (0 if res is None else np.float64(res))
    return np.where(v < 0, 0.0, v) if act else v


def bound64(ref, S, K):
    """The derived bound of the module's docstring for sums of K products; S = sum |x w| + |bias| + |res| per output."""
    g = (K + 2) * 2.0 ** -24
    return g * S + 2.0 ** -11 * (np.abs(ref) + g * S) + 2.0 ** -25


def launch(x, w, bias, res, stride, act, pitched=False):
    """One call on fp16 arrays; pitched: x_pitch = Cin + 8 and out the middle slice of a wider buffer.  -> out fp16 array."""
    from bevformer_tensorrt_amd.utils import lib as L
    arena = Arena(4 << 20, 0xFF)
    B, Z, Y, X, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    zo, yo, xo = ((n + 2 * (k // 2) - k) // stride + 1 for n in (Z, Y, X))
    xp, (op, oc0) = (Cin + 8, (Cout + 24, 8)) if pitched else (Cin, (Cout, 0))
    xb = arena.empty((B, Z, Y, X, xp), torch.float16, 16, "x")
    xb[..., :Cin].copy_(torch.from_numpy(x))
    dev = [None if a is None else arena.place(torch.from_numpy(a), 16, n) for a, n in ((w, "w"), (bias, "bias"), (res, "res"))]
    ob = arena.empty((B, zo, yo, xo, op), torch.float16, 16, "out")
    ov = ob[..., oc0:oc0 + Cout]
    args = (xb.data_ptr(), xp, dev[0].data_ptr(), None if bias is None else dev[1].data_ptr(),
            None if res is None else dev[2].data_ptr(), Cout, ov.data_ptr(), op, B, Z, Y, X, Cin, Cout, k, stride, act)
    assert L.load_library().bevops_conv3d_slice_f16(*args, L.current_stream_ptr(torch.device("cuda"))) == L.SUCCESS
    arena.check()
    whole = ob.cpu().numpy().view(np.uint16)
    outside = np.ones(whole.shape[-1], bool)
    outside[oc0:oc0 + Cout] = False
    assert (whole[..., outside] == 0xFFFF).all(), "bytes outside the output slice changed"
    LAST.update(arena=arena, ov=ov, args=args)
    return whole[..., oc0:oc0 + Cout].view(np.float16).copy()


def lattice(shape, cin, cout, k, stride, seed=0):
    r = np.random.default_rng(seed)
    B, Z, Y, X = shape
    x = (r.integers(-8, 9, (B, Z, Y, X, cin)) / 2).astype(np.float16)
    w = (r.integers(-8, 9, (cout, k, k, k, cin)) / 4).astype(np.float16)
    bias = (r.integers(-64, 65, cout) / 8).astype(np.float16)
    res = (r.integers(-64, 65, conv64(x, w, stride).shape) / 8).astype(np.float16)
    return x, w, bias, res


def same_bits(got, want64):
    want = want64.astype(np.float16)
    bad = got.view(np.uint16) != want.view(np.uint16)
    assert not bad.any(), f"{bad.sum()} of {bad.size} outputs differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64), (96, 72), (32, 136)])
@pytest.mark.parametrize("shape,stride", [((1, 3, 5, 7), 1), ((2, 4, 6, 9), 1), ((1, 1, 1, 1), 1), ((1, 1, 9, 17), 1),
                                          ((1, 5, 7, 9), 2), ((2, 4, 6, 8), 2)])
def test_lattice_exact(shape, stride, cin, cout, k, pitched):
    x, w, bias, res = lattice(shape, cin, cout, k, stride)
    same_bits(launch(x, w, bias, res, stride, 1, pitched), ref64(x, w, bias, res, stride, 1))
    same_bits(launch(x, w, None, None, stride, 0, pitched), ref64(x, w, None, None, stride, 0))


def test_identity_in_front_of_relu():
    x, w, bias, res = lattice((2, 4, 6, 9), 32, 32, 3, 1, seed=1)
    x, w, res = np.abs(x), -np.abs(w), np.abs(res) + np.float16(1)                 # conv <= 0, identity >= 1
    pre = conv64(x, w, 1) + np.float64(bias)
    assert (np.maximum(pre + res, 0) != np.maximum(pre, 0) + res).mean() > 0.5     # the premise: the order shows
    same_bits(launch(x, w, bias, res, 1, 1), ref64(x, w, bias, res, 1, 1))


@pytest.mark.parametrize("tap", range(27))
def test_one_hot_tap(tap):
    kz, ky, kx = tap // 9, tap // 3 % 3, tap % 3
    x = np.random.default_rng(2).integers(-1000, 1000, (1, 4, 5, 6, 32)).astype(np.float16)
    w = np.zeros((32, 3, 3, 3, 32), np.float16)
    w[:, kz, ky, kx, 5] = 1
    padded = np.pad(np.float64(x[..., 5]), ((0, 0), (1, 1), (1, 1), (1, 1)))
    want = padded[:, kz:kz + 4, ky:ky + 5, kx:kx + 6, None].repeat(32, -1)          # the input shifted by the tap, zeros outside
    same_bits(launch(x, w, None, None, 1, 0), want)


@pytest.mark.parametrize("stride", [1, 2])
def test_gaussian_bound(stride):
    r = np.random.default_rng(4)
    x = r.standard_normal((2, 4, 6, 9, 96)).astype(np.float16)
    w = (r.standard_normal((72, 3, 3, 3, 96)) / 16).astype(np.float16)
    bias = r.standard_normal(72).astype(np.float16)
    res = r.standard_normal(conv64(x, w, stride).shape).astype(np.float16)
    got = np.float64(launch(x, w, bias, res, stride, 1, pitched=True))
    ref = ref64(x, w, bias, res, stride, 1)
    S = conv64(np.abs(np.float64(x)), np.abs(np.float64(w)), stride) + np.abs(np.float64(bias)) + np.abs(np.float64(res))
    bound, err = bound64(ref, S, 27 * 96), np.abs(got - ref)
    print(f"stride {stride}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("stride,at", [(1, (1, 0, 5, 8, 17)), (2, (0, 3, 2, 5, 40)), (2, (1, 1, 3, 4, 0))])
def test_nan_containment(stride, at):
    """One NaN in x reaches exactly the outputs whose window holds it (and there every channel)."""
    x, w, bias, res = lattice((2, 4, 6, 9), 64, 40, 3, stride, seed=5)
    w[w == 0] = 1
    x[at] = np.nan
    got = launch(x, w, bias, res, stride, 1)
    want = np.zeros(got.shape[:4], bool)
    for m in np.ndindex(*got.shape[:4]):
        want[m] = m[0] == at[0] and all(abs(stride * m[i] - at[i]) <= 1 for i in (1, 2, 3))
    assert want.any() and (np.isnan(got) == want[..., None]).all()


def test_replay_and_repeat():
    x, w, bias, res = lattice((2, 4, 6, 9), 96, 72, 3, 1, seed=6)
    first = launch(x, w, bias, res, 1, 1, pitched=True)
    from bevformer_tensorrt_amd.utils import lib as L
    ov, args = LAST["ov"], LAST["args"]
    fn = L.load_library().bevops_conv3d_slice_f16
    ov.fill_(7)
    assert fn(*args, L.current_stream_ptr(torch.device("cuda"))) == L.SUCCESS
    assert torch.equal(ov.cpu().view(torch.int16), torch.from_numpy(first.view(np.int16)))     # two calls, the same bits
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert fn(*args, L.current_stream_ptr(torch.device("cuda"))) == L.SUCCESS
    for fill in (0, 3, -1):                                                         # several replays against the eager result
        ov.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ov.cpu().view(torch.int16), torch.from_numpy(first.view(np.int16)))
    LAST["arena"].check()
