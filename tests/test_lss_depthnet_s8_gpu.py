"""bevops_se_gate2_nhwc_s8 and bevops_global_avgpool_nhwc_s8 (csrc/lss_depthnet_s8.hip) through the C ABI in the guarded
arena of tests/util_arena.py under both poisons, every byte of the output buffers outside the output slices compared.

Both launches are BIT-EQUAL to the numpy float32 / integer statements of tests/util_lss_depthnet_s8.py at general (not
power-of-two) scales: their operation orders hold no addition, so there is nothing to contract.  Shapes: n hw in
{1, 35, 1408} x c in {16, 80, 256} (the pool: hw in {1, 35, 704}), dense and as slices of wider buffers; hand-made ties,
saturation, NaN and infinities; the Python wrappers eagerly and from a captured graph."""
import numpy as np
import pytest
import torch

import util_lss_depthnet_s8 as U
from util_arena import POISONS, Arena

pytestmark = pytest.mark.gpu

CAPACITY = 8 << 20
S_X, S_A, S_B = 0.0371, 0.0123, 0.0291


def _case(n, hw, c, seed):
    r = np.random.default_rng([n, hw, c, seed])
    x = r.integers(-127, 128, (n, hw, c)).astype(np.int8)
    x.reshape(-1)[:2] = [-128, 127]
    gates = (1.0 / (1.0 + np.exp(-r.normal(0, 2, (2, n, c))))).astype(np.float32)       # sigmoid outputs
    return x, gates


@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("c", [16, 80, 256])
@pytest.mark.parametrize("n,hw", [(1, 1), (5, 7), (2, 704)], ids=["1", "35", "1408"])
def test_gate_bits(n, hw, c, pitched):
    x, gates = _case(n, hw, c, 1)
    want_a, want_b = U.gate_statement(x, S_X, gates[0], S_A), U.gate_statement(x, S_X, gates[1], S_B)
    got = [U.gate_call(Arena(CAPACITY, poison), x, S_X, gates, S_A, S_B, pitched) for poison in POISONS]
    for a, b in got:
        assert np.array_equal(a, want_a) and np.array_equal(b, want_b)
    if n * hw * c >= 35 * 80:
        assert (want_a == 127).any() and (want_a == -127).any() and not np.array_equal(want_a, want_b)


@pytest.mark.parametrize("pitched", [False, True], ids=["dense", "slices"])
@pytest.mark.parametrize("c", [16, 80, 256])
@pytest.mark.parametrize("n,hw", [(3, 1), (2, 35), (2, 704)], ids=["1", "35", "704"])
def test_pool_bits(n, hw, c, pitched):
    x, _ = _case(n, hw, c, 2)
    x[0, :, 0], x[n - 1, :, c - 1] = 127, -127                       # the largest sums of either sign
    want = U.pool_statement(x, S_X)
    got = [U.pool_call(Arena(CAPACITY, poison), x, S_X, pitched) for poison in POISONS]
    for g in got:
        assert np.array_equal(g.view(np.int16), want.view(np.int16))
    assert want.any()


def test_hand_made_ties_saturation_and_non_finite_gates():
    x, sx, g, sa, sb, want_a, want_b = U.handmade_gate_case()
    for poison in POISONS:
        a, b = U.gate_call(Arena(CAPACITY, poison), x, sx, g, sa, sb, True)
        assert np.array_equal(a, want_a) and np.array_equal(b, want_b)
    xp, sp, want = U.handmade_pool_case()
    for poison in POISONS:
        got = U.pool_call(Arena(CAPACITY, poison), xp, sp, True)
        assert np.array_equal(got.view(np.int16), want.view(np.int16))
    over = U.pool_call(Arena(CAPACITY, POISONS[0]), xp, 1024.0, False)
    assert np.isposinf(over[0, 4]) and np.isneginf(over[0, 5])


def test_wrappers_eager_and_replayed():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.functions.yolox_ops import nhwc_empty
    n, H, W, c = 2, 5, 7, 80
    x, gates = _case(n, H * W, c, 3)
    dev = torch.device("cuda")
    buf = nhwc_empty(n, 2 * c + 16, H, W, dev, torch.int8)
    buf.zero_()
    xd = buf[:, 16:16 + c]
    xd.copy_(torch.from_numpy(x.reshape(n, H, W, c)).to(dev).permute(0, 3, 1, 2))
    gd = torch.from_numpy(gates).to(dev)
    want_a, want_b = U.gate_statement(x, S_X, gates[0], S_A), U.gate_statement(x, S_X, gates[1], S_B)
    want_p = U.pool_statement(x, S_X)

    def host(t):
        return t.permute(0, 2, 3, 1).reshape(n, H * W, c).cpu().numpy()

    a, b = bev.se_gate2_nhwc_q(xd, S_X, gd, S_A, S_B)
    pooled = bev.global_avgpool_nhwc_q(xd, S_X)
    assert a.dtype == torch.int8 and pooled.dtype == torch.float16 and tuple(pooled.shape) == (n, c)
    assert np.array_equal(host(a), want_a) and np.array_equal(host(b), want_b)
    assert np.array_equal(pooled.cpu().numpy().view(np.int16), want_p.view(np.int16))
    oa, ob, op = torch.zeros_like(a), torch.zeros_like(b), torch.zeros((n, c + 8), dtype=torch.float16, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            bev.se_gate2_nhwc_q(xd, S_X, gd, S_A, S_B, out_a=oa, out_b=ob)
            bev.global_avgpool_nhwc_q(xd, S_X, out=op)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        oa.zero_(), ob.zero_(), op.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(oa), want_a) and np.array_equal(host(ob), want_b)
        assert np.array_equal(op[:, :c].cpu().numpy().view(np.int16), want_p.view(np.int16)) and not op[:, c:].any()
