"""GPU parity of inverse (csrc/inverse.hip): the reference's own outputs (tests/golden/inverse.npz), the reference test's
identities, random well-conditioned batches against fp64, permutations, a singular matrix inside a batch, leading
dimensions, graph capture and determinism, the domain."""
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu


def _well_conditioned(count, n, seed, cond=100.0):
    """U diag(s) V^T with singular values from 1 to cond: the inverse's entries are at most 1, so the absolute bars
    below act as relative ones (with singular values from 1 / cond to 1 the inverse's entries reach 100, and the fp32
    rounding of those entries alone is 1.3e-5 on average)."""
    g = torch.Generator().manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(count, n, n, generator=g, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(count, n, n, generator=g, dtype=torch.float64))
    s = torch.logspace(0, torch.log10(torch.tensor(cond)).item(), n, dtype=torch.float64)
    return (u * s) @ v.transpose(1, 2)


def test_inverse_matches_reference_fixtures():
    import bevformer_tensorrt_amd as bev
    g = golden("inverse")
    for name in [k[2:] for k in g if k.startswith("a_")]:
        got = bev.inverse(torch.from_numpy(g["a_" + name]).cuda())
        want = torch.from_numpy(g["x_" + name]).cuda()
        err = (got - want).abs()
        assert err.mean().item() <= 1e-5 and err.max().item() <= 1e-4 * max(1.0, want.abs().max().item()), name


def test_inverse_reference_test_input_is_identity():
    import bevformer_tensorrt_amd as bev
    x = torch.eye(32, device="cuda").repeat(8, 256, 1, 1)            # test_inverse.py:5-21
    out = bev.inverse(x)
    assert out.shape == x.shape and out.dtype == torch.float32
    assert torch.equal(out, x)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 31, 32])
def test_inverse_well_conditioned_against_fp64(n):
    import bevformer_tensorrt_amd as bev
    a64 = _well_conditioned(200, n, seed=n)
    a = a64.float().cuda()
    got = bev.inverse(a)
    want = torch.linalg.inv(a.double())
    assert (got.double() - want).abs().mean().item() <= 1e-5
    resid = (a.double() @ got.double() - torch.eye(n, device="cuda", dtype=torch.float64)).abs().max().item()
    assert resid <= 1e-4, resid
    assert torch.equal(bev.inverse(a), got)                          # deterministic


@pytest.mark.parametrize("n", [2, 5, 32])
def test_inverse_of_permutations_is_the_transpose(n):
    import bevformer_tensorrt_amd as bev
    g = torch.Generator().manual_seed(n)
    p = torch.stack([torch.eye(n)[torch.randperm(n, generator=g)] for _ in range(16)]).cuda()
    assert torch.equal(bev.inverse(p), p.transpose(1, 2))


def test_singular_matrix_is_nan_and_neighbours_are_unaffected():
    import bevformer_tensorrt_amd as bev
    a = _well_conditioned(6, 5, seed=11).float().cuda()
    a[2, :, 3] = 0                                                   # exactly singular: column 3 is zero
    got = bev.inverse(a)
    assert torch.isnan(got[2]).all()
    keep = [0, 1, 3, 4, 5]
    assert torch.isfinite(got[keep]).all()
    assert torch.equal(got[keep], bev.inverse(a[keep]))


def test_inverse_leading_dimensions():
    import bevformer_tensorrt_amd as bev
    a = _well_conditioned(30, 4, seed=5).float().cuda().view(2, 3, 5, 4, 4)
    got = bev.inverse(a)
    assert got.shape == (2, 3, 5, 4, 4)
    assert torch.equal(got.view(30, 4, 4), bev.inverse(a.view(30, 4, 4)))
    assert bev.inverse(a[:, :, :0]).shape == (2, 3, 0, 4, 4)


def test_inverse_graph_capture():
    import bevformer_tensorrt_amd as bev
    a = _well_conditioned(64, 3, seed=3).float().cuda()
    eager = bev.inverse(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bev.inverse(a)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = bev.inverse(a)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_inverse_domain():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    for x in (torch.eye(33, device="cuda")[None], torch.eye(3, device="cuda", dtype=torch.float16)[None]):
        with pytest.raises(L.BevopsError) as e:
            bev.inverse(x)
        assert e.value.status == L.NOT_SUPPORTED
    with pytest.raises(ValueError):
        bev.inverse(torch.zeros(2, 3, 4, device="cuda"))
