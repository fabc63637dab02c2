"""bevops_occ_head_f16 (csrc/occ_head.hip) through functions.occ_head_nhwc in the guarded arena of tests/util_arena.py,
against the float64 statement of tests/util_occ_head.py: exact bits on integer operands (Softplus is the identity above
20), column routing with one-hot rows, the derived bound on Gaussian operands (design/flashocc.md), containment, replay."""
import pytest
import torch

from util_arena import POISONS, Arena
from util_occ_head import EXACT_CASES, GENERAL_CASES, exact_operands, general_operands, statement

pytestmark = pytest.mark.gpu
F16 = torch.float16


def launch(poison, ops, Dz, Ncls, rows, logits=True, pitched=True):
    """One call in a fresh arena on the first `rows` rows.  pitched: y is channels 8 .. of a buffer 40 wider and a pixel's
    bytes lie Dz + 3 apart; else both are dense (Dz = 16: the 16-byte store).  -> (occ [rows, Dz], logits [rows, Dz Ncls]
    or None) on the host."""
    from bevformer_tensorrt_amd.functions.occ_head import occ_head_nhwc, pack_occ_head_tensors
    y, W1, b1, W2, b2 = ops
    C, (B, H, W) = y.shape[1], (1, 1, rows)
    A = Arena(8 << 20, poison)
    p = pack_occ_head_tensors(W1, b1, W2, b2, Dz, Ncls)
    p = p._replace(**{k: A.place(getattr(p, k), 16, k) for k in ("w1", "b1", "w2", "b2")})
    ybuf = A.empty((B, C + (40 if pitched else 0), H, W), F16, 16, "y", channels_last=True)
    ys = ybuf[:, 8:8 + C] if pitched else ybuf
    ys.copy_(y[:rows].t().reshape(C, B, H, W).permute(1, 0, 2, 3))
    obuf = A.empty((B, H, W, Dz + (3 if pitched else 0)), torch.uint8, 16 if not pitched else 1, "occ")
    before = obuf.clone()
    out = obuf[..., :Dz]
    lg = A.empty((B, H, W, Dz * Ncls), F16, 2, "logits") if logits else None
    occ_head_nhwc(ys, p, logits=lg if logits else False, out=out)
    A.check()
    assert torch.equal(obuf[..., Dz:], before[..., Dz:]), "bytes between two pixels were written"
    return out.reshape(rows, Dz).cpu().long(), (lg.reshape(rows, -1).cpu() if logits else None)


def both_poisons(*args, **kw):
    a, b = (launch(p, *args, **kw) for p in POISONS)
    assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)))
    return a


@pytest.mark.parametrize("logits,pitched", [(True, True), (False, False)])
@pytest.mark.parametrize("rows", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_chain_bits(case, rows, logits, pitched):
    ops, (occ, lg, _, _) = exact_operands(*case)
    got, got_lg = both_poisons(ops, *case[2:], rows, logits, pitched)
    assert torch.equal(got, occ[:rows]), f"{int((got != occ[:rows]).sum())} voxels differ"
    if logits:
        assert torch.equal(got_lg.double(), lg[:rows]), f"{int((got_lg.double() != lg[:rows]).sum())} logits differ"


@pytest.mark.parametrize("Dz,Ncls", [(16, 16), (3, 18), (11, 23), (15, 17), (1, 32)])
def test_one_hot_rows_route_every_column(Dz, Ncls):
    """C = Hd = 256, y = e_m, W1 = 32 I, b1 = 24 (h = 56 at unit m, 24 elsewhere), W2 = I, b2 = -100: row m's logits are
    -44 in column m and -76 everywhere else.  Voxel m // Ncls of row m answers m % Ncls, every other voxel ties and answers
    0; all logits are negative, so a padded column (logit 0) that took part would win; the last row is the last class of
    the last z."""
    N = Dz * Ncls
    y, W1, b1 = torch.eye(N, 256), 32.0 * torch.eye(256), torch.full((256,), 24.0)
    W2, b2 = torch.eye(N, 256), torch.full((N,), -100.0)
    ops = tuple(t.half() for t in (y, W1, b1, W2, b2))
    occ, lg, _, _ = statement(*ops, Dz, Ncls)
    m = torch.arange(N)
    want = torch.zeros(N, Dz, dtype=torch.long)
    want[m, m // Ncls] = m % Ncls
    assert torch.equal(occ, want) and float(lg.max()) == -44.0 and int(occ[N - 1, Dz - 1]) == Ncls - 1
    got, got_lg = both_poisons(ops, Dz, Ncls, N)
    assert torch.equal(got_lg.double(), lg) and torch.equal(got, want)


@pytest.mark.parametrize("rows", [129, 300])
@pytest.mark.parametrize("case", GENERAL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gaussian_operands_within_the_derived_bound(case, rows):
    ops, (occ, lg, _, _), eps, sure = general_operands(*case)
    got, got_lg = both_poisons(ops, *case[2:], rows)
    err = (got_lg.double() - lg[:rows]).abs()
    print(f"{case} rows {rows}: max |err| {float(err.max()):.3e}, max err / eps {float((err / eps[:rows]).max()):.3f}, "
          f"decided {float(sure[:rows].float().mean()):.3f}")
    assert bool((err <= eps[:rows]).all()), f"{int((err > eps[:rows]).sum())} logits beyond the bound"
    assert torch.equal(got[sure[:rows]], occ[:rows][sure[:rows]])


def test_a_nan_stays_in_its_row():
    case = GENERAL_CASES[0]
    ops = general_operands(*case)[0]
    clean = both_poisons(ops, *case[2:], 300)
    y = ops[0].clone()
    y[130, 5] = float("nan")
    got = both_poisons((y,) + ops[1:], *case[2:], 300)
    keep = torch.arange(300) != 130
    assert torch.isnan(got[1][130]).all()
    assert torch.equal(got[0][keep], clean[0][keep]) and torch.equal(got[1][keep].view(torch.int16), clean[1][keep].view(torch.int16))


def test_replay_equals_eager_and_never_packs_under_capture():
    import bevformer_tensorrt_amd as bev
    case = EXACT_CASES[2]
    (y, W1, b1, W2, b2), (occ, _, _, _) = exact_operands(*case)
    y, W1, b1, W2, b2 = (t.cuda() for t in (y, W1, b1, W2, b2))
    ys = y.t().reshape(1, case[0], 1, -1)
    p = bev.functions.pack_occ_head(W1, b1, W2, b2, *case[2:])
    assert bev.functions.pack_occ_head(W1, b1, W2, b2, *case[2:]) is p
    out = torch.empty((1, 1, 300, case[2]), dtype=torch.uint8, device="cuda")
    eager = bev.functions.occ_head_nhwc(ys, p, out=out).clone()
    assert torch.equal(eager.view(300, -1).cpu().long(), occ)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bev.functions.occ_head_nhwc(ys, bev.functions.pack_occ_head(W1, b1, W2, b2, *case[2:]), out=out)
    for _ in range(3):
        out.fill_(255)
        graph.replay()
        assert torch.equal(out, eager)
    W2.mul_(2.0)                                                     # a changed weight: never repacked in a capture
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        out.add_(1)
        with pytest.raises(RuntimeError, match="capturing"):
            bev.functions.pack_occ_head(W1, b1, W2, b2, *case[2:])
