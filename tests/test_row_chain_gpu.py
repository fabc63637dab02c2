"""bevops_row_chain_f16 (csrc/row_chain.hip): a chain of dense stages over the same rows as one launch.

Reference: a float64 evaluation of the same stages that rounds to fp16 where the chain does (each stage's output, after
bias, identity, norm and activation).  Bound: the error of the per-layer route (one few-row GEMM per stage, the
one-pass LayerNorm behind it) against that same reference on the same inputs, times 1.5 -- measured in the same test
and printed.  Every row count of the issue is covered through row independence: the call on the first m rows must give
the bits of the 900-row call, which is the one held against the reference."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 15, 16, 17, 33)


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.float16).to(DEV)


def _stage(gen, K, N, groups=1, bias=True, norm=False, **kw):
    lead = (groups,) if groups > 1 else ()
    st = {"weight": _rand(gen, *lead, N, K, scale=K ** -0.5), "bias": _rand(gen, *lead, N, scale=0.5) if bias else None}
    if norm:
        st["norm"] = ((1 + _rand(gen, *lead, N, scale=0.2)).contiguous(), _rand(gen, *lead, N, scale=0.2), 1e-5)
    st.update(kw)
    return st


def _chains(gen, M):
    """name -> (x, stages, groups).  Between them: 1, 3 and 7 stages, K in {256, 512}, N in {10, 96, 256, 512, 768},
    bias / no bias, identity from a tensor / from an earlier stage, LayerNorm, ReLU, two destinations, unstored
    intermediates, a stage that reads an earlier stage's output, groups 2 and 6."""
    c = {}
    c["one"] = (_rand(gen, M, 256), [_stage(gen, 256, 96, res=_rand(gen, M, 96), relu=True, store=[64, 32])], 1)
    c["ffn"] = (_rand(gen, M, 256), [
        _stage(gen, 256, 256, res=_rand(gen, M, 256), norm=True, store=True),
        _stage(gen, 256, 512, relu=True),
        _stage(gen, 512, 256, bias=False, res_stage=1, norm=True, store=True)], 1)
    c["tail"] = (_rand(gen, M, 256), [
        _stage(gen, 256, 256, res=_rand(gen, M, 256), norm=True),
        _stage(gen, 256, 512, relu=True),
        _stage(gen, 512, 256, res_stage=1, norm=True, store=True),
        _stage(gen, 256, 256, relu=True),
        _stage(gen, 256, 256, relu=True),
        _stage(gen, 256, 10, store=True),
        _stage(gen, 256, 768, bias=False, input=2, res=_rand(gen, M, 768), store=True)], 1)
    for G in (2, 6):
        c[f"head{G}"] = (_rand(gen, G * M, 256), [
            _stage(gen, 256, 256, G, norm=True, relu=True),
            _stage(gen, 256, 256, G, norm=True, relu=True),
            _stage(gen, 256, 10, G, store=True)], G)
    return c


def _h(t):      # one rounding to fp16, kept in float64
    return t.to(torch.float16).double()


def _reference(x, stages, groups):
    """float64, rounded to fp16 at each stage's output -> the stored tensors in stage order"""
    M = x.shape[0] // groups
    outs = []
    vals = []
    for i, st in enumerate(stages):
        src = st.get("input", -1)
        src = i - 1 if src < 0 else src
        xin = x.double() if src < 0 else vals[src]
        ys = []
        for g in range(groups):
            pick = (lambda t: t[g]) if groups > 1 else (lambda t: t)
            rows = slice(g * M, (g + 1) * M)
            y = xin[rows] @ pick(st["weight"]).double().t()
            if st.get("bias") is not None:
                y = y + pick(st["bias"]).double()
            if st.get("res") is not None:
                y = y + st["res"][rows].double()
            elif st.get("res_stage", -1) >= 0:
                r = st["res_stage"]
                rs = stages[r].get("input", -1)
                rs = r - 1 if rs < 0 else rs
                y = y + (x.double() if rs < 0 else vals[rs])[rows]
            if st.get("norm") is not None:
                gamma, beta, eps = st["norm"]
                y = F.layer_norm(y, (y.shape[-1],), pick(gamma).double(), pick(beta).double(), eps)
            if st.get("relu"):
                y = y.clamp_min(0)
            ys.append(_h(y))
        vals.append(torch.cat(ys))
        store = st.get("store", False)
        if isinstance(store, list):
            outs += list(vals[-1].split(store, dim=1))
        elif store is not False:
            outs.append(vals[-1])
    return outs


def _per_layer(x, stages, groups):
    """the per-layer route: one few-row GEMM per stage (bias, identity, ReLU in its epilogue), the one-pass LayerNorm"""
    import bevformer_tensorrt_amd as bev
    M = x.shape[0] // groups
    outs, vals = [], []
    for i, st in enumerate(stages):
        src = st.get("input", -1)
        src = i - 1 if src < 0 else src
        xin = x if src < 0 else vals[src]
        ys = []
        for g in range(groups):
            pick = (lambda t: t[g]) if groups > 1 else (lambda t: t)
            rows = slice(g * M, (g + 1) * M)
            res = None
            if st.get("res") is not None:
                res = st["res"][rows]
            elif st.get("res_stage", -1) >= 0:
                r = st["res_stage"]
                rs = stages[r].get("input", -1)
                rs = r - 1 if rs < 0 else rs
                res = (x if rs < 0 else vals[rs])[rows]
            norm = st.get("norm")
            b = pick(st["bias"]) if st.get("bias") is not None else None
            y = bev.functions.small_gemm(xin[rows].contiguous(), pick(st["weight"]), b, None if res is None else res.contiguous(),
                                         bool(st.get("relu")) and norm is None)
            if norm is not None:
                y = bev.functions.layer_norm(y, pick(norm[0]), pick(norm[1]), norm[2])
                if st.get("relu"):
                    y = F.relu(y)
            ys.append(y)
        vals.append(torch.cat(ys))
        store = st.get("store", False)
        if isinstance(store, list):
            outs += list(vals[-1].split(store, dim=1))
        elif store is not False:
            outs.append(vals[-1])
    return outs


def _leading(x, stages, groups, m):
    """the same chain on the first m rows of every group"""
    M = x.shape[0] // groups
    rows = torch.cat([torch.arange(g * M, g * M + m) for g in range(groups)]).to(x.device)
    sub = [dict(st, res=st["res"][rows].contiguous()) if st.get("res") is not None else st for st in stages]
    return x[rows].contiguous(), sub, rows


@pytest.fixture(scope="module")
def cases():
    import bevformer_tensorrt_amd as bev
    gen = torch.Generator().manual_seed(7)
    out = {}
    for name, (x, stages, groups) in _chains(gen, 900).items():
        got = bev.functions.row_chain(x, stages, groups)
        out[name] = (x, stages, groups, got, _reference(x, stages, groups))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["one", "ffn", "tail", "head2", "head6"])
def test_chain_within_the_per_layer_routes_error(cases, name):
    x, stages, groups, got, want = cases[name]
    old = _per_layer(x, stages, groups)
    assert len(got) == len(want) == len(old)
    for i, (a, b, w) in enumerate(zip(got, old, want)):
        e_new, e_old = (a.double() - w).abs(), (b.double() - w).abs()
        print(f"{name}[{i}] {tuple(a.shape)}: chain max {e_new.max():.3e} mean {e_new.mean():.3e} | "
              f"per-layer max {e_old.max():.3e} mean {e_old.mean():.3e}")
        assert torch.isfinite(a).all()
        assert e_new.max() <= 1.5 * e_old.max() and e_new.mean() <= 1.5 * e_old.mean()


@pytest.mark.parametrize("name", ["one", "ffn", "tail", "head2", "head6"])
def test_rows_are_independent(cases, name):
    """M in {1, 15, 16, 17, 33}: the call on the leading rows gives the 900-row call's bits on those rows (rows 0 .. 16
    of M = 900 against M = 17 among them)"""
    import bevformer_tensorrt_amd as bev
    x, stages, groups, got, _ = cases[name]
    for m in ROWS:
        xs, sub, rows = _leading(x, stages, groups, m)
        small = bev.functions.row_chain(xs, sub, groups)
        for a, b in zip(small, got):
            assert torch.equal(a, b[rows]), (name, m)


@pytest.mark.parametrize("name", ["one", "tail", "head6"])
def test_packed_weights_give_the_row_major_bits(cases, name):
    """weights in the order the matrix instruction reads them (pack_chain_weight: the model's form) hold the same values
    in the same registers: bit-equal results, N = 10 and 96 (a last tile with zero rows) among them"""
    import bevformer_tensorrt_amd as bev
    x, stages, groups, got, _ = cases[name]
    packed = [dict(st, weight=bev.functions.pack_chain_weight(st["weight"]), packed=tuple(st["weight"].shape[-2:]))
              for st in stages]
    for a, b in zip(bev.functions.row_chain(x, packed, groups), got):
        assert torch.equal(a, b)


def _dyadic(gen, *shape, lim):
    return (torch.randint(-lim, lim + 1, shape, generator=gen).double() / 8).to(torch.float16).to(DEV)


@pytest.mark.parametrize("M", [1, 17, 33])
def test_exact_on_dyadic_operands(M):
    """values in (1/8)Z and K = 64: every partial sum is an fp32 number in any order, so the bits are predictable --
    a LayerNorm-free chain of two stages with identities and ReLU, and a LayerNorm whose row is +-1 (mean 0, variance
    1, eps 0)"""
    import bevformer_tensorrt_amd as bev
    gen = torch.Generator().manual_seed(3)
    x = _dyadic(gen, M, 64, lim=16)
    stages = [{"weight": _dyadic(gen, 64, 64, lim=8), "bias": _dyadic(gen, 64, lim=8), "relu": True, "store": True,
               "res": _dyadic(gen, M, 64, lim=16)},
              {"weight": _dyadic(gen, 32, 64, lim=8), "bias": None, "store": [24, 8]}]
    got = bev.functions.row_chain(x, stages)
    for a, w in zip(got, _reference(x, stages, 1)):
        assert torch.equal(a, w.to(torch.float16))
    sign = torch.tensor([1.0, -1.0]).repeat(16)
    ln = [{"weight": torch.diag(sign).to(torch.float16).to(DEV), "bias": None, "store": True,
           "norm": (_dyadic(gen, 32, lim=16), _dyadic(gen, 32, lim=16), 0.0)}]
    ones = torch.ones(M, 32, dtype=torch.float16, device=DEV)
    got = bev.functions.row_chain(ones, ln)[0]
    want = (sign.to(DEV).double() * ln[0]["norm"][0].double() + ln[0]["norm"][1].double()).to(torch.float16)
    assert torch.equal(got, want.expand(M, 32))


def test_outputs_stay_inside_their_ranges():
    """destinations inside poisoned guard bands (pitched rows, a 10-column one among them): nothing else changes"""
    import bevformer_tensorrt_amd as bev
    gen = torch.Generator().manual_seed(5)
    M = 33
    x, stages, _ = _chains(gen, M)["tail"]
    plain = bev.functions.row_chain(x, stages)
    bands, views = [], []
    guarded = []
    for st in stages:
        st = dict(st)
        if st.get("store") is True:
            N = st["weight"].shape[0]
            pitch = (N + 7) // 8 * 8 + 16
            band = torch.full((M + 2, pitch), 777.0, dtype=torch.float16, device=DEV)
            st["store"] = band[1:M + 1, 8:8 + N]
            bands.append(band)
            views.append((N, st["store"]))
        guarded.append(st)
    got = bev.functions.row_chain(x, guarded)
    torch.cuda.synchronize()
    assert len(got) == len(plain) == 3
    for a, b in zip(got, plain):
        assert torch.equal(a, b)
    for band, (N, view) in zip(bands, views):
        mask = torch.ones_like(band, dtype=torch.bool)
        mask[1:M + 1, 8:8 + N] = False
        assert (band[mask] == 777.0).all()


def test_rejections_queue_nothing():
    import bevformer_tensorrt_amd as bev
    from bevformer_tensorrt_amd.utils import lib as L
    gen = torch.Generator().manual_seed(9)
    M = 17
    out = torch.full((M, 64), 777.0, dtype=torch.float16, device=DEV)

    def st(K, N=64, **kw):
        return dict({"weight": _rand(gen, N, K), "bias": None, "store": out if N == 64 else False}, **kw)
    x48, x800, x256 = _rand(gen, M, 48), _rand(gen, M, 800), _rand(gen, M, 256)
    odd = _rand(gen, M * 256 + 4)[4:].view(M, 256)           # 8-byte aligned rows
    bad = [(x48, [st(48)]),                                    # K % 32
           (x800, [st(800)]),                                  # K > 768
           (x256, [st(256, 800, store=False), st(800)]),      # N > 768
           (x256, [st(256, 256, store=False)] * 8 + [st(256)]),   # nine stages
           (odd, [st(256)]),                                   # pointer alignment
           (x256, [st(256, res=_rand(gen, M, 66)[:, :64])])]  # identity pitch
    for x, stages in bad:
        with pytest.raises(L.BevopsError) as exc:
            bev.functions.row_chain(x, stages)
        assert exc.value.status == L.NOT_SUPPORTED
    torch.cuda.synchronize()
    assert (out == 777.0).all()


def test_captures_into_a_graph():
    import bevformer_tensorrt_amd as bev
    gen = torch.Generator().manual_seed(11)
    x, stages, groups = _chains(gen, 33)["head2"]
    eager = bev.functions.row_chain(x, stages, groups)[0].clone()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = bev.functions.row_chain(x, stages, groups)[0]
        for _ in range(2):
            out.fill_(0)
            graph.replay()
            stream.synchronize()
            assert torch.equal(out, eager)
