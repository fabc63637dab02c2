#!/usr/bin/env python3
"""The row-chain sites of the BEVFormer decoder (bevformer._ROW_CHAIN, csrc/row_chain.hip) against the per-layer launches
they replace, under HIP-graph replay, old and new alternately, three rounds each (the protocol of
tools/merged_proj_time.py): one JSON line per site with every round's figure and the keep rule (worst new round < best
old round).  Both routes run the model's own code: one DecoderLayer behind its sampler, and the head's batched branch.
  dec.tail       900 rows: output_proj + norm, fc1, fc2 + norm, the regression branch, the next layer's in-projection
                 (7 launches -> 1)
  dec.tail_last  the same without a next layer (6 -> 1)
  head.cls       6 x 900 rows: Linear-LN-ReLU-Linear-LN-ReLU-Linear(10) with stacked parameters (the framework's batched
                 GEMMs, norms and element-wise launches -> 1)
`max_abs_diff` is the difference of the two routes' results (they round at different points: design/model.md)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bevformer_tensorrt_amd as bev  # noqa: E402
from bevformer_tensorrt_amd import bevformer as B  # noqa: E402
from merged_proj_time import graph_median_us  # noqa: E402


def sites(gen):
    dev, dtype, n = torch.device("cuda"), torch.float16, B.NUM_QUERY
    rnd = lambda *shape, s=1.0: (torch.randn(*shape, generator=gen) * s).to(dev, dtype)
    model = B.BEVFormer("tiny", seed=0).to(dev, dtype)
    layer, nxt, reg, ops = model.decoder[0], model.decoder[1], model.reg_branches[0], model.ops
    sampled, query_n, query_pos = rnd(n, B.EMBED, s=0.5), rnd(n, 1, B.EMBED), rnd(n, 1, B.EMBED)
    out, reg_out = torch.empty(n, B.EMBED, device=dev, dtype=dtype), torch.empty(n, 10, device=dev, dtype=dtype)
    term = nxt._qkv_term(ops, sampled, query_pos)
    fn = B._gemm_entry(ops)

    def tail_old(with_next):
        q = B._dense_norm(ops, layer.cross_attn.output_proj, sampled.view(n, 1, B.EMBED), query_n, layer.norms[1])
        o = layer.ffn(q, ops, norm=layer.norms[2])
        r = B._mlp(ops, reg, o)
        qkv = fn(o.view(n, B.EMBED), nxt.self_attn.in_proj_weight, None, term, False) if with_next else None
        return o.view(n, B.EMBED), r.view(n, 10), qkv

    def tail_new(with_next):
        return layer._tail(ops, sampled, query_n, query_pos, reg, nxt if with_next else None, out, reg_out)

    for name, with_next in (("dec.tail", True), ("dec.tail_last", False)):
        yield name, (lambda w=with_next: tail_old(w)), (lambda w=with_next: tail_new(w))
    hs = rnd(6, n, B.EMBED, s=0.5)

    def head(on):
        saved = B._ROW_CHAIN["enabled"]
        B._ROW_CHAIN["enabled"] = on
        try:
            return (model._cls_batched(hs),)
        finally:
            B._ROW_CHAIN["enabled"] = saved
    yield "head.cls", (lambda: head(False)), (lambda: head(True))


def main(rounds=3):
    from bevformer_tensorrt_amd.functions.dispatch import using
    with torch.no_grad(), using(own=True):      # (the own-kernel dispatch, as inside the model's frame)
        for name, old, new in sites(torch.Generator().manual_seed(0)):
            a, b = old(), new()
            diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, b) if x is not None)
            us = {"old": [], "new": []}
            for _ in range(rounds):
                us["old"].append(round(graph_median_us(old), 2))
                us["new"].append(round(graph_median_us(new), 2))
            print(json.dumps({"site": name, "us_old": us["old"], "us_new": us["new"], "max_abs_diff": diff,
                              "keep": max(us["new"]) < min(us["old"])}), flush=True)


if __name__ == "__main__":
    main()
