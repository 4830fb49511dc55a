"""Preprocessing of a Mutagenicity-shaped data set (4337 graphs), both ways, in one process:

  loop     one ``HopGraph.from_edge_index`` per graph, as bench.py's ``run_c2`` sets up (a dozen framework launches, a
           ``gnan_bfs_dense`` launch and a device read per graph);
  batched  one ``HopGraph.batch_from_edge_index`` over the whole set (four launches, one read of the results);
  attach   ``gnan_amd.attach_hop_graphs`` on per-graph objects (the batched builder plus the concatenation of their edges);

and a 32-graph training batch: ``HopBlocks.from_edge_index`` against 32 ``from_edge_index`` calls + ``HopBlocks.from_blocks``.

The edges are uploaded once, before anything is timed.  First every graph of the batched result is compared with the loop's, bit for
bit; then both methods are warmed up and timed ``--repeats`` times, ALTERNATING, by a host clock around work that ends in
``torch.cuda.synchronize()``.  Prints one JSON line with every repeat.  Needs the MI355X: there is no CPU fallback.

    python tools/preprocess_bench.py [--graphs 4337] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gnan_amd  # noqa: E402
from gnan_amd import HopGraph  # noqa: E402
from gnan_amd import synthetic as syn  # noqa: E402
from gnan_amd.batched import HopBlocks  # noqa: E402
from gnan_amd.graph import cat_edges  # noqa: E402


class Bag:
    pass


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4337)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_bench needs the GPU: a timing taken anywhere else says nothing about it")
    dev = torch.device("cuda", 0)
    edges, sizes, xs = [], [], []
    for ei, x, _ in syn.mutagenicity_shaped_graphs(args.graphs, seed=0):
        edges.append(torch.as_tensor(ei).to(dev))
        xs.append(x.to(dev))
        sizes.append(int(x.shape[0]))
    ei_all, batch_all = cat_edges(edges, sizes, dev)
    batch_all = batch_all.long()                                    # what a PyG Batch holds
    k = min(args.batch, len(sizes))
    ei_k, batch_k = cat_edges(edges[:k], sizes[:k], dev)
    batch_k = batch_k.long()
    torch.cuda.synchronize()

    def loop():
        return [HopGraph.from_edge_index(e, n) for e, n in zip(edges, sizes)]

    def batched():
        return HopGraph.batch_from_edge_index(ei_all, batch_all)

    def attach():
        datas = []
        for e, x in zip(edges, xs):
            d = Bag()
            d.x, d.edge_index = x, e
            datas.append(d)
        return gnan_amd.attach_hop_graphs(datas)

    def blocks_loop():
        hops = []
        for e, n in zip(edges[:k], sizes[:k]):
            code = HopGraph.from_edge_index(e, n).code
            hops.append(torch.where(code == 255, -1.0, code.float()))
        return HopBlocks.from_blocks(hops)

    def blocks_batched():
        return HopBlocks.from_edge_index(ei_k, batch_k)

    # bit-equality first (this also warms both methods up)
    want, got, att = loop(), batched(), attach()
    assert len(want) == len(got) == len(att) == len(sizes)
    for i, (a, b, c) in enumerate(zip(want, got, att)):
        for other in (b, c.gnan_graph):
            assert a.n_codes == other.n_codes and torch.equal(a.code, other.code) and torch.equal(a.cnt, other.cnt), i
    wb, gb = blocks_loop(), blocks_batched()
    assert wb.sizes == gb.sizes and wb.n_codes == gb.n_codes
    assert torch.equal(wb.code, gb.code) and torch.equal(wb.node_off, gb.node_off) and torch.equal(wb.code_off, gb.code_off)
    del want, got, att, wb, gb
    for fn in (loop, batched, attach, blocks_loop, blocks_batched):                    # one more warm round
        timed(fn)
    times = {"loop": [], "batched": [], "attach": [], "blocks_loop": [], "blocks_batched": []}
    for _ in range(args.repeats):
        for name, fn in (("loop", loop), ("batched", batched), ("attach", attach), ("blocks_loop", blocks_loop),
                         ("blocks_batched", blocks_batched)):
            times[name].append(timed(fn)[0])
    ms = {name: [round(1e3 * t, 3) for t in ts] for name, ts in times.items()}
    print(json.dumps({
        "tool": "preprocess_bench", "graphs": len(sizes), "nodes": sum(sizes), "pairs": sum(n * n for n in sizes),
        "max_nodes": max(sizes), "batch_graphs": k, "repeats": args.repeats, "bit_equal": True, "ms": ms,
        "slowest_batched_ms": max(ms["batched"]), "fastest_loop_ms": min(ms["loop"]),
        "batched_beats_loop": max(ms["batched"]) < min(ms["loop"]),
        "slowest_blocks_batched_ms": max(ms["blocks_batched"]), "fastest_blocks_loop_ms": min(ms["blocks_loop"]),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
