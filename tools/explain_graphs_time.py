#!/usr/bin/env python3
"""Explaining a data set of small graphs on one MI355X: ``interpret.explain_graphs`` / ``importance_graphs`` (``gnan_attr_blocks``,
csrc/attr_blocks.hip) against the loop a user had to write before them — ``explain`` + ``explain_sources`` per graph.

Data: ``synthetic.mutagenicity_shaped_graphs(count)`` (the C2 shape: 4337 graphs of about 30 nodes, 15 feature columns) and a default
``models.TensorGNAN`` graph task.  Set-up outside every timed region: the graphs' hop codes (``attach_hop_graphs`` for the loop,
``GraphBatch.from_datas`` for the batch fronts), the module, one untimed pass of each route.

Routes, each a whole pass over the data set, timed wall-clock around a device synchronisation (the loop's cost IS its host work
and device reads), alternately, ``--warmup`` passes then ``--samples``; median, min, max and the spread (max - min) / median:
  loop          ``explain(m, d)`` and ``explain_sources(m, d)`` for every graph ``d``
  explain       ``explain_graphs(m, batch)`` over runs of graphs whose per-node result stays under ``ATTR_MAX_BYTES``
  importance    ``importance_graphs(m, batch, groups=labels)``
and ``run()`` alone (HIP events, windows of about 20 ms): ``gnan_attr_blocks`` on the whole data set, per graph, next to
``gnan_attr_cols`` on one 30-node graph.  One JSON line per route, then one with the ratios."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnan_amd  # noqa: E402,F401
from gnan_amd import attribution, interpret, models  # noqa: E402
from gnan_amd import synthetic as syn  # noqa: E402
from gnan_amd.graph import attach_hop_graphs  # noqa: E402

DEV = "cuda"


class Bag:
    pass


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stats(ts):
    med = statistics.median(ts)
    return {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "spread": (max(ts) - min(ts)) / med, "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=4337)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--samples", type=int, default=5)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("explain_graphs_time.py measures on the GPU: no device visible")
    datas, labels = [], []
    for ei, x, y in syn.mutagenicity_shaped_graphs(opt.graphs):
        d = Bag()
        d.x, d.edge_index = x.to(DEV), torch.from_numpy(ei).to(DEV)
        datas.append(d)
        labels.append(int(y > 0))
    F = datas[0].x.shape[1]
    torch.manual_seed(0)
    m = models.TensorGNAN(F, 1, 3, hidden_channels=16, is_graph_task=True).to(DEV).eval()
    attach_hop_graphs(datas)
    batch = interpret.GraphBatch.from_datas(datas)
    G, N, D = batch.n_graphs, batch.total_nodes, batch.n_codes
    # runs of graphs whose [n, D, W] per-node result stays under the byte budget
    W = F * (1 if m.readout_n_layers > 0 else m.out_channels)
    budget = attribution.ATTR_MAX_BYTES // (D * W * 4)
    runs, g0 = [], 0
    while g0 < G:
        g1, nodes = g0, 0
        while g1 < G and (g1 == g0 or nodes + batch.sizes[g1] <= budget):
            nodes += batch.sizes[g1]
            g1 += 1
        runs.append(batch if (g0, g1) == (0, G) else batch.graphs(g0, g1))
        g0 = g1

    def loop():
        for d in datas:
            interpret.explain(m, d)
            interpret.explain_sources(m, d)

    def explain():
        for r in runs:
            interpret.explain_graphs(m, r)

    def importance():
        interpret.importance_graphs(m, batch, groups=labels)

    routes = {"loop": loop, "explain": explain, "importance": importance}
    times = {k: [] for k in routes}
    for i in range(opt.warmup + opt.samples):
        for name, fn in routes.items():
            t = wall(fn)
            if i >= opt.warmup:
                times[name].append(t)
    head = {"what": "explain_graphs_time", "graphs": G, "nodes": N, "D": D, "W": W, "runs": len(runs)}
    res = {}
    for name in routes:
        res[name] = stats(times[name])
        print(json.dumps({**head, "route": name, **res[name], "ms_per_graph": res[name]["median_ms"] / G}), flush=True)

    # run() alone: the batch kernels on the first run of graphs, the one-graph kernels on one 30-node graph
    t = interpret._graph_terms(m, runs[0], "explain_graphs")
    launch = attribution.prepare_blocks(runs[0].blocks, t.fx, t.table, t.cnt)
    info = attribution.describe_blocks(launch.args)
    one = min(range(G), key=lambda g: abs(batch.sizes[g] - 30))
    t1 = interpret._terms(m, datas[one], "explain_sources")
    launch1 = attribution.prepare_sources(t1.g, t1.fx, t1.table, t1.use_cnt)
    for name, fn, per in (("run_blocks", launch.run, runs[0].n_graphs), ("run_cols_one_graph", launch1.run, 1)):
        reps = max(1, min(1000, int(20.0 / max(events(fn, 1), 1e-3))))
        ts = [events(fn, reps) for _ in range(5 + 30)][5:]
        res[name] = stats(ts)
        line = {**head, "route": name, **res[name], "graphs_per_call": per, "us_per_graph": 1e3 * res[name]["median_ms"] / per, "reps_per_sample": reps}
        if name == "run_blocks":
            line.update(launches=info["launches"], bin_passes=info["bin_passes"], lds_bytes=info["lds_bytes"], n_tiles=info["n_tiles"],
                        workspace_bytes=info["workspace_bytes"], pairs=launch.pairs)
        print(json.dumps(line), flush=True)
    print(json.dumps({**head, "loop_over_explain_graphs": res["loop"]["median_ms"] / res["explain"]["median_ms"],
                      "loop_over_importance_graphs": res["loop"]["median_ms"] / res["importance"]["median_ms"],
                      "loop_spread": res["loop"]["spread"],
                      "cols_one_graph_over_blocks_per_graph": res["run_cols_one_graph"]["median_ms"] * runs[0].n_graphs / res["run_blocks"]["median_ms"]}),
          flush=True)


if __name__ == "__main__":
    main()
