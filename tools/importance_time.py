#!/usr/bin/env python3
"""Attributions reduced over groups of rows (``gnan_attr_reduce``, csrc/attr_reduce.hip) on one MI355X against the composed route a
user had before it: ``attribution.shell_attributions`` (``gnan_attr_rows``) in as few row batches as ``ATTR_MAX_BYTES`` allows,
each followed by float64 torch reductions of the ``[rows, D, W]`` terms into the same ``M [G, 3, D + 1, W]``.

Cases
  a1 / a40   all rows of the arxiv-shaped twin (169,343 nodes, an R-MAT graph with arxiv's edge count; no data sets offline), K = 1
             hop-coded CSR, W = 129; one group, and 40 groups (a random class per node, the rows sorted by class)
  b          the same graph at W = 5,120 (F = 128, C = 40) on the first 16,384 rows: one composed batch
  c          all rows of a 417-node dense graph of the Mutagenicity shape (a random tree plus extra edges, W = 15)
  d          all rows of the bench's R-MAT graph (scale 24, 10M nodes, 100M edges, K = 1) at W = 64: eight composed batches

Protocol: both routes in this one process, alternately; HIP events around ``reps`` calls (``reps`` sized so that a window holds about
20 ms of work), 3 warm-ups, 15 samples (10 where one call takes more than 100 ms); median, min and max per call.  Both routes are
prepared outside the window (``prepare_reduced`` / ``prepare`` per batch): the window holds the launches and, for the composed route,
its torch reductions.  ``max_rel_diff``: the two results compared, relative to the largest entry.  One JSON line per case and
route; the fused line says whether its median lies below the composed median by more than the composed route's max - min."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnan_amd  # noqa: E402,F401
from gnan_amd import HopGraph, attribution  # noqa: E402
from gnan_amd import synthetic as syn  # noqa: E402
from gnan_amd.functional import column_sums  # noqa: E402

DEV = "cuda"
WARM, SAMPLES, WINDOW_MS = 3, 15, 20.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def composed_route(g, S, lut, use_cnt, rows, group_ptr, s_total):
    """-> a callable computing ``M`` from ``gnan_attr_rows`` batches and float64 torch reductions."""
    D, W = g.n_codes, S.shape[1]
    ids = torch.arange(g.n_rows, device=DEV, dtype=torch.int32) if rows is None else rows.to(torch.int32)
    R = ids.numel()
    gp = torch.tensor([0, R], device=DEV) if group_ptr is None else group_ptr.to(DEV)
    G = gp.numel() - 1
    who = torch.repeat_interleave(torch.arange(G, device=DEV), gp[1:] - gp[:-1])
    step = max(1, attribution.ATTR_MAX_BYTES // (D * W * 4))
    batches = [(attribution.prepare(g, S, lut, use_cnt, ids[r0:r0 + step], s_total), who[r0:r0 + step]) for r0 in range(0, R, step)]

    def run():
        M = torch.zeros((G, 3, D + 1, W), dtype=torch.float64, device=DEV)
        for launch, w in batches:
            a = launch.run().double()
            a = torch.cat([a, a.sum(dim=1, keepdim=True)], dim=1)
            if G == 1:
                M[0, 0] += a.sum(0)
                M[0, 1] += a.abs().sum(0)
                M[0, 2] += (a * a).sum(0)
            else:
                M[:, 0].index_add_(0, w, a)
                M[:, 1].index_add_(0, w, a.abs())
                M[:, 2].index_add_(0, w, a * a)
        return M
    return run, len(batches)


def measure(case, g, S, lut, use_cnt, rows, group_ptr, s_total):
    launch = attribution.prepare_reduced(g, S, lut, use_cnt, rows, group_ptr, s_total)
    info = attribution.describe_reduced(launch.calls[0])
    composed, n_batches = composed_route(g, S, lut, use_cnt, rows, group_ptr, s_total)
    routes = {"gnan_attr_reduce": launch.run, "attr_rows_then_torch_fp64": composed}
    ref = routes["attr_rows_then_torch_fp64"]()
    got = routes["gnan_attr_reduce"]()
    rel = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    del ref, got
    reps, samples = {}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        once = timed(fn, 1)
        reps[name] = max(1, min(1000, int(WINDOW_MS / max(once, 1e-3))))
        samples[name] = 10 if once > 100.0 else SAMPLES
    times = {k: [] for k in routes}
    for i in range(WARM + SAMPLES):
        for name, fn in routes.items():                               # alternately: both see the same neighbours on the machine
            if i < WARM + samples[name]:
                t = timed(fn, reps[name])
                if i >= WARM:
                    times[name].append(t)
    base = times["attr_rows_then_torch_fp64"]
    for name in routes:
        ts = times[name]
        line = {"what": "importance_time", "case": case, "route": name, "rows": int(launch.args.n_rows), "groups": int(launch.A.shape[0]),
                "pairs": int(launch.pairs), "W": int(S.shape[1]), "D": int(g.n_codes), "median_ms": statistics.median(ts),
                "min_ms": min(ts), "max_ms": max(ts), "reps_per_sample": reps[name], "samples": len(ts), "max_rel_diff": rel}
        if name == "gnan_attr_reduce":
            line.update(launches=sum(attribution.describe_reduced(c)["launches"] for c in launch.calls), calls=len(launch.calls),
                        blocks=info["n_blocks"], block_rows=info["block_rows"], lds_bytes=info["lds_bytes"],
                        partials_bytes=info["partials_bytes"], long_items_bytes=info["long_items_bytes"],
                        gather_bytes=int(launch.pairs) * S.shape[1] * 4 * info["shell_passes"],
                        below_composed_by_more_than_its_spread=statistics.median(ts) < statistics.median(base) - (max(base) - min(base)))
        else:
            line.update(batches=n_batches, terms_bytes=int(launch.args.n_rows) * g.n_codes * S.shape[1] * 4)
        print(json.dumps(line), flush=True)


def arxiv_graph():
    n, e = 169343, 1166243
    return syn.hop1_csr(*syn.rmat_edges(18, n, e, seed=1, device=DEV), n), n


def case_a():
    g, n = arxiv_graph()
    gen = torch.Generator(device=DEV).manual_seed(1)
    S = torch.randn((n, 129), generator=gen, device=DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    tot = column_sums(S)
    measure("a1: all rows, arxiv shape, K=1 CSR, W=129, one group", g, S, lut, True, None, None, tot)
    label = torch.randint(0, 40, (n,), generator=gen, device=DEV)
    order = torch.sort(label, stable=True).indices.to(torch.int32)
    gp = torch.zeros(41, dtype=torch.int64, device=DEV)
    torch.cumsum(torch.bincount(label, minlength=40), 0, out=gp[1:])
    measure("a40: all rows, arxiv shape, K=1 CSR, W=129, 40 groups", g, S, lut, True, order, gp, tot)


def case_b():
    g, n = arxiv_graph()
    gen = torch.Generator(device=DEV).manual_seed(2)
    S = torch.randn((n, 128 * 40), generator=gen, device=DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    rows = torch.arange(16384, device=DEV, dtype=torch.int32)
    measure("b: 16,384 rows, arxiv shape, K=1 CSR, W=5120, one group", g, S, lut, True, rows, None, column_sums(S))


def case_c():
    n, W = 417, 15
    gen = torch.Generator().manual_seed(2)
    tree = torch.stack([torch.arange(1, n), (torch.rand(n - 1, generator=gen) * torch.arange(1, n)).long()])
    extra = torch.randint(0, n, (2, n // 30 + 1), generator=gen)
    e = torch.cat([tree, extra], 1)
    ei = torch.stack([torch.cat([e[0], e[1]]), torch.cat([e[1], e[0]])])
    g = HopGraph.from_edge_index(ei.to(DEV), n)
    S = torch.randn((n, W), generator=gen).to(DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen).to(DEV)
    measure("c: all rows, 417-node dense graph, Mutagenicity shape, W=15", g, S, lut, True, None, None, None)


def case_d():
    n, e, W = 10_000_000, 100_000_000, 64
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = syn.hop1_csr(*syn.rmat_edges(24, n, e, seed=0, device=DEV), n)
    S = torch.randn((n, W), generator=gen, device=DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    measure("d: all rows, the bench's R-MAT graph, K=1 CSR, W=64", g, S, lut, True, None, None, column_sums(S))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("importance_time.py measures on the GPU: no device visible")
    which = sys.argv[1:] or ["a", "b", "c"]
    for name, fn in (("a", case_a), ("b", case_b), ("c", case_c), ("d", case_d)):
        if name in which:
            fn()
            torch.cuda.empty_cache()
