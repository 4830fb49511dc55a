#!/usr/bin/env python3
"""Attributions by source node (``gnan_attr_cols``, csrc/attr_cols.hip) on one MI355X against the only alternative a user had
before it: a device restatement with stock torch ops — an ``index_add_`` of the pairs' weights over (source, shell), the rest
bucket from the weights' total, the product with the operand rows.  That route adds with float atomics: it is not reproducible
from run to run, the kernel route is.

Cases
  a1 / a129    every row and every source of the arxiv shape's twin (169,343 nodes, an R-MAT graph with arxiv's edge count, K = 1
               hop-coded CSR: D = 3) at W = 1 and W = 129
  m            every row and every source of a 30-node dense graph of the Mutagenicity shape (a random tree plus extra edges, W = 15)

Protocol: both routes in this one process, alternately; HIP events around ``reps`` calls (``reps`` sized so that a window holds
about 20 ms of work), 5 warm-ups, 30 samples; median, min and max per call.  The kernel route is ``attribution.SourceLaunch.run``
— the launches, nothing else (the transposed graph and the chunk list are the prepared call's, as the pair -> row expansion is
the torch route's: both are built outside the window).  ``walk_GBps``: pairs x (5 index bytes + 4 of the count gather) plus the
``P * D * W * 4`` result bytes, over the median.  The two results are compared (``max_rel_diff``, relative to the largest entry).
One JSON line per case and route, and one with the ratio and both routes' spread."""
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

DEV = "cuda"
WARM, SAMPLES, WINDOW_MS = 5, 30, 20.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_route(g, S, lut, use_cnt, rest_from_total):
    """-> a callable computing ``B [n_cols, D, W]`` for every row and every source with stock torch ops on the device."""
    D, W, Cw = g.n_codes, S.shape[1], lut.shape[-1]
    if g.is_dense:
        row_of = torch.arange(g.n_rows, device=DEV).repeat_interleave(g.n_cols)
        col = torch.arange(g.n_cols, device=DEV).repeat(g.n_rows)
        code = g.code.long().reshape(-1)
    else:
        rp = g.rowptr.long()
        row_of = torch.repeat_interleave(torch.arange(g.n_rows, device=DEV), rp[1:] - rp[:-1])
        col, code = g.col.long(), g.code.long()
    if rest_from_total:
        keep = code < D - 1
        row_of, col, code = row_of[keep], col[keep], code[keep]
    shell = code.clamp(max=D - 1)
    slot = col * D + shell

    def run(dtype=torch.float32):
        table, rows = lut.to(dtype), S.to(dtype)
        w = table[shell]                                                      # [pairs, Cw]
        w_rest = table[D - 1].unsqueeze(0).expand(g.n_rows, Cw)
        if use_cnt:
            cnt = g.cnt.clamp_min(1).to(dtype)
            w = w / cnt[row_of, shell].unsqueeze(-1)
            w_rest = w_rest / cnt[:, D - 1].unsqueeze(-1)
        V = torch.zeros((g.n_cols * D, Cw), dtype=dtype, device=DEV).index_add_(0, slot, w).view(g.n_cols, D, Cw)
        if rest_from_total:
            listed = torch.zeros((g.n_cols, Cw), dtype=dtype, device=DEV).index_add_(0, col, w_rest[row_of])
            V[:, D - 1] = w_rest.sum(dim=0, keepdim=True) - listed
        return V.repeat(1, 1, W // Cw) * rows.unsqueeze(1)
    return run


def measure(case, g, S, lut, use_cnt):
    rft = not g.is_dense
    launch = attribution.prepare_sources(g, S, lut, use_cnt, None, None, rft)
    info = attribution.describe_sources(launch.args)
    routes = {"gnan_attr_cols": launch.run, "torch_index_add": torch_route(g, S, lut, use_cnt, rft)}
    ref = routes["torch_index_add"]()
    got = routes["gnan_attr_cols"]().clone()                         # (run() hands out the launch's own buffer)
    rel = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    truth = routes["torch_index_add"](torch.float64)                  # the same restatement in float64: which route is the closer one
    err = {"gnan_attr_cols": float((got - truth).abs().max() / truth.abs().max().clamp_min(1e-300)),
           "torch_index_add": float((ref - truth).abs().max() / truth.abs().max().clamp_min(1e-300))}
    del truth
    launch.A.fill_(float("nan"))
    again = routes["gnan_attr_cols"]()
    same_bits = bool(torch.equal(got.view(torch.int32), again.view(torch.int32)))
    del ref, got, again
    reps = {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        reps[name] = max(1, min(1000, int(WINDOW_MS / max(timed(fn, 1), 1e-3))))
    times = {k: [] for k in routes}
    for i in range(WARM + SAMPLES):
        for name, fn in routes.items():                               # alternately: both see the same neighbours on the machine
            t = timed(fn, reps[name])
            if i >= WARM:
                times[name].append(t)
    P, D, W = launch.A.shape
    moved = launch.pairs * 9 * info["bin_passes"] + P * D * W * 4
    med = {}
    for name in routes:
        ts = times[name]
        med[name] = statistics.median(ts)
        line = {"what": "explain_sources_time", "case": case, "route": name, "sources": int(P), "pairs": int(launch.pairs), "W": int(W),
                "D": int(D), "median_ms": med[name], "min_ms": min(ts), "max_ms": max(ts), "reps_per_sample": reps[name],
                "samples": len(ts), "max_rel_diff": rel, "max_rel_err_vs_float64": err[name]}
        if name == "gnan_attr_cols":
            line.update(walk_bytes=moved, walk_GBps=moved / med[name] / 1e6, work_items=info["n_items"], launches=info["launches"],
                        bin_passes=info["bin_passes"], workspace_bytes=info["workspace_bytes"], two_runs_same_bits=same_bits)
        print(json.dumps(line), flush=True)
    spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
    print(json.dumps({"what": "explain_sources_time", "case": case, "torch_over_kernel": med["torch_index_add"] / med["gnan_attr_cols"],
                      "spread_kernel": spread["gnan_attr_cols"], "spread_torch": spread["torch_index_add"]}), flush=True)


def symmetric(src, dst):
    return torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])


def case_arxiv():
    n, e = 169343, 1166243
    gen = torch.Generator(device=DEV).manual_seed(1)
    ei = symmetric(*syn.rmat_edges(18, n, e, seed=1, device=DEV))
    g = syn.hop1_csr(ei[0], ei[1], n)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    for W in (1, 129):
        S = torch.randn((n, W), generator=gen, device=DEV)
        measure(f"a{W}: all rows, all sources, arxiv shape, K=1 CSR, W={W}", g, S, lut, True)
        del S
        torch.cuda.empty_cache()


def case_mutagenicity():
    n, W = 30, 15
    gen = torch.Generator().manual_seed(2)
    tree = torch.stack([torch.arange(1, n), (torch.rand(n - 1, generator=gen) * torch.arange(1, n)).long()])
    extra = torch.randint(0, n, (2, n // 10 + 1), generator=gen)
    e = torch.cat([tree, extra], 1)
    g = HopGraph.from_edge_index(symmetric(e[0], e[1]).to(DEV), n)
    S = torch.randn((n, W), generator=gen).to(DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen).to(DEV)
    measure("m: all rows, all sources, 30-node dense graph, Mutagenicity shape", g, S, lut, True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("explain_sources_time.py measures on the GPU: no device visible")
    which = sys.argv[1:] or ["a", "m"]
    for name, fn in (("a", case_arxiv), ("m", case_mutagenicity)):
        if name in which:
            fn()
            torch.cuda.empty_cache()
