#!/usr/bin/env python3
"""Per-row attributions (``gnan_attr_rows``, csrc/attr_rows.hip) on one MI355X against the only alternative a user had before
it: the plain torch restatement on the same device — a one-hot ``index_add_`` of the gathered operand rows over (row, shell).

Cases
  a1 / a1024   one row and 1,024 rows of the arxiv shape (169,343 nodes, F = 128, C = 40: W = 5,120), K = 2 hop-coded CSR of a
               row block of an R-MAT graph with arxiv's edge count (no data sets offline)
  b            all rows of a 417-node dense graph of the Mutagenicity shape (a random tree plus extra edges, W = 15)
  c            the longest (hub) row of the bench's R-MAT graph (scale 24, 10M nodes, 100M edges, K = 1) at W = 64

Protocol: both routes in this one process, alternately; HIP events around ``reps`` calls (``reps`` sized so that a window holds
about 20 ms of work), 5 warm-ups, 30 samples (5 where one call takes more than a second); median, min and max per call.  The
kernel route is ``attribution.Launch.run`` — the two launches, nothing else; the torch route gets its batch split (it cannot hold
``pairs x W`` floats at once) computed outside the window.  ``gather_GBps``: pairs of the requested rows x W x 4 bytes x shell
passes over the median (the operand bytes the first launch gathers; index and output bytes are not counted).  The two results
are compared (``max_rel_diff``, relative to the largest entry).  One JSON line per case and route."""
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
WARM, SAMPLES, WINDOW_MS = 5, 30, 20.0
TORCH_BATCH_BYTES = 1 << 31          # gathered rows the torch route holds at once


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_route(g, S, lut, use_cnt, rows, s_total):
    """-> a callable computing ``A [R, D, W]`` with stock torch ops on the device, rows in batches of TORCH_BATCH_BYTES."""
    D, W, Cw = g.n_codes, S.shape[1], lut.shape[-1]
    ids = torch.arange(g.n_rows, device=DEV) if rows is None else rows.long()
    if g.is_dense:
        deg = torch.full((ids.numel(),), g.n_cols, dtype=torch.int64, device=DEV)
    else:
        rp = g.rowptr.long()
        deg = rp[ids + 1] - rp[ids]
    batches, lo, acc = [], 0, 0
    for q, d in enumerate(deg.tolist()):                              # the split: host work outside the timed window
        if acc and (acc + d) * W * 4 > TORCH_BATCH_BYTES:
            batches.append((lo, q))
            lo, acc = q, 0
        acc += d
    batches.append((lo, ids.numel()))
    code, col = g.code.long() if g.is_dense else g.code, None if g.is_dense else g.col.long()

    def run():
        out = []
        for b0, b1 in batches:
            r = ids[b0:b1]
            n = r.numel()
            if g.is_dense:
                slot = (torch.arange(n, device=DEV).unsqueeze(1) * D + code[r].clamp(max=D - 1)).reshape(-1)
                src = torch.arange(g.n_cols, device=DEV).repeat(n)
            else:
                first, dg = rp[r], deg[b0:b1]
                q_of = torch.repeat_interleave(torch.arange(n, device=DEV), dg)
                pair = torch.arange(int(dg.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(dg, 0) - dg, dg) + first[q_of]
                slot = q_of * D + code[pair].long().clamp(max=D - 1)
                src = col[pair]
            Z = torch.zeros((n * D, W), dtype=torch.float32, device=DEV).index_add_(0, slot, S[src]).view(n, D, W)
            if s_total is not None:
                Z[:, D - 1] = s_total.unsqueeze(0) - Z[:, : D - 1].sum(dim=1)
            wt = lut.unsqueeze(0).expand(n, D, Cw)
            if use_cnt:
                wt = wt / g.cnt[r].clamp_min(1).float().unsqueeze(-1)
            out.append(wt.repeat(1, 1, W // Cw) * Z)
        return torch.cat(out)
    return run


def measure(case, g, S, lut, use_cnt, rows, s_total):
    launch = attribution.prepare(g, S, lut, use_cnt, rows, s_total)
    info = attribution.describe(launch.args)
    routes = {"gnan_attr_rows": launch.run, "torch_index_add": torch_route(g, S, lut, use_cnt, rows, s_total)}
    ref = routes["torch_index_add"]()
    got = routes["gnan_attr_rows"]()
    rel = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    del ref, got
    reps, samples = {}, {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        once = timed(fn, 1)
        reps[name] = max(1, min(1000, int(WINDOW_MS / max(once, 1e-3))))
        samples[name] = 5 if once > 1000.0 else SAMPLES
    times = {k: [] for k in routes}
    for i in range(WARM + SAMPLES):
        for name, fn in routes.items():                               # alternately: both see the same neighbours on the machine
            if i < WARM + samples[name]:
                t = timed(fn, reps[name])
                if i >= WARM:
                    times[name].append(t)
    gathered = launch.pairs * S.shape[1] * 4 * info["shell_passes"]
    for name in routes:
        ts = times[name]
        line = {"what": "explain_time", "case": case, "route": name, "rows": int(launch.A.shape[0]), "pairs": int(launch.pairs),
                "W": int(S.shape[1]), "D": int(g.n_codes), "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                "reps_per_sample": reps[name], "samples": len(ts), "max_rel_diff": rel}
        if name == "gnan_attr_rows":
            line.update(gather_bytes=gathered, gather_GBps=gathered / statistics.median(ts) / 1e6, work_items=info["n_items"],
                        col_tiles=info["col_tiles"], shell_passes=info["shell_passes"], workspace_bytes=info["workspace_bytes"])
        print(json.dumps(line), flush=True)


def symmetric(src, dst):
    return torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])


def case_arxiv():
    n, e, W = 169343, 1166243, 128 * 40
    gen = torch.Generator(device=DEV).manual_seed(1)
    ei = symmetric(*syn.rmat_edges(18, n, e, seed=1, device=DEV))
    g = HopGraph.from_edge_index(ei, n, max_hops=2, layout="csr", rows=(0, 1024))      # the rows asked for: a block of 1,024
    S = torch.randn((n, W), generator=gen, device=DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    tot = column_sums(S)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long()
    median_row = torch.argsort(deg)[deg.numel() // 2].view(1).to(torch.int32)
    measure("a1: one row (median length), arxiv shape, K=2 CSR", g, S, lut, True, median_row, tot)
    measure("a1024: 1,024 rows, arxiv shape, K=2 CSR", g, S, lut, True, None, tot)


def case_mutagenicity():
    n, W = 417, 15
    gen = torch.Generator().manual_seed(2)
    tree = torch.stack([torch.arange(1, n), (torch.rand(n - 1, generator=gen) * torch.arange(1, n)).long()])
    extra = torch.randint(0, n, (2, n // 30 + 1), generator=gen)
    e = torch.cat([tree, extra], 1)
    g = HopGraph.from_edge_index(symmetric(e[0], e[1]).to(DEV), n)
    S = torch.randn((n, W), generator=gen).to(DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen).to(DEV)
    measure("b: all rows, 417-node dense graph, Mutagenicity shape", g, S, lut, True, None, None)


def case_hub():
    n, e, W = 10_000_000, 100_000_000, 64
    gen = torch.Generator(device=DEV).manual_seed(3)
    g = syn.hop1_csr(*syn.rmat_edges(24, n, e, seed=0, device=DEV), n)
    S = torch.randn((n, W), generator=gen, device=DEV)
    lut = torch.randn((g.n_codes, 1), generator=gen, device=DEV)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    hub = torch.argmax(deg).view(1).to(torch.int32)
    measure("c: the hub row of the bench's R-MAT graph, W=64", g, S, lut, True, hub, column_sums(S))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("explain_time.py measures on the GPU: no device visible")
    which = sys.argv[1:] or ["a", "b", "c"]
    for name, fn in (("a", case_arxiv), ("b", case_mutagenicity), ("c", case_hub)):
        if name in which:
            fn()
            torch.cuda.empty_cache()
