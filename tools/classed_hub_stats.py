"""C4 graph (python3 tools/classed_hub_stats.py): per-class pair totals of the hub rows and the classed plan's sizes / build time per threshold and slice length."""
import json, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gnan_amd  # noqa
from gnan_amd import synthetic as syn, graph as G
src, dst = syn.rmat_edges(24, 10_000_000, 100_000_000, seed=0, device="cuda")
g = syn.hop1_csr(src, dst, 10_000_000)
del src, dst
copy, order, plan = g.degree_sorted_copy()
print(json.dumps({"nnz": g.nnz, "hub_rows_512": plan.n_long, "slices_512": plan.n_slices}), flush=True)
for thr, se in ((512, 2048), (256, 2048), (128, 2048), (512, 1024), (512, 4096)):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    cp = copy.classed_hub_plan(None, thr, se)
    torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
    cls = torch.bincount((cp.index.long() & 7), minlength=8).tolist()
    mean = sum(cls) / 8
    q = [int(((cp.slot_slice[k::8]) >= 0).sum()) for k in range(8)]
    print(json.dumps({"threshold": thr, "slice_edges": se, "build_ms": round(ms, 2), "hub_rows": cp.n_long, "pairs": int(cp.index.numel()),
                      "pair_share": round(cp.index.numel() / g.nnz, 4), "class_pairs": cls, "max_over_mean": round(max(cls) / mean, 4),
                      "slices": cp.n_slices, "slots": cp.n_slots, "queue_lengths": q}), flush=True)
