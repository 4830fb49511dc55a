#!/usr/bin/env python3
"""Eager training steps of a graph-level task UNDER TRAINING-MODE DROPOUT on one MI355X: what the reference's one documented
invocation feeds (run.sh: n_layers = 3, hidden_channels = 64, dropout = 0.6, a module that starts in train mode).

``models.TensorGNAN(F = 15, out = 1, n_layers = 3, hidden_channels = 64, dropout = 0.6, is_graph_task, readout_n_layers = 0)``
in ``train()`` mode on ONE dense graph per size: a Mutagenicity-shaped graph of 30 nodes (``synthetic.mutagenicity_shaped_graphs``:
the first it draws with 30 nodes) and the same recipe at 130 and 417 nodes.  A step is the public module API only — forward,
BCE-with-logits, ``backward()``, Adam over ``gnan_amd.optim_params`` — so this file runs unchanged on a tree from before the
one-launch Dropout routes and on one with them (fresh processes, alternating, on one machine: that is the comparison).

    python tools/small_graph_dropout_time.py                   wall clock around 20 steps that end in torch.cuda.synchronize(),
                                                               30 samples after 5 warm-ups: one JSON line per size
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o k -- python tools/small_graph_dropout_time.py --count
                                                               per size: a marker launch, COUNT_STEPS steps, a marker launch
    python tools/small_graph_dropout_time.py --parse DIR       kernel launches per step from that trace: one JSON line per size
"""
import csv
import glob
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

DEV = "cuda"
F, H, P = 15, 64, 0.6
SIZES = (30, 130, 417)
STEPS, SAMPLES, WARM = 20, 30, 5
COUNT_STEPS = 10
MARKER = "erfinv"            # a kernel no step launches: the trace is cut at its launches


def graph_of(n):
    """Tree + n // 30 + 1 extra edges, one-hot of 14 atom types + the ones column: synthetic.mutagenicity_shaped_graphs' recipe (its
    own first 30-node graph at n = 30)."""
    import microbench as mb
    from gnan_amd import synthetic
    if n == 30:
        ei, x, label = next(t for t in synthetic.mutagenicity_shaped_graphs(4096, seed=0) if t[1].shape[0] == 30)
    else:
        rng = np.random.default_rng(n)
        tree = np.stack([np.arange(1, n), rng.integers(0, np.arange(1, n))])
        extra = np.stack([rng.integers(0, n, n // 30 + 1), rng.integers(0, n, n // 30 + 1)])
        ei = np.concatenate([tree, extra], axis=1)
        ei = np.concatenate([ei, ei[::-1]], axis=1)
        ei = np.unique(ei[:, ei[0] != ei[1]], axis=1)
        x = torch.zeros(n, F)
        x[torch.arange(n), torch.from_numpy(rng.integers(0, F - 1, n))] = 1.0
        x[:, -1] = 1.0
        label = 1.0
    nd, norm = mb.dense_inputs(ei, n)
    return mb.Bag(x=x.to(DEV), y=torch.tensor([[1.0 if label > 0 else 0.0]], device=DEV), edge_index=None, node_distances=nd,
                  normalization_matrix=norm)


def stepper(n):
    """-> a function that runs one eager training step on the n-node graph"""
    import gnan_amd
    import microbench as mb
    from gnan_amd.models import TensorGNAN
    data = graph_of(n)
    torch.manual_seed(0)
    m = TensorGNAN(F, 1, 3, hidden_channels=H, dropout=P, is_graph_task=True, readout_n_layers=0, device=DEV)
    mb.redraw(m)
    m = m.to(DEV).train()
    opt = torch.optim.Adam(gnan_amd.optim_params(m), lr=1e-3)
    loss_fn = torch.nn.BCEWithLogitsLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = loss_fn(m(data).view(1, 1), data.y)
        loss.backward()
        opt.step()
    return step


def measure(n):
    step = stepper(n)
    ts = []
    for i in range(WARM + SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3 / STEPS)
    return {"what": "small_graph_dropout_time", "nodes": n, "F": F, "H": H, "dropout": P, "median_ms": statistics.median(ts),
            "min_ms": min(ts), "max_ms": max(ts), "steps_per_sample": STEPS, "samples": SAMPLES}


def count(n):
    step = stepper(n)
    for _ in range(WARM):
        step()
    mark = torch.full((1,), 0.5, device=DEV)
    torch.cuda.synchronize()
    torch.erfinv(mark)
    for _ in range(COUNT_STEPS):
        step()
    torch.erfinv(mark)
    torch.cuda.synchronize()


def parse(out_dir):
    """Launches between the 2 k-th and the 2 k + 1-th marker of the kernel trace, per step, for size k; and which kernels they were."""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for f in files for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
    if len(cuts) != 2 * len(SIZES):
        sys.exit("small_graph_dropout_time.py: expected %d marker launches in the trace, found %d" % (2 * len(SIZES), len(cuts)))
    for k, n in enumerate(SIZES):
        seg = rows[cuts[2 * k] + 1: cuts[2 * k + 1]]
        names = {}
        for r in seg:
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            names[name] = names.get(name, 0) + 1
        ours = sum(c for name, c in names.items() if "_kernel" in name and "at::" not in name)
        print(json.dumps({"what": "small_graph_dropout_launches", "nodes": n, "launches_per_step": len(seg) / COUNT_STEPS,
                          "library_launches_per_step": ours / COUNT_STEPS, "steps": COUNT_STEPS,
                          "per_step": {k_: c / COUNT_STEPS for k_, c in sorted(names.items())}}), flush=True)


if __name__ == "__main__":
    if "--parse" in sys.argv:
        parse(sys.argv[sys.argv.index("--parse") + 1])
        sys.exit(0)
    if not torch.cuda.is_available():
        sys.exit("small_graph_dropout_time.py measures on the GPU: no device visible")
    warnings.simplefilter("ignore")              # (the one-time note that Dropout steps leave the table path)
    for n in SIZES:
        if "--count" in sys.argv:
            count(n)
        else:
            print(json.dumps(measure(n)), flush=True)
