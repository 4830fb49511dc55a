#!/usr/bin/env python3
"""A replayed training step of a graph-level task WITH a NAM read-out on ONE dense graph of 130, 200 and 417 nodes, on one MI355X:
the route of csrc/mid_graph_nam.hip (one launch forward, two backward) against the general kernels (``small_graph.MID_GRAPH_NAM`` off:
the table, the operand, ``rho_aggregate``, ``gnan_colsum`` and the read-out's MLPs — the route such graphs took before).

``models.TensorGNAN(F = 15, out = 1, n_layers = 3, hidden_channels = 64, is_graph_task, readout_n_layers = R)`` for R = 1 and R = 2;
tools/mid_graph_time.py's protocol, unchanged: the step is the harness's own per-shape captured step (forward + BCE loss + backward +
Adam over ``optim_params``).  Both routes are captured in this one process and their replays are timed alternately: HIP events around
``REPLAYS`` replays, 30 samples after 5 warm-ups, median / min / max in ms per step, and the kernel count of each captured step.
Prints one JSON line per read-out depth, size and route; ``faster`` says whether the new route's median lies below the general route's
by more than the general route's own spread (max - min of its 30 samples)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import microbench as mb  # noqa: E402
import gnan_amd  # noqa: E402
from gnan_amd import harness, small_graph  # noqa: E402
from mid_graph_time import DEV, F, H, REPLAYS, SAMPLES, SIZES, WARM, graph_of, sample  # noqa: E402

READOUTS = (1, 2)


def captured_step(data, readout, mid):
    """-> (the model, what keeps its step alive, its captured per-shape step) with the route frozen into the capture."""
    shipped = small_graph.MID_GRAPH_NAM
    small_graph.MID_GRAPH_NAM = mid
    try:
        torch.manual_seed(0)
        m = mb.TensorGNAN(F, 1, 3, hidden_channels=H, is_graph_task=True, readout_n_layers=readout, device=DEV)
        mb.redraw(m)
        m = m.to(DEV).eval()
        opt = torch.optim.Adam(gnan_amd.optim_params(m), lr=1e-3)
        loss_fn = torch.nn.BCEWithLogitsLoss()
        for _ in range(12):
            harness.train_epoch(m, [data], loss_fn, opt, DEV, classify=True, is_graph_task=True)
            recs = [r for r in harness._steps_of(m).graph.buckets.values() if r["step"] is not None]
            if recs:
                return m, (opt, loss_fn), recs[0]["step"].step
    finally:
        small_graph.MID_GRAPH_NAM = shipped
    raise SystemExit("mid_graph_nam_time.py: the per-shape step was not captured")


def measure(n, readout):
    data = graph_of(n, n)
    routes = {"general": captured_step(data, readout, False), "mid_graph_nam": captured_step(data, readout, True)}
    times = {k: [] for k in routes}
    for i in range(WARM + SAMPLES):
        for name, (_, _, step) in routes.items():          # alternately: both routes see the same neighbours on the machine
            t = sample(step)
            if i >= WARM:
                times[name].append(t)
    out = []
    for name, (_, _, step) in routes.items():
        ts = times[name]
        out.append({"what": "mid_graph_nam_time", "readout_n_layers": readout, "route": name, "nodes": n, "F": F, "H": H,
                    "shells": int(step.model.hop_graph(data).n_codes), "kernels": step.graph.kernel_nodes,
                    "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "replays_per_sample": REPLAYS,
                    "samples": SAMPLES})
    old, new = out
    new["faster"] = new["median_ms"] < old["median_ms"] - (old["max_ms"] - old["min_ms"])
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("mid_graph_nam_time.py measures on the GPU: no device visible")
    for readout in READOUTS:
        for n in SIZES:
            for line in measure(n, readout):
                print(json.dumps(line), flush=True)
