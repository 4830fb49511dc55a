#!/usr/bin/env python3
"""A replayed training step of a graph-level task on ONE dense graph of 130, 200 and 417 nodes, on one MI355X: the one-launch
route of csrc/mid_graph.hip against the general kernels (``small_graph.MID_GRAPH`` off: the route such graphs took before).

``models.TensorGNAN(F = 15, out = 1, n_layers = 3, hidden_channels = 64, is_graph_task, readout_n_layers = 0)``; the step is
the harness's own per-shape captured step (forward + BCE loss + backward + Adam over ``optim_params``).  Both routes are
captured in this one process and their replays are timed alternately: HIP events around ``REPLAYS`` replays, 30 samples after
5 warm-ups, median / min / max in ms per step, and the kernel count of each captured step.  Prints one JSON line per route;
``faster`` says whether the new route's median lies below the general route's by more than the general route's own spread
(max - min of its 30 samples).

``--model standalone``: the stand-alone class ``gnan_amd.GNAN.TensorGNAN(15, 1, 3, hidden_channels = 64, is_graph_task)`` with its
default pre-rho normalisation (GNAN.py:65-67) — the one-launch route behind ``small_graph.MID_GRAPH_PRE_RHO`` against the general
kernels (the switch off: rho's row table, the operand, ``pre_rho_aggregate`` and their backward launches).  The same protocol."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import microbench as mb  # noqa: E402
import gnan_amd  # noqa: E402
from gnan_amd import harness, small_graph  # noqa: E402

DEV = "cuda"
F, H = 15, 64
SIZES = (130, 200, 417)
REPLAYS, SAMPLES, WARM = 20, 30, 5


class Data(mb.Bag):
    def to(self, device):
        return self


def graph_of(n, seed):
    """A random tree + n / 30 extra edges, one-hot of 14 atom types + a ones column (tools/graphed_step.py's muta_shaped)."""
    rng = np.random.default_rng(seed)
    tree = np.stack([np.arange(1, n), rng.integers(0, np.arange(1, n))])
    extra = np.stack([rng.integers(0, n, n // 30 + 1), rng.integers(0, n, n // 30 + 1)])
    ei = np.concatenate([tree, extra], axis=1)
    nd, norm = mb.dense_inputs(np.concatenate([ei, ei[::-1]], axis=1), n)
    x = torch.zeros(n, F)
    x[torch.arange(n), torch.from_numpy(rng.integers(0, F - 1, n))] = 1.0
    x[:, -1] = 1.0
    return Data(x=x.to(DEV), y=torch.tensor([[1.0]]).to(DEV), edge_index=None, node_distances=nd.to(DEV),
                normalization_matrix=norm.to(DEV))


MODEL = "models"              # --model: "models" (models.TensorGNAN, post-rho) or "standalone" (GNAN.TensorGNAN, pre-rho)


def captured_step(data, mid):
    """-> (the model, its captured per-shape step) with the route frozen into the capture."""
    switch = "MID_GRAPH" if MODEL == "models" else "MID_GRAPH_PRE_RHO"
    shipped = getattr(small_graph, switch)
    setattr(small_graph, switch, mid)
    torch.manual_seed(0)
    if MODEL == "models":
        m = mb.TensorGNAN(F, 1, 3, hidden_channels=H, is_graph_task=True, readout_n_layers=0, device=DEV)
    else:
        from gnan_amd import GNAN as standalone
        m = standalone.TensorGNAN(F, 1, 3, hidden_channels=H, is_graph_task=True, device=DEV)
    mb.redraw(m)
    m = m.to(DEV).eval()
    opt = torch.optim.Adam(gnan_amd.optim_params(m), lr=1e-3)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    keep = (opt, loss_fn)
    for _ in range(12):
        harness.train_epoch(m, [data], loss_fn, opt, DEV, classify=True, is_graph_task=True)
        recs = [r for r in harness._steps_of(m).graph.buckets.values() if r["step"] is not None]
        if recs:
            setattr(small_graph, switch, shipped)
            return m, keep, recs[0]["step"].step
    raise SystemExit("mid_graph_time.py: the per-shape step was not captured")


def sample(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        step.graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPLAYS


def measure(n):
    data = graph_of(n, n)
    routes = {"general": captured_step(data, False), "mid_graph": captured_step(data, True)}
    times = {k: [] for k in routes}
    for i in range(WARM + SAMPLES):
        for name, (_, _, step) in routes.items():          # alternately: both routes see the same neighbours on the machine
            t = sample(step)
            if i >= WARM:
                times[name].append(t)
    out = []
    for name, (_, _, step) in routes.items():
        ts = times[name]
        out.append({"what": "mid_graph_time", "model": MODEL, "route": name, "nodes": n, "F": F, "H": H, "shells": int(step.model.hop_graph(data).n_codes),
                    "kernels": step.graph.kernel_nodes, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                    "replays_per_sample": REPLAYS, "samples": SAMPLES})
    old, new = out
    new["faster"] = new["median_ms"] < old["median_ms"] - (old["max_ms"] - old["min_ms"])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", choices=("models", "standalone"), default="models")
    MODEL = ap.parse_args().model
    if not torch.cuda.is_available():
        sys.exit("mid_graph_time.py measures on the GPU: no device visible")
    for n in SIZES:
        for line in measure(n):
            print(json.dumps(line), flush=True)
