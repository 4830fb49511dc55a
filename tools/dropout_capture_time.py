#!/usr/bin/env python3
"""REPLAYED training steps of a graph-level task under training-mode Dropout on one MI355X: the workload of
tools/small_graph_dropout_time.py (``models.TensorGNAN``, F = 15, H = 64, L = 3, ``dropout = 0.6``, ``train()``, one dense graph of
30 / 130 / 417 nodes; forward + BCE + backward + Adam over ``optim_params``) through the two captured paths a Dropout-active model
may take since the seed lives in a device cell:

    python tools/dropout_capture_time.py --route replay     the module's own replay inside the unchanged loop (replay.py: two
                                                            hipGraph launches, one seed store, the loss and Adam eager)
    python tools/dropout_capture_time.py --route harness    harness.train_epoch's captured step (one hipGraph launch, one slot
                                                            load, one seed store per step)
    python tools/dropout_capture_time.py --route floor      --route replay with dropout = 0: the Dropout-free replayed step

The EAGER step to compare with is tools/small_graph_dropout_time.py run on a tree from before this route (there every capture
gate refuses a Dropout-active model; here it measures the eager step as long as ``small_graph.CAPTURE_DROPOUT`` is off, its
default — this tool switches it on).  Protocol (both tools): wall clock
around 20 steps that end in torch.cuda.synchronize(), 30 samples after 5 warm-ups; three fresh processes per route, alternating,
on one machine.  One JSON line per size and run.
"""
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from small_graph_dropout_time import DEV, F, H, P, SAMPLES, SIZES, STEPS, WARM, graph_of      # noqa: E402

ROUTES = ("replay", "harness", "floor")


def stepper(n, route):
    """-> (a function that runs STEPS training steps on the n-node graph, a function that says how many of them were replayed)"""
    import gnan_amd
    import microbench as mb
    from gnan_amd import harness, small_graph
    from gnan_amd.models import TensorGNAN
    small_graph.CAPTURE_DROPOUT = True           # (what is measured here; see the switch for its default)
    data = graph_of(n)
    torch.manual_seed(0)
    m = TensorGNAN(F, 1, 3, hidden_channels=H, dropout=0.0 if route == "floor" else P, is_graph_task=True, readout_n_layers=0,
                   device=DEV)
    mb.redraw(m)
    m = m.to(DEV).train()
    opt = torch.optim.Adam(gnan_amd.optim_params(m), lr=1e-3)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    if route == "harness":
        class Resident(mb.Bag):                      # (the harness moves every batch to the device: this one is there)
            def to(self, device):
                return self
        loader = [Resident(**data.__dict__)] * STEPS

        def steps():
            harness.train_epoch(m, loader, loss_fn, opt, DEV, classify=True, is_graph_task=True)

        def replayed():
            book = harness._steps_of(m).graph
            found = [s.step for s in book.slots.values()] + [r["step"].step for r in book.buckets.values() if r["step"] is not None]
            return sum(s.graph.replays for s in found)
        return steps, replayed

    def steps():
        for _ in range(STEPS):
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(m(data).view(1, 1), data.y)
            loss.backward()
            opt.step()

    def replayed():
        slots = getattr(m.__dict__.get("_replay_slots"), "plans", {})
        cache = m.__dict__.get("_replays")
        plans = [r["plan"] for r in slots.values()] + ([e.value["plan"] for e in cache.entries.values()] if cache is not None else [])
        return sum(p.gen for p in plans if p is not None)
    return steps, replayed


def measure(n, route):
    steps, replayed = stepper(n, route)
    ts = []
    for i in range(WARM + SAMPLES):
        if i == WARM:
            before = replayed()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3 / STEPS)
    share = (replayed() - before) / (SAMPLES * STEPS)
    return {"what": "dropout_capture_time", "route": route, "nodes": n, "F": F, "H": H, "dropout": 0.0 if route == "floor" else P,
            "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps_per_sample": STEPS, "samples": SAMPLES,
            "replayed_share": share}


if __name__ == "__main__":
    route = sys.argv[sys.argv.index("--route") + 1] if "--route" in sys.argv else None
    if route not in ROUTES:
        sys.exit("dropout_capture_time.py --route {%s}" % " | ".join(ROUTES))
    if not torch.cuda.is_available():
        sys.exit("dropout_capture_time.py measures on the GPU: no device visible")
    warnings.simplefilter("ignore")              # (the one-time note that Dropout steps leave the table path)
    for n in SIZES:
        print(json.dumps(measure(n, route)), flush=True)
