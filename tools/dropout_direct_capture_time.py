#!/usr/bin/env python3
"""``harness.train_epoch`` steps under training-mode Dropout (``dropout = 0.6``, ``train()``) on the GENERAL route of one MI355X —
the shapes whose Dropout forwards run the direct kernels (gnan_fmlp_fwd / gnan_fmlp_bwd and their matrix-core relatives):

    tolokers   a full-batch node task, n = 11 758, F = 10, one output channel, H = 64, L = 3, a one-hop CSR graph
    cora       a full-batch node task, n = 2 708, F = 1 433, C = 7, H = 64, L = 3, a one-hop CSR graph
    dense449   a graph-level task's training step on one dense graph of 449 nodes, F = 15 (past the one-launch routes)

    python tools/dropout_direct_capture_time.py [--shape tolokers|cora|dense449]

This tree: ``functional.CAPTURE_DROPOUT_DIRECT`` is switched on, so from the third step on every step is a replayed hipGraph whose
kernels read the masks' seed from a device cell (``replayed_share`` must be 1.0).  A tree from before the switch — copy this file
into its ``tools/`` — has no such attribute: every capture gate refuses a Dropout-active model on these shapes and the same loop
runs eagerly (``replayed_share`` 0.0): the figure to compare with.  Protocol (that of tools/dropout_capture_time.py): wall clock
around 20 steps that end in torch.cuda.synchronize(), 30 samples after 5 warm-ups; three fresh processes per tree, alternating, on
one machine.  One JSON line per shape and run.
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

DEV, P, H, STEPS, WARM, SAMPLES = "cuda", 0.6, 64, 20, 5, 30
SHAPES = {"tolokers": (11758, 10, 1), "cora": (2708, 1433, 7), "dense449": (449, 15, 1)}


class Resident:
    """A batch that lives on the device (the harness moves every batch there: this one is)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to(self, device):
        return self


def node_task(n, F, C):
    from gnan_amd import synthetic as syn
    g = torch.Generator().manual_seed(0)
    x = torch.rand(n, F, generator=g)
    y = torch.randint(0, max(C, 2), (n,), generator=g)
    masks = torch.rand(n, generator=g)
    src, dst = syn.uniform_edges(n, 6 * n, 0, DEV)
    return Resident(x=x.to(DEV), y=y.to(DEV), edge_index=None, train_mask=(masks < 0.6).to(DEV), val_mask=(masks >= 0.8).to(DEV),
                    test_mask=(masks >= 0.8).to(DEV), gnan_graph=syn.hop1_csr(src, dst, n))


def stepper(shape):
    """-> (a function that runs STEPS training steps, a function that says how many steps were replayed so far)"""
    import gnan_amd
    import microbench as mb
    from gnan_amd import functional, harness
    from gnan_amd.models import TensorGNAN
    functional.CAPTURE_DROPOUT_DIRECT = True         # (what is measured here; a tree from before the switch ignores the name)
    n, F, C = SHAPES[shape]
    graph_task = shape == "dense449"
    torch.manual_seed(0)
    m = TensorGNAN(F, C, 3, hidden_channels=H, dropout=P, is_graph_task=graph_task, readout_n_layers=0, device=DEV)
    mb.redraw(m)
    m = m.to(DEV).train()
    opt = torch.optim.Adam(gnan_amd.optim_params(m), lr=1e-3)
    if graph_task:
        from small_graph_dropout_time import graph_of
        loss_fn = torch.nn.BCEWithLogitsLoss()
        loader = [Resident(**graph_of(n).__dict__)] * STEPS

        def steps():
            harness.train_epoch(m, loader, loss_fn, opt, DEV, classify=True, is_graph_task=True)

        def replayed():
            book = harness._steps_of(m).graph
            if book is None:
                return 0
            found = [s.step for s in book.slots.values()] + [r["step"].step for r in book.buckets.values() if r["step"] is not None]
            return sum(s.graph.replays for s in found)
        return steps, replayed
    data = node_task(n, F, C)
    loss_fn = torch.nn.BCEWithLogitsLoss() if C == 1 else torch.nn.CrossEntropyLoss()

    def steps():
        for _ in range(STEPS):
            harness.train_epoch(m, [data], loss_fn, opt, DEV, classify=True, is_graph_task=False)

    def replayed():
        recs = [e.value["step"] for e in harness._steps_of(m).node.entries.values()]
        return sum(s.graph.replays for s in recs if s is not None)
    return steps, replayed


def measure(shape):
    steps, replayed = stepper(shape)
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
    n, F, C = SHAPES[shape]
    return {"what": "dropout_direct_capture_time", "shape": shape, "nodes": n, "F": F, "C": C, "H": H, "dropout": P,
            "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "steps_per_sample": STEPS, "samples": SAMPLES,
            "replayed_share": (replayed() - before) / (SAMPLES * STEPS)}


if __name__ == "__main__":
    only = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else None
    if only is not None and only not in SHAPES:
        sys.exit("dropout_direct_capture_time.py [--shape {%s}]" % " | ".join(SHAPES))
    if not torch.cuda.is_available():
        sys.exit("dropout_direct_capture_time.py measures on the GPU: no device visible")
    warnings.simplefilter("ignore")              # (the one-time note that Dropout steps leave the table path)
    for shape in ([only] if only else SHAPES):
        print(json.dumps(measure(shape)), flush=True)
