#!/usr/bin/env python3
"""Three-layer shape functions of 128 hidden units (L = 3, H = 128): the parameter-gradient route of the tree this file runs in,
on one MI355X, at the arxiv shape (F = 128, n = 169 343).

  grads   the last stage of the table path's backward on one set of tables and moments, C = 1 and C = 40: gnan_fpwl_param_grads
          where ``functional._wide_table_grads_applies`` says so, else pwl.parameter_grads_from_moments (two probe points per piece
          in float64) — which is what a tree from before the wide instance, or one with ``WIDE_TABLE_GRADS`` off, takes
  step    the arxiv-shaped harness training step (forward + loss + backward + Adam) at H = 128 with the tree's defaults

The same file measures both sides of a comparison: run it in this tree and in the parent commit's built tree (fresh processes,
alternating, on one box); the route taken is part of every line.  Wall-clock medians with a device synchronisation per call (host
launch overhead is what the probe route is made of), 30 calls after 5 warm-ups.  Prints one JSON line per measurement.
``python tools/wide_tables_time.py [grads] [step]``."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import microbench as mb  # noqa: E402
from gnan_amd import functional, harness, pwl  # noqa: E402

DEV = "cuda"
L, H = 3, 128


def wide_route(C):
    gate = getattr(functional, "_wide_table_grads_applies", None)
    return bool(gate is not None and gate(L, H, C))


def model(F, C=1):
    torch.manual_seed(0)
    m = mb.TensorGNAN(F, C, L, hidden_channels=H, device=DEV)
    mb.redraw(m)
    return m.to(DEV).eval()


def grad_times():
    F, n = 128, 169_343
    for C in (1, 40):
        m = model(F, C)
        with torch.no_grad():
            st = mb.stack_mlps(m.fs)
            t = pwl.build_tables(st)
            x = mb.syn.block_features(n, F, 0, n, 1, DEV)
            g = torch.randn(n, C, device=DEV)
            M = functional._fpwl_moments(x, t, g, True, raw=True)
            M32 = functional._fpwl_moments(x, t, g, True)

        def hip():
            return functional._fpwl_param_grads_launch(list(st[:6]), t, M, L, H, C, F)

        def probe():
            leaves = [None if q is None else q.detach().clone().requires_grad_(True) for q in st[:6]]
            return pwl.parameter_grads_from_moments(
                functional.StackedMLP(*leaves, *st[6:]), t, M32,
                lambda U, q: functional._fmlp_eager(U, functional.StackedMLP(*[None if a is None else a.double() for a in q[:6]], *q[6:]),
                                                    False))
        wide = wide_route(C)
        med, low = mb.timeit(hip if wide else probe, reps=30, warm=5)
        print(json.dumps({"what": "grads", "shape": "arxiv", "F": F, "L": L, "H": H, "C": C, "pieces": int(t.anchor.numel()),
                          "route": "gnan_fpwl_param_grads" if wide else "probe_points", "ms": med, "min_ms": low}), flush=True)


def step_times():
    import graphed_step as gs
    d, n, F, C = gs.arxiv_shaped(1)
    gen = torch.Generator().manual_seed(1)
    d.y = torch.randint(0, 2, (n,), generator=gen).to(DEV)
    d.train_mask = (torch.rand(n, generator=gen) < 0.6).to(DEV)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    m = model(F)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    med, low = mb.timeit(lambda: harness.train_epoch(m, [d], loss_fn, opt, DEV, classify=True, is_graph_task=False), reps=30, warm=6)
    store = harness._steps_of(m)
    replays = sum(r.value["step"].graph.replays for r in store.node.entries.values() if r.value["step"] is not None)
    harness.release_steps(m)
    print(json.dumps({"what": "step", "shape": "arxiv", "F": F, "L": L, "H": H, "C": C,
                      "route": "gnan_fpwl_param_grads" if wide_route(C) else "probe_points", "ms": med, "min_ms": low,
                      "replays": replays}), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["grads", "step"]
    if "grads" in which:
        grad_times()
    if "step" in which:
        step_times()
