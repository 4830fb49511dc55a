#!/usr/bin/env python3
"""Four-layer shape functions (L = 4, H = 64): the kernel routes against the torch routes they replace, on one MI355X.

  build   gnan_pwl_build (two launches + the read-back) vs the graph-replayed pwl._build_padded, counted from the weights'
          copy to the end of tolist(), for the arxiv shape (F = 128, C = 1) and the C4 shape (F = 64, C = 1)
  grads   gnan_fpwl_param_grads vs pwl.parameter_grads_from_moments on the arxiv shape's tables and moments
  step    the arxiv-shaped harness training step (forward + loss + backward + Adam): replayed hipGraph with the kernels vs
          the eager loop with the torch builder and the probe-point gradients (what a four-layer model ran before)

Wall-clock medians with a device synchronisation per call (host launch overhead is what the torch routes are made of).
Prints one JSON line per measurement.  ``python tools/deep_tables_time.py [build] [grads] [step]``."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import microbench as mb  # noqa: E402
from gnan_amd import functional, harness, pwl  # noqa: E402

DEV = "cuda"
L, H = 4, 64


def model(F, C=1):
    torch.manual_seed(0)
    m = mb.TensorGNAN(F, C, L, hidden_channels=H, device=DEV)
    mb.redraw(m)
    return m.to(DEV).eval()


def build_times():
    for name, F in (("arxiv", 128), ("c4", 64)):
        m = model(F)
        with torch.no_grad():
            st = mb.stack_mlps(m.fs)
            out = {"what": "build", "shape": name, "F": F, "L": L, "H": H}
            for tag, backend in (("hip", "auto"), ("torch_graph", "torch")):
                pwl.BUILD_BACKEND = backend
                t = pwl.build_tables(st)
                out[tag + "_ms"] = mb.timeit(lambda: pwl.build_tables(st), reps=30, warm=5)[0]
                out[tag + "_pieces"] = int(t.anchor.numel())
            pwl.BUILD_BACKEND = "auto"
        print(json.dumps(out), flush=True)


def grad_times():
    F, C, n = 128, 1, 169_343
    m = model(F)
    with torch.no_grad():
        st = mb.stack_mlps(m.fs)
        t = pwl.build_tables(st)
        x = mb.syn.block_features(n, F, 0, n, 1, DEV)
        g = torch.randn(n, C, device=DEV)
        M = functional._fpwl_moments(x, t, g, True, raw=True)
        M32 = functional._fpwl_moments(x, t, g, True)
        hip = lambda: functional._fpwl_param_grads_launch(list(st[:6]), t, M, L, H, C, F)                 # noqa: E731

    def probe():
        leaves = [None if q is None else q.detach().clone().requires_grad_(True) for q in st[:6]]
        return pwl.parameter_grads_from_moments(
            functional.StackedMLP(*leaves, *st[6:]), t, M32,
            lambda U, q: functional._fmlp_eager(U, functional.StackedMLP(*[None if a is None else a.double() for a in q[:6]], *q[6:]), False))
    print(json.dumps({"what": "grads", "shape": "arxiv", "F": F, "L": L, "H": H, "pieces": int(t.anchor.numel()),
                      "hip_ms": mb.timeit(hip, reps=30, warm=5)[0], "probe_points_ms": mb.timeit(probe, reps=30, warm=5)[0]}), flush=True)


def step_times():
    import graphed_step as gs
    d, n, F, C = gs.arxiv_shaped(1)
    gen = torch.Generator().manual_seed(1)
    d.y = torch.randint(0, 2, (n,), generator=gen).to(DEV)
    d.train_mask = (torch.rand(n, generator=gen) < 0.6).to(DEV)
    loss_fn = torch.nn.BCEWithLogitsLoss()
    out = {"what": "step", "shape": "arxiv", "F": F, "L": L, "H": H}
    for tag, kernels in (("torch_routes_eager", False), ("kernels_replayed", True)):
        harness.GRAPHED_STEPS = kernels
        functional.HIP_TABLE_GRADS = kernels
        pwl.BUILD_BACKEND = "auto" if kernels else "torch"
        m = model(F)
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out[tag + "_ms"] = mb.timeit(lambda: harness.train_epoch(m, [d], loss_fn, opt, DEV, classify=True, is_graph_task=False),
                                     reps=30, warm=6)[0]
        if kernels:
            store = harness._steps_of(m)
            out["replays"] = sum(r.value["step"].graph.replays for r in store.node.entries.values() if r.value["step"] is not None)
            harness.release_steps(m)
    harness.GRAPHED_STEPS, functional.HIP_TABLE_GRADS, pwl.BUILD_BACKEND = True, True, "auto"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["build", "grads", "step"]
    if "build" in which:
        build_times()
    if "grads" in which:
        grad_times()
    if "step" in which:
        step_times()
