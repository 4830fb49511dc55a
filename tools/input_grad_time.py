#!/usr/bin/env python3
"""The backward pass of the shape functions with ``x.requires_grad`` on the table path, on one MI355X.

Per shape three backward passes of ``feature_mlps(x, p, sum_features=True)`` are timed, each from the gradient of the result to
the last gradient kernel (HIP events around ``backward``; the forward runs before the first event):

  x_grad        parameters and x need gradients: moments + gnan_fpwl_param_grads + gnan_pwl_piece_dfdx + gnan_fpwl_input_grad
  restatement   the same call on the route it took before the tables served x.grad (``HIP_TABLE_GRADS`` off for the backward:
                the batched-GEMM restatement in chunks of nodes, parameter gradients and x.grad from ``[F, n, H]`` activations)
  params_only   x needs no gradient: moments + gnan_fpwl_param_grads

and, on their own, the two new launches (``dfdx``, ``lookup``).  Shapes: n = 2^18, H = 64; F = 64, C = 1 at L = 3 and L = 4;
F = 128, C = 40 at L = 3.  Median of 30 after 5 warm-up passes (the restatement: 10 after 2 — it runs for a large part of a
second).  Prints one JSON line per shape; the two conditions the numbers are held to are evaluated and printed, not enforced."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import microbench as mb  # noqa: E402
from gnan_amd import _lib, functional  # noqa: E402

DEV = "cuda"
N, H = 1 << 18, 64
SHAPES = [(64, 1, 3), (64, 1, 4), (128, 40, 3)]          # (F, C, L)


def event_median(fn, reps, warm):
    """``fn(start, stop)`` records the two events around what it times; median over ``reps`` in ms."""
    times = []
    for i in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(a, b)
        torch.cuda.synchronize()
        if i >= warm:
            times.append(a.elapsed_time(b))
    return statistics.median(times)


def measure(F, C, L):
    torch.manual_seed(0)
    m = mb.TensorGNAN(F, C, L, hidden_channels=H, device=DEV)
    mb.redraw(m)
    m = m.to(DEV)
    st = mb.stack_mlps(m.fs)
    params = [q for q in st[:6] if q is not None]
    gen = torch.Generator(device=DEV).manual_seed(1)
    x0 = torch.rand(N, F, device=DEV, generator=gen) * 4 - 2
    gy = torch.randn(N, C, device=DEV, generator=gen)

    def backward(with_x, table_grads):
        def run(a, b):
            x = x0.clone().requires_grad_(True) if with_x else x0
            y = functional.feature_mlps(x, st, True)
            functional.HIP_TABLE_GRADS = table_grads
            a.record()
            torch.autograd.grad(y, params + ([x] if with_x else []), gy)
            b.record()
            functional.HIP_TABLE_GRADS = True
        return run

    out = {"what": "input_grad", "n": N, "F": F, "C": C, "L": L, "H": H}
    out["x_grad_ms"] = event_median(backward(True, True), 30, 5)
    out["params_only_ms"] = event_median(backward(False, True), 30, 5)
    out["restatement_ms"] = event_median(backward(True, False), 10, 2)
    # the two new launches on their own
    with torch.no_grad():
        _, tables, _ = functional._fmlp_forward(x0, st, True, False, True)
        raw = [None if q is None else q.detach() for q in st[:6]]
        dfdx = functional._piece_dfdx_launch(raw, tables, L, H, C, F)
        d = []
        functional._fpwl_input_grad(x0, tables, dfdx, gy, True, describe=d)

        def only(fn):
            def run(a, b):
                a.record()
                fn()
                b.record()
            return run
        out["dfdx_ms"] = event_median(only(lambda: functional._piece_dfdx_launch(raw, tables, L, H, C, F)), 30, 5)
        out["lookup_ms"] = event_median(only(lambda: functional._fpwl_input_grad(x0, tables, dfdx, gy, True)), 30, 5)
    out["pieces"] = int(tables.anchor.numel())
    out["plan"] = d[0]
    out["lookup_bytes"] = N * F * 8 + N * C * 4 + int(tables.anchor.numel()) * (1 + C) * 4 * d[0]["n_blocks"]
    out["lookup_GBps"] = out["lookup_bytes"] / out["lookup_ms"] / 1e6
    out["faster_than_restatement"] = out["x_grad_ms"] < out["restatement_ms"]
    out["under_twice_params_only"] = out["x_grad_ms"] < 2 * out["params_only_ms"]
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("input_grad_time.py measures on the GPU: no device visible")
    functional.FMLP_ALGO = _lib.FMLP_PWL
    for F, C, L in SHAPES:
        print(json.dumps(measure(F, C, L)), flush=True)
