#!/usr/bin/env python3
"""Forward and backward of ``functional.feature_mlps_dropout`` with MANY output channels (C = 40: the arxiv model of the
reference's run.sh; training-mode Dropout, p = 0.6, a fixed seed, sum_features) on one MI355X: the route of the commit before
the many-channel kernels (``gnan_fmlp_fwd`` lane kernel + the batched restatement's backward with drawn masks) against
``gnan_fmlp_mc_fwd`` + ``gnan_fmlp_mc_bwd``.  A sibling of tools/dropout_mfma_time.py (C <= 8), same protocol.

    python tools/dropout_mc_time.py                      one process, this tree: one JSON line per shape — HIP events around the
                                                         forward and around the backward (parameter gradients), median of 30
                                                         after 5 warm-ups.  On a tree that has the switches they are forced ON
                                                         at every size (the point is to measure what they would do)
    python tools/dropout_mc_time.py --tree PARENT        the same process on another checkout (its package, its built library):
                                                         a tree from before the feature has no switches and runs its own route
    python tools/dropout_mc_time.py --budget-s 8         stop sampling a shape once its samples took that many seconds (at least
                                                         three samples after one warm-up): the restatement's backward takes
                                                         seconds per sample at the full shape.  The line records the counts.
    python tools/dropout_mc_time.py --drive PARENT OUT   three fresh processes of PARENT's build (with --budget-s 8) and three of
                                                         this tree, alternating, on one box; every line is appended to OUT
                                                         (.jsonl), then one "verdict" line: the switches and the threshold

Shapes: the arxiv shape (169 343 x 129, H = 64, L = 3, C = 40) and a threshold sweep at F = 64, C = 40, n = 2^10 ... 2^18 by
powers of four.

The rule.  spread = the parent's max - min over its three processes' medians.  A pass (forward / backward)
ships on only if, at the arxiv shape, the new tree's slowest process beats the parent's fastest by more than that spread.
DROPOUT_MC_MIN_WORK = the smallest swept n * F from which on every shipped pass stays ahead in the same way, never below
functional.DROPOUT_MFMA_CLAMP."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SEED, H, L, C = 0.6, 20240607, 64, 3, 40
SAMPLES, WARM = 30, 5
SHAPES = [("arxiv", 169343, 129)] + [("sweep", 1 << e, 64) for e in (10, 12, 14, 16, 18)]
FULL = ("arxiv",)


def measure(tree, budget_s=None):
    sys.path.insert(0, tree)
    import torch
    import gnan_amd  # noqa: F401
    from gnan_amd import functional
    from gnan_amd.functional import StackedMLP, feature_mlps_dropout
    if not torch.cuda.is_available():
        sys.exit("dropout_mc_time.py measures on the GPU: no device visible")
    route = "parent"
    if hasattr(functional, "DROPOUT_MC"):
        functional.DROPOUT_MC = functional.DROPOUT_MC_BACKWARD = True
        functional.DROPOUT_MC_MIN_WORK = 1
        route = "mc"
    dev = "cuda"
    for name, n, F in SHAPES:
        gen = torch.Generator().manual_seed(F + C)
        t = lambda *s: (torch.randn(*s, generator=gen) * (2.0 / (s[-1] + s[-2])) ** 0.5).to(dev).requires_grad_(True)   # noqa: E731
        b = lambda *s: (torch.randn(*s, generator=gen) * 0.5).to(dev).requires_grad_(True)                              # noqa: E731
        leaves = [t(F, H, 1).squeeze(-1).detach().requires_grad_(True), b(F, H), t(1, F, H, H), b(1, F, H), t(F, C, H), b(F, C)]
        st = StackedMLP(*leaves, L, H, C, F)
        x = (torch.rand(n, F, generator=gen) * 2 - 0.5).to(dev)
        gup = torch.randn(n, C, generator=gen).to(dev)
        fwd, bwd = [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        warm = WARM
        began = time.monotonic()
        i = 0
        while len(fwd) < SAMPLES:
            ev[0].record()
            y = feature_mlps_dropout(x, st, True, P, seed=SEED)
            ev[1].record()
            torch.autograd.grad(y, leaves, gup)
            ev[2].record()
            torch.cuda.synchronize()
            if i >= warm:
                fwd.append(ev[0].elapsed_time(ev[1]))
                bwd.append(ev[1].elapsed_time(ev[2]))
            i += 1
            if budget_s is not None and time.monotonic() - began > budget_s:
                if i < warm:
                    warm = i                                    # (slow shape: the samples start after the calls already made)
                elif len(fwd) >= 3:
                    break
        print(json.dumps({"what": "dropout_mc_time", "route": route, "shape": name, "n": n, "F": F, "H": H, "L": L, "C": C, "p": P,
                          "sum_features": True, "work": n * F, "fwd_ms": statistics.median(fwd), "bwd_ms": statistics.median(bwd),
                          "fwd_min_ms": min(fwd), "bwd_min_ms": min(bwd), "samples": len(fwd), "warmups": warm,
                          "budget_s": budget_s}), flush=True)


def verdict(lines, clamp):
    """The rule of the module docstring over the drive's lines -> the verdict record."""
    def per(route, key):
        out = {}
        for r in lines:
            if r["route"] == route:
                out.setdefault((r["shape"], r["n"]), []).append(r[key])
        return out

    res = {"what": "dropout_mc_verdict", "clamp": clamp, "passes": {}}
    ahead_from = []
    for key, switch in (("fwd_ms", "DROPOUT_MC"), ("bwd_ms", "DROPOUT_MC_BACKWARD")):
        old, new = per("parent", key), per("mc", key)
        rows = {}
        for shape in old:
            spread = max(old[shape]) - min(old[shape])
            rows[shape] = {"parent_ms": sorted(old[shape]), "new_ms": sorted(new[shape]), "spread_ms": spread,
                           "ahead": max(new[shape]) < min(old[shape]) - spread}
        on = all(rows[s]["ahead"] for s in rows if s[0] in FULL)
        sweep = sorted((s for s in rows if s[0] == "sweep"), key=lambda s: s[1])
        first = None
        for i, s in enumerate(sweep):
            if all(rows[t]["ahead"] for t in sweep[i:]):
                first = s[1] * 64
                break
        res["passes"][switch] = {"on": on, "ahead_from_work": first, "shapes": {"%s:%d" % s: v for s, v in rows.items()}}
        if on:
            ahead_from.append(first)
    if ahead_from and all(a is not None for a in ahead_from):
        res["DROPOUT_MC_MIN_WORK"] = max(clamp, max(ahead_from))
    else:                                   # nothing ships on (or a shipped pass never stays ahead in the sweep)
        res["DROPOUT_MC_MIN_WORK"] = None if ahead_from else clamp
    return res


def drive(parent, out):
    lines = []
    with open(out, "a") as f:
        for proc in range(3):
            for tree in (parent, HERE):
                cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree] + (["--budget-s", "8"] if tree == parent else [])
                got = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if got.returncode != 0:
                    sys.exit("dropout_mc_time.py: process %d of %s ended with %d\n%s" % (proc, tree, got.returncode, got.stderr[-2000:]))
                for ln in got.stdout.splitlines():
                    if ln.startswith("{"):
                        r = json.loads(ln)
                        r["process"] = proc
                        lines.append(r)
                        f.write(json.dumps(r) + "\n")
                        f.flush()
                        print(json.dumps(r), flush=True)
        sys.path.insert(0, HERE)
        from gnan_amd import functional
        v = verdict(lines, functional.DROPOUT_MFMA_CLAMP)
        f.write(json.dumps(v) + "\n")
        print(json.dumps(v), flush=True)


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    if "--drive" in sys.argv:
        i = sys.argv.index("--drive")
        drive(os.path.abspath(sys.argv[i + 1]), sys.argv[i + 2])
    else:
        budget = float(sys.argv[sys.argv.index("--budget-s") + 1]) if "--budget-s" in sys.argv else None
        measure(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE, budget)
