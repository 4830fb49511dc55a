#!/usr/bin/env python3
"""Forward and backward of ``functional.feature_mlps_dropout`` (training-mode Dropout, p = 0.6, a fixed seed) on one MI355X:
the lane route (``gnan_fmlp_fwd`` lane kernel + ``gnan_fmlp_bwd``) against the matrix-core route (``GNAN_FMLP_MFMA`` under
Dropout + ``gnan_fmlp_bwd_mfma``).

    python tools/dropout_mfma_time.py                      one process, this tree: one JSON line per shape — HIP events around
                                                           the forward and around the backward (parameter gradients), median
                                                           of 30 after 5 warm-ups.  On a tree that has the switches they are
                                                           forced ON at every size (the point is to measure what they would do)
    python tools/dropout_mfma_time.py --tree PARENT        the same process on another checkout (its package, its built library):
                                                           a tree from before the feature has no switches and runs its lane route
    python tools/dropout_mfma_time.py --drive PARENT OUT   three fresh processes of PARENT's build and three of this tree,
                                                           alternating, on one box; every line is appended to OUT (.jsonl), then
                                                           one "verdict" line: the switches and the threshold by the rule below

Shapes: the arxiv shape (169 343 x 129, H = 64, L = 3, C = 1), the Cora shape (2 708 x 1 434, C = 7) and a threshold sweep at
F = 64, C = 1, n = 2^10 ... 2^18 by powers of four.

The rule.  spread = the parent's max - min over its three processes' medians.  A pass (forward / backward)
is switched on only if, at BOTH full shapes, the new tree's slowest process beats the parent's fastest by more than that spread.
DROPOUT_MFMA_MIN_WORK = the smallest swept n * F from which on every switched-on pass stays ahead in the same way, never below
functional.DROPOUT_MFMA_CLAMP."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, SEED, H, L = 0.6, 20240607, 64, 3
SAMPLES, WARM = 30, 5
SHAPES = [("arxiv", 169343, 129, 1), ("cora", 2708, 1434, 7)] + [("sweep", 1 << e, 64, 1) for e in (10, 12, 14, 16, 18)]
FULL = ("arxiv", "cora")


def measure(tree):
    sys.path.insert(0, tree)
    import torch
    import gnan_amd  # noqa: F401
    from gnan_amd import functional
    from gnan_amd.functional import StackedMLP, feature_mlps_dropout
    if not torch.cuda.is_available():
        sys.exit("dropout_mfma_time.py measures on the GPU: no device visible")
    route = "lane"
    if hasattr(functional, "DROPOUT_MFMA"):
        functional.DROPOUT_MFMA = functional.DROPOUT_MFMA_BACKWARD = True
        functional.DROPOUT_MFMA_MIN_WORK = 1
        route = "mfma"
    dev = "cuda"
    for name, n, F, C in SHAPES:
        gen = torch.Generator().manual_seed(F + C)
        t = lambda *s: (torch.randn(*s, generator=gen) * (2.0 / (s[-1] + s[-2])) ** 0.5).to(dev).requires_grad_(True)   # noqa: E731
        b = lambda *s: (torch.randn(*s, generator=gen) * 0.5).to(dev).requires_grad_(True)                              # noqa: E731
        leaves = [t(F, H, 1).squeeze(-1).detach().requires_grad_(True), b(F, H), t(1, F, H, H), b(1, F, H), t(F, C, H), b(F, C)]
        st = StackedMLP(*leaves, L, H, C, F)
        x = (torch.rand(n, F, generator=gen) * 2 - 0.5).to(dev)
        gup = torch.randn(n, F * C, generator=gen).to(dev)
        fwd, bwd = [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for i in range(WARM + SAMPLES):
            ev[0].record()
            y = feature_mlps_dropout(x, st, False, P, seed=SEED)
            ev[1].record()
            torch.autograd.grad(y, leaves, gup)
            ev[2].record()
            torch.cuda.synchronize()
            if i >= WARM:
                fwd.append(ev[0].elapsed_time(ev[1]))
                bwd.append(ev[1].elapsed_time(ev[2]))
        print(json.dumps({"what": "dropout_mfma_time", "route": route, "shape": name, "n": n, "F": F, "H": H, "L": L, "C": C, "p": P,
                          "work": n * F, "fwd_ms": statistics.median(fwd), "bwd_ms": statistics.median(bwd),
                          "fwd_min_ms": min(fwd), "bwd_min_ms": min(bwd), "samples": SAMPLES, "warmups": WARM}), flush=True)


def verdict(lines, clamp):
    """The rule of the module docstring over the drive's lines -> the verdict record."""
    def per(route, key):
        out = {}
        for r in lines:
            if r["route"] == route:
                out.setdefault((r["shape"], r["n"]), []).append(r[key])
        return out

    res = {"what": "dropout_mfma_verdict", "clamp": clamp, "passes": {}}
    ahead_from = []
    for key, switch in (("fwd_ms", "DROPOUT_MFMA"), ("bwd_ms", "DROPOUT_MFMA_BACKWARD")):
        old, new = per("lane", key), per("mfma", key)
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
        res["passes"][switch] = {"on": on, "ahead_from_work": first,
                                 "shapes": {"%s:%d" % s: v for s, v in rows.items()}}
        if on:
            ahead_from.append(first)
    if ahead_from and all(a is not None for a in ahead_from):
        res["DROPOUT_MFMA_MIN_WORK"] = max(clamp, max(ahead_from))
    else:                                   # nothing switched on (or a switched-on pass never stays ahead in the sweep)
        res["DROPOUT_MFMA_MIN_WORK"] = None if ahead_from else clamp
    return res


def drive(parent, out):
    lines = []
    with open(out, "a") as f:
        for proc in range(3):
            for tree in (parent, HERE):
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree], capture_output=True, text=True,
                                     timeout=600)
                if got.returncode != 0:
                    sys.exit("dropout_mfma_time.py: process %d of %s ended with %d\n%s" % (proc, tree, got.returncode, got.stderr[-2000:]))
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
        measure(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else HERE)
