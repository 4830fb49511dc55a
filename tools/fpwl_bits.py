#!/usr/bin/env python3
"""One SHA-1 per output of the table look-up kernels (csrc/fpwl*.hip) for a fixed list of small cases: run it with two builds of
the library (GNAN_HIP_LIB=/path/to/libgnan_hip.so) and compare the lines — a refactor of those kernels must leave every hash as it
was.  One process, a few seconds, no pytest; every input comes from seeded generators (tests/moments_ref.py builds the tables).

forward, n = 777 nodes (node blocks are at least 256 nodes: four blocks, a ragged last one and a ragged last pass):
  F in {16, 20, 64} x feature groups of 4, 8, 16, one channel: feature sum (kept pieces too where the kernel writes them), fp32
  rows with fused column sums over the first 700 rows, bf16 rows;  C = 3 and C = 40 with the feature sum (accumulators in LDS);
  a feature of 64, 65, 256, 257, 1024 pieces for the tree depths (the edge-* tables of tests/moments_ref.py).
moments: every tests/moments_ref.py case, raw bins (int64) or float moments, and its scales.  Lines that start with "~" are the
  float-bin cases with non-integer gradients: float LDS atomics, not reproducible run to run, so not to be compared.
locate: 262 144 nodes x 16 and x 17 features (the tree search's gate).   input gradient: C = 1 and C = 3.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gnan_amd  # noqa: E402,F401
import moments_ref as R  # noqa: E402
from gnan_amd import functional  # noqa: E402

DEV = "cuda"
N = 777


def sha(*tensors):
    h = hashlib.sha1()
    for t in tensors:
        if t is None:
            h.update(b"none")
            continue
        t = t.detach().contiguous().cpu()
        if t.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        h.update(str(tuple(t.shape)).encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


def tables(counts, C, fpg, seed):
    rng = np.random.default_rng(seed)
    ht = R.hand_tables(counts, rng)
    t = R.as_pwl(ht, C, np.random.default_rng(seed + 1), DEV, fpg)
    x = torch.from_numpy(R.draw_x(rng, "cover", ht, N)).to(DEV)
    return ht, t, x


def counts_for(F):
    return (R.MIX32 * 2 + R.MIX16)[:F]


def forward_cases():
    for F in (16, 20, 64):
        for fpg in (4, 8, 16):
            _, t, x = tables(counts_for(F), 1, fpg, 100 * F + fpg)
            tag = f"fwd F{F} fg{fpg}"
            located = []
            out = functional._fpwl_launch(x, t, True, located=located)
            yield f"{tag} sum", sha(out)
            yield f"{tag} sum pieces", sha(*located) if located else "none kept"
            out, total = functional._fpwl_launch(x, t, False, want_total=True, total_rows=700)
            yield f"{tag} rows", sha(out)
            yield f"{tag} rows column sums", sha(total) if total is not None else "no total (ragged groups)"
            if F % fpg == 0:
                out, total = functional._fpwl_launch(x, t, False, want_total=True, out_dtype=torch.bfloat16, total_rows=700)
                yield f"{tag} bf16 rows", sha(out)
                yield f"{tag} bf16 column sums", sha(total)
    for C, F, fpg in ((3, 16, 4), (3, 20, 2), (40, 8, 1), (40, 20, 1)):
        _, t, x = tables(counts_for(F), C, fpg, 1000 + 10 * C + F)
        yield f"fwd F{F} fg{fpg} C{C} sum", sha(functional._fpwl_launch(x, t, True))
        yield f"fwd F{F} fg{fpg} C{C} rows", sha(functional._fpwl_launch(x, t, False))
    for top in (64, 65, 256, 257, 1024):
        _, t, x = tables((top, 1, 2, 3) + (4,) * 12, 1, 16, 2000 + top)
        located = []
        yield f"fwd depth {top} sum", sha(functional._fpwl_launch(x, t, True, located=located))
        yield f"fwd depth {top} sum pieces", sha(*located) if located else "none kept"
        yield f"fwd depth {top} rows", sha(functional._fpwl_launch(x, t, False))


def moment_inputs(case):
    """The tables, x and gradient of a tests/moments_ref.py case, drawn as build_case draws them (without its exact references:
    they take minutes for all cases); column-offset views as launch_inputs makes them."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    ht = R.hand_tables(case.counts, rng, case.step, case.offset)
    x = R.draw_x(rng, case.xfam, ht, case.n)
    g = R.draw_g(rng, case.gfam, case.n, case.C if case.sum_features else ht.F * case.C)

    def put(a, shift):
        v = torch.from_numpy(a).to(DEV)
        if not shift:
            return v
        wide = torch.zeros((a.shape[0], a.shape[1] + 3), dtype=v.dtype, device=DEV)
        wide[:, 1:a.shape[1] + 1] = v
        return wide[:, 1:a.shape[1] + 1]
    return R.as_pwl(ht, case.C, np.random.default_rng(1), DEV, case.fpg or None), put(x, case.xshift), put(g, case.gshift)


def moment_cases():
    for case in R.CASES:
        functional.MOMENTS_GENERAL = case.general
        functional.MOMENTS_FIXED_POINT = case.fixed
        functional.FPWL_ROWS_MIN_NODES = case.rows_min or ROWS_MIN
        t, xd, gd = moment_inputs(case)
        rows = case.route.startswith("rows")
        located = None
        if case.kept:
            located = []
            functional._fpwl_launch(xd, t, case.sum_features if rows else True, located=located)
        elif case.stale_pieces:
            fg = t.features_per_group
            located = [torch.zeros(((xd.shape[1] + fg - 1) // fg, case.n, fg), dtype=torch.uint8, device=DEV)]
        d = []
        if case.fixed:
            M, scales = functional._fpwl_moments(xd, t, gd, case.sum_features, raw=True, located=located, describe=d)
            h = sha(M, scales)
        else:
            h = sha(functional._fpwl_moments(xd, t, gd, case.sum_features, located=located, describe=d))
            if case.gfam != "integers":     # float atomics: the sum depends on their order, two runs of ONE build differ
                h = "~" + h[1:]
        yield f"moments {case.name} [{R.KERNELS[d[0]['kernel']]}]", h
    functional.MOMENTS_GENERAL, functional.MOMENTS_FIXED_POINT, functional.FPWL_ROWS_MIN_NODES = False, True, ROWS_MIN


def locate_cases():
    for F in (16, 17):
        rng = np.random.default_rng(3000 + F)
        ht = R.hand_tables(counts_for(F), rng)
        t = R.as_pwl(ht, 4, np.random.default_rng(1), DEV, 4)
        x = torch.from_numpy(R.draw_x(rng, "uniform", ht, 262144)).to(DEV)
        piece, dx = functional._fpwl_locate(x, t, functional._fpwl_args(x, t, True))
        yield f"locate 262144 x {F}", sha(piece, dx)


def input_grad_cases():
    for C, fpg in ((1, 16), (1, 4), (3, 4), (3, 1)):
        for sum_features in (True, False):
            ht, t, x = tables(counts_for(20), C, fpg, 4000 + 10 * C + fpg)
            g = torch.from_numpy(np.random.default_rng(5).standard_normal((N, C if sum_features else 20 * C)).astype(np.float32)).to(DEV)
            dfdx = torch.from_numpy(np.random.default_rng(6).standard_normal((int(ht.off[-1]), C)).astype(np.float32)).to(DEV)
            yield f"input grad C{C} fg{fpg} {'sum' if sum_features else 'per'}", sha(functional._fpwl_input_grad(x, t, dfdx, g, sum_features))


if __name__ == "__main__":
    ROWS_MIN = functional.FPWL_ROWS_MIN_NODES
    functional.SUM_VIA_FEATURES_MAX_NODES = 0     # the feature sum over several channels inside the look-up, whatever the batch
    for cases in (forward_cases, moment_cases, locate_cases, input_grad_cases):
        for name, h in cases():
            print(f"{h}  {name}", flush=True)
    torch.cuda.synchronize()
