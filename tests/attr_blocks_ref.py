"""Attributions of a batch of graphs (``gnan_attr_blocks``) restated in float64 with a DERIVED bound per element — TEST
INFRASTRUCTURE ONLY, in the manner of ``tests/attr_cols_ref.py``.

The inputs are the kernel's own: the packed ``[n_g, n_g]`` code blocks (entry (i, j): the hop at which row i sees node j), the
graphs' sizes, ``S [N, W]``, the weight table (shared ``[D, Cw]`` or per forward row ``[N, D, Cw]``) and the counts ``[N, D]`` or none.

Truth        wt(i, d, c) = lut[(i,) d, c] / max(cnt[i, d], 1)
             V[j, d, c]  = sum of wt(i, d, c) over the nodes i of j's graph with min(code_g[i, j], D-1) == d
             B[j, d, w]  = V[j, d, w % Cw] S[j, w]             T[g, d, w] = sum over the nodes j of graph g of B[j, d, w]
Magnitude    M[j, d, w]  = |S[j, w]| sum of |wt| over the same nodes;   for T: the sum of M over the graph's nodes
Bound        |got - truth| <= gamma_k magnitude,   gamma_k = k u / (1 - k u),   u = 2^-24

The count k, from the kernel's own roundings (csrc/attr_blocks.hip).  A term lut / cnt carries one rounding (the division; none
without counts, k is not lowered for that).  The n terms of V[j, d, c] are added in a fixed tree — a lane's running sum over the
rows of its row slice, then the four slices as (s0 + s1) + (s2 + s3).  Every accumulator starts at +0, 0 + x and x + 0 are exact,
and every other addition on a term's way to the root merges disjoint groups that hold at least one term each: at most n - 1
rounded additions.  The product with S adds one: k_B = 1 + (n - 1) + 1 = n + 1.  n == 0: V is exactly +0, M == 0 and B must be
exactly 0.  T adds the products of the graph's n_g nodes in node order from +0: a term carries its own k_B and at most n_g - 1
further additions (where the compiler fuses product and addition the product's rounding goes away; k is not lowered for that):
k_T[g, d] = max over the graph's nodes of k_B[j, d] + (n_g - 1).  An empty graph, or a shell no pair of the graph falls into: the
magnitude is 0 and T must be exactly 0.  No element is left out of the comparison.
"""
import numpy as np
import torch

from attr_ref import _idx, _t64, gamma


def reference(code, sizes, S, lut, cnt=None):
    """``(B, bound_B, T, bound_T)``, float64 numpy ``[N, D, W]`` / ``[G, D, W]``."""
    code = _idx(code).reshape(-1)
    S, lut = _t64(S), _t64(lut)
    sizes = [int(s) for s in sizes]
    N, G = sum(sizes), len(sizes)
    D, Cw = lut.shape[-2], lut.shape[-1]
    W = S.shape[1]
    ch = torch.arange(W) % Cw
    wt = (lut if lut.dim() == 3 else lut.unsqueeze(0).expand(N, -1, -1)).clone()               # [N, D, Cw]
    if cnt is not None:
        wt = wt / _idx(cnt)[:, :D].clamp_min(1).double().unsqueeze(-1)
    B, MB, kB = np.zeros((N, D, W)), np.zeros((N, D, W)), np.zeros((N, D))
    T, MT, kT = np.zeros((G, D, W)), np.zeros((G, D, W)), np.zeros((G, D))
    n0 = c0 = 0
    for g, n in enumerate(sizes):
        if n:
            shell = code[c0: c0 + n * n].view(n, n).clamp_max(D - 1)                           # [i, j]
            i = torch.arange(n).repeat_interleave(n)
            j = torch.arange(n).repeat(n)
            d = shell.reshape(-1)
            w = wt[n0 + i, d]                                                                  # [n * n, Cw]
            V = torch.zeros((n * D, Cw), dtype=torch.float64).index_add_(0, j * D + d, w).view(n, D, Cw)
            Va = torch.zeros((n * D, Cw), dtype=torch.float64).index_add_(0, j * D + d, w.abs()).view(n, D, Cw)
            terms = torch.bincount(j * D + d, minlength=n * D).view(n, D).double()
            Sg = S[n0: n0 + n]
            B[n0: n0 + n] = (V[:, :, ch] * Sg.unsqueeze(1)).numpy()
            MB[n0: n0 + n] = (Va[:, :, ch] * Sg.abs().unsqueeze(1)).numpy()
            kB[n0: n0 + n] = (terms + 1.0).numpy()
            T[g] = B[n0: n0 + n].sum(0)
            MT[g] = MB[n0: n0 + n].sum(0)
            kT[g] = kB[n0: n0 + n].max(0) + (n - 1)
        n0, c0 = n0 + n, c0 + n * n
    return B, gamma(kB)[:, :, None] * MB, T, gamma(kT)[:, :, None] * MT
