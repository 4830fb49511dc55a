"""Attributions by source node (``gnan_attr_cols``) restated in float64 with a DERIVED bound per element — TEST INFRASTRUCTURE
ONLY, in the manner of ``tests/attr_ref.py``.

The inputs are the kernel's own: the TRANSPOSED adjacency (CSR ``rowptr_t / row / code`` per source, or a dense ``code [n_src,
n_rows]``), ``S``, the weight table (shared ``[D, Cw]`` or per forward row ``[n_rows, D, Cw]``), the forward counts or none, the
requested rows (with repeats: ``mult[i]`` = how often row i occurs) and sources.

Truth        wt(i, d, c)  = lut[(i,) d, c] / max(cnt[i, d], 1)
             V[p, d, c]   = sum of mult[i_l] wt(i_l, d, c) over the pairs l of source j_p with min(code_l, D-1) == d, mult[i_l] > 0
             V[p, D-1, c] = T[c] - sum of mult[i_l] wt(i_l, D-1, c) over the pairs with code_l < D-1,     T[c] = sum_i mult[i] wt(i, D-1, c)
                                                                                                              (rest_from_total)
             B[p, d, w]   = V[p, d, w % Cw] S[j_p, w]
Magnitude    M[p, d, w]   = |S[j_p, w]| sum of |the terms of V|;   rest_from_total: the rest shell's terms are those of T and those
             of the listed sum, M = |S| (sum_i mult[i] |wt(i, D-1, c)| + sum over the listed pairs of mult |wt(i_l, D-1, c)|) — "|T|"
             is the magnitude of T's TERMS: T is formed inside the library in float32, its rounding error scales with them, not
             with the float64 value of T (which cancellation between rows of opposite sign can make arbitrarily small).
Bound        |got - B| <= gamma_k M,   gamma_k = k u / (1 - k u),   u = 2^-24

The count k, from the kernel's own roundings (csrc/attr_cols.hip).  A term mult * (lut / cnt) carries one rounding for the division
and one for the product with the multiplicity (none where it is fused into the addition; k is not lowered for that).  A sum of n
terms is formed in a fixed tree — a lane's running sum, the butterfly over the lanes, the chunks of the column (for T: a thread's
rows, the lanes, the waves, the blocks).  Every accumulator starts at +0, 0 + x and x + 0 are exact, and every other addition on a
term's way to the root merges disjoint groups that hold at least one term each: at most n - 1 rounded additions, whatever the
tree.  The product with S adds one: k = 2 + (n - 1) + 1 = n + 2.  n == 0: V is exactly +0, M == 0 and the output must be exactly 0.
The rest shell under rest_from_total: T with n_T terms (the distinct requested rows) and the listed sum with n' terms each carry
at most max(n_T, n') + 1 roundings per term, the subtraction one, the product one: k = max(n_T, n') + 3.
Where the bound is 0 the output must be exactly 0; no element is left out of the comparison.
"""
import numpy as np
import torch

from attr_ref import _idx, _t64, gamma


def reference(code, S, lut, rowptr_t=None, row=None, cnt=None, rows=None, cols=None, rest_from_total=False, n_rows=None):
    """``(truth, bound, magnitude)``, float64 numpy ``[P, D, W]``.  ``rowptr_t is None``: ``code`` is the dense ``[n_src, n_rows]``
    matrix (forward row = column index); else the transposed CSR's.  ``rows``: the requested rows (default: all ``n_rows``, once);
    ``cols``: the requested sources, in order (default: all)."""
    code = _idx(code)
    S, lut = _t64(S), _t64(lut)
    dense = rowptr_t is None
    if dense:
        n_rows = code.shape[1]
    else:
        rowptr_t, row = _idx(rowptr_t), _idx(row)
    n_src = code.shape[0] if dense else rowptr_t.numel() - 1
    cols = torch.arange(n_src) if cols is None else _idx(cols).reshape(-1)
    mult = torch.ones(n_rows, dtype=torch.float64) if rows is None else \
        torch.bincount(_idx(rows).reshape(-1), minlength=n_rows).double()
    D, Cw = lut.shape[-2], lut.shape[-1]
    W = S.shape[1]
    ch = torch.arange(W) % Cw
    wt = (lut if lut.dim() == 3 else lut.unsqueeze(0).expand(n_rows, -1, -1)).clone()          # [n_rows, D, Cw]
    if cnt is not None:
        wt = wt / _idx(cnt)[:, :D].clamp_min(1).double().unsqueeze(-1)
    T = (mult.unsqueeze(-1) * wt[:, D - 1]).sum(0)                                             # [Cw]
    Ta = (mult.unsqueeze(-1) * wt[:, D - 1].abs()).sum(0)
    nT = float((mult > 0).sum())
    P = cols.numel()
    truth, mag, k = np.zeros((P, D, W)), np.zeros((P, D, W)), np.zeros((P, D))
    for p, j in enumerate(cols.tolist()):
        if dense:
            pr, pd = torch.arange(n_rows), code[j]
        else:
            lo, hi = int(rowptr_t[j]), int(rowptr_t[j + 1])
            pr, pd = row[lo:hi], code[lo:hi]
        keep = mult[pr] > 0
        if rest_from_total:
            keep = keep & (pd < D - 1)
        pr, pd = pr[keep], pd[keep].clamp_max(D - 1)
        m = mult[pr].unsqueeze(-1)
        V = torch.zeros((D, Cw), dtype=torch.float64).index_add_(0, pd, m * wt[pr, pd])
        Va = torch.zeros((D, Cw), dtype=torch.float64).index_add_(0, pd, m * wt[pr, pd].abs())
        n = torch.bincount(pd, minlength=D).double()
        kp = n + 2.0
        if rest_from_total:
            V[D - 1] = T - (m * wt[pr, D - 1]).sum(0)
            Va[D - 1] = Ta + (m * wt[pr, D - 1].abs()).sum(0)
            kp[D - 1] = max(nT, float(pr.numel())) + 3.0
        truth[p] = (V[:, ch] * S[j].unsqueeze(0)).numpy()
        mag[p] = (Va[:, ch] * S[j].abs().unsqueeze(0)).numpy()
        k[p] = kp.numpy()
    return truth, gamma(k)[:, :, None] * mag, mag


# ---------------------------------------------------------------------------------------------
# model level: interpret.explain_sources restated densely in float64, straight from node_distances / normalization_matrix
# (SURVEY.md Appendix A.1-A.3), by source node.  No hop code is formed: a pair belongs to distance d because its node_distances
# entry EQUALS float32(1 / (1 + d)), to the rest because the entry is 0 — as attr_ref.explain_restatement.
# ---------------------------------------------------------------------------------------------
def explain_sources_restatement(kind, x, nd, norm, params, normalize_rho, n_dist, rows=None, sources=None):
    """``[P, F, n_dist, C]`` float64: ``f_k(x[j, k])[c] * sum over the requested rows i (with repeats) at distance d from j of
    m[i, j, c]``.  ``kind`` as in ``attr_ref.explain_restatement``."""
    from oracle import gnan_oracle as O
    x64, nd64 = x.detach().cpu().double(), nd.detach().cpu().double()
    p64 = {k: v.detach().cpu().double() for k, v in params.items()}
    fx = O.feature_mlps(x64, p64)                                             # [N, F, C]
    n = x64.shape[0]
    rho = O.mlp_layers(p64, "rho")
    if kind == "standalone_tensor":
        u = nd64 / norm.detach().cpu().double() if normalize_rho else nd64
        m = O.mlp_apply(rho, u.reshape(-1, 1)).reshape(n, n, -1)
    else:
        m = O.mlp_apply(rho, nd64.reshape(-1, 1)).reshape(n, n, -1)
        if normalize_rho:
            m = m / norm.detach().cpu().double().unsqueeze(-1)
    ids = torch.arange(n) if rows is None else torch.as_tensor(rows).long().reshape(-1)
    src = torch.arange(n) if sources is None else torch.as_tensor(sources).long().reshape(-1)
    nd32 = nd.detach().cpu().float()
    m = m.expand(-1, -1, fx.shape[2])
    out = torch.zeros((src.numel(), fx.shape[1], n_dist, fx.shape[2]), dtype=torch.float64)
    for d in range(n_dist):
        value = np.float32(0.0) if d == n_dist - 1 else np.float32(1.0) / (np.float32(d) + np.float32(1.0))
        mask = (nd32[ids][:, src] == float(value)).double().unsqueeze(-1)     # [R, P, 1]
        v = (m[ids][:, src] * mask).sum(0)                                    # [P, C]: the rows, repeats included
        out[:, :, d, :] = v.unsqueeze(1) * fx[src]
    return out
