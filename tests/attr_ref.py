"""Per-row attributions (``gnan_attr_rows``) restated in float64 with a DERIVED bound per element — TEST INFRASTRUCTURE ONLY,
in the manner of ``tests/rowwise.py``.

The inputs are the kernel's own: the adjacency (CSR ``rowptr / col / code`` or a dense ``code [n_rows, n_cols]``), ``S``, the
weight table (shared ``[D, Cw]`` or per-row ``[n, D, Cw]``), the counts or none, and the float32 ``s_total`` handed to the launch.

Truth        Z[q, d, w]   = sum of S[col_l, w] over the pairs l of row i_q with min(code_l, D-1) == d
             Z[q, D-1, w] = s_total[w] - sum over the pairs with code_l < D-1 of S[col_l, w]              (s_total given)
             A[q, d, w]   = w(i_q, d, w % Cw) Z[q, d, w],        w = lut / max(cnt, 1)
Magnitude    M[q, d, w]   = |w| sum over the shell's pairs of |S[col_l, w]|
             M[q, D-1, w] = |w| (|s_total[w]| + sum over the pairs with code_l < D-1 of |S|)               (s_total given)
Bound        |got - A| <= gamma_k M,   gamma_k = k u / (1 - k u),   u = 2^-24

The count k, from the kernel's roundings (csrc/attr_rows.hip).  A shell with m pairs is summed in a fixed tree: a stream's
running sum, the slots of a wave, the four waves, the row's chunks.  Every accumulator starts at +0 and 0 + x is exact, as is
x + 0 for a stream, slot, wave or chunk that holds no pair of the shell; every other addition on a term's way to the root merges
a disjoint group that holds at least one pair.  So a term passes at most m - 1 rounded additions, whatever the tree: gamma_{m-1}
on the sum.  The weight adds one rounding for the division lut / cnt and one for the product: k = m + 1.  (Without counts the
division is absent; k is not lowered for that.)  m == 0: the sum is exactly +0, M == 0 and the output must be exactly 0.
The rest shell with s_total: the listed sum over the m' pairs coded below D - 1 is the shells' sums added in shell order — the
same argument, gamma_{m'-1} — then one rounding for the subtraction, one for the division, one for the product: k = m' + 2
(m' == 0: the listed sum is exactly 0 and the subtraction exact; 2 roundings remain).
Where the bound is 0 the output must be exactly 0; no element is left out of the comparison.
"""
import numpy as np
import torch

U = 2.0 ** -24


def _t64(v):
    if torch.is_tensor(v):
        return v.detach().cpu().double()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)))


def _idx(v):
    if torch.is_tensor(v):
        return v.detach().cpu().long()
    return torch.from_numpy(np.asarray(v).astype(np.int64))


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def reference(code, S, lut, rowptr=None, col=None, cnt=None, s_total=None, rows=None):
    """``(truth, bound, magnitude)``, float64 numpy ``[R, D, W]``.  ``rowptr is None``: ``code`` is the dense ``[n_rows, n_cols]``
    matrix (neighbour = column); else the CSR's.  ``rows``: the requested rows, in order (default: all)."""
    code = _idx(code)
    S, lut = _t64(S), _t64(lut)
    dense = rowptr is None
    if not dense:
        rowptr, col = _idx(rowptr), _idx(col)
    n_all = code.shape[0] if dense else rowptr.numel() - 1
    rows = torch.arange(n_all) if rows is None else _idx(rows).reshape(-1)
    D, Cw = lut.shape[-2], lut.shape[-1]
    W = S.shape[1]
    ch = torch.arange(W) % Cw
    tot = None if s_total is None else _t64(s_total).reshape(-1)
    cnt = None if cnt is None else _idx(cnt)
    R = rows.numel()
    truth = np.zeros((R, D, W))
    mag = np.zeros((R, D, W))
    k = np.zeros((R, D))
    for q, i in enumerate(rows.tolist()):
        if dense:
            pc, pd = torch.arange(code.shape[1]), code[i]
        else:
            lo, hi = int(rowptr[i]), int(rowptr[i + 1])
            pc, pd = col[lo:hi], code[lo:hi]
        pd = pd.clamp_max(D - 1)
        Z = torch.zeros((D, W), dtype=torch.float64).index_add_(0, pd, S[pc])
        Za = torch.zeros((D, W), dtype=torch.float64).index_add_(0, pd, S[pc].abs())
        m = torch.bincount(pd, minlength=D).double()
        kq = m + 1.0
        if tot is not None:
            Z[D - 1] = tot - Z[: D - 1].sum(0)
            Za[D - 1] = tot.abs() + Za[: D - 1].sum(0)
            kq[D - 1] = m[: D - 1].sum() + 2.0
        w = (lut[i] if lut.dim() == 3 else lut)[:, ch]                        # [D, W]
        if cnt is not None:
            w = w / cnt[i, :D].clamp_min(1).double().unsqueeze(1)
        truth[q], mag[q], k[q] = (w * Z).numpy(), (w.abs() * Za).numpy(), kq.numpy()
    return truth, gamma(k)[:, :, None] * mag, mag


def violations(got, truth, bound):
    """Indices of the elements of ``got`` outside the bound (every element is judged; a non-finite value is a violation)."""
    g = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    g = g.reshape(truth.shape)
    bad = ~np.isfinite(g) | ~(np.abs(g - truth) <= bound)
    return np.argwhere(bad)


def check(got, truth, bound, what=""):
    bad = violations(got, truth, bound)
    if len(bad):
        q, d, w = bad[0]
        g = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
        g = g.reshape(truth.shape)
        raise AssertionError(f"{what}: {len(bad)} of {truth.size} elements outside their bound; first [{q}, {d}, {w}]: got "
                             f"{g[q, d, w]!r}, truth {truth[q, d, w]!r}, |diff| {abs(g[q, d, w] - truth[q, d, w]):.3e} > "
                             f"bound {bound[q, d, w]:.3e}")


# ---------------------------------------------------------------------------------------------
# model level: interpret.explain restated densely in float64, straight from node_distances / normalization_matrix
# (SURVEY.md Appendix A.1-A.3).  No hop code is formed: a pair belongs to distance d because its node_distances entry EQUALS
# float32(1 / (1 + d)), to the rest because the entry is 0 — so the hop coding itself is under test.
# ---------------------------------------------------------------------------------------------
def explain_restatement(kind, x, nd, norm, params, normalize_rho, n_dist, rows=None):
    """``[R, F, n_dist, C]`` float64: ``sum over the nodes j at distance d of row i of m[i, j, c] f_k(x[j, k])[c]``.
    ``kind``: "standalone_tensor" (rho of the normalised distance, GNAN.py:65-67) or "post" (rho of the distance, divided by
    the normalisation matrix: models.py:368-370 and GNAN.forward, GNAN.py:162-168)."""
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
    nd32 = nd.detach().cpu().float()
    out = torch.zeros((ids.numel(), fx.shape[1], n_dist, fx.shape[2]), dtype=torch.float64)
    for d in range(n_dist):
        value = np.float32(0.0) if d == n_dist - 1 else np.float32(1.0) / (np.float32(d) + np.float32(1.0))
        mask = (nd32[ids] == float(value)).double().unsqueeze(-1)             # [R, N, 1]
        out[:, :, d, :] = torch.einsum("ijc,jkc->ikc", (m[ids] * mask).expand(-1, -1, fx.shape[2]), fx)
    return out
