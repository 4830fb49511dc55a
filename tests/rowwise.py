"""The wide aggregation restated in float64 with a DERIVED bound per output element — TEST INFRASTRUCTURE ONLY.

``helpers.rule`` compares against the largest entry of the whole result, so an error confined to one short row hides under the
hub rows.  Here every element is judged against its own row's magnitude.  The inputs are the kernel's: CSR, codes, ``S``,
the weight table (shared ``[D, Cw]`` or per-row ``[n, D, Cw]``), the counts or none, and the float32 ``s_total`` actually
handed to the launch (so the column-sum kernel's own error is an input, not part of what is judged).

Truth        t[i, c] = sum_l w(i, d_l) S[j_l, c] + w(i, rest) (tot[c] - sum_l S[j_l, c]),      w = lut / max(cnt, 1)
             (listed codes >= D - 1 are clipped to the rest code, as the kernel does; without ``s_total``: the first sum alone)
Magnitude    A[i, c] = sum_l |w(i, d_l)| |S[j_l, c]| + |w(i, rest)| (sum_l |S[j_l, c]| + |tot[c]|)
Bound        |y - t| <= gamma_k A,   gamma_k = k u / (1 - k u),   u = 2^-24,   k = L_i + 5
             the 5: one division, the fold w_d - w_rest (inherits two roundings, adds one), the final fmaf; the L: the fmaf
             chain over the row's pairs.  Rows above the hub threshold: k = 2 L_i (slice partials and the fix-up add at most
             one rounding per slice, and a row has no more slices than pairs).
Fused read-out   channel c' collects the columns c = c' (mod cr):  gamma_{k + 10} sum_c A[i, c]  (at most 4 adds within a
             lane, 6 butterfly steps).
Where the bound is 0 the output must be exactly 0; no element is left out of the comparison.
"""
import numpy as np
import torch

U = 2.0 ** -24
HUB_THRESHOLD = 512          # graph.LONG_ROW_THRESHOLD (tests/test_rowwise_bound.py holds the two equal): rows with more pairs are cut into slices


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


def reference(rowptr, col, code, S, lut, cnt=None, s_total=None, reduce_cr=0, hub_threshold=HUB_THRESHOLD, rows=None):
    """``(truth, bound)``, float64 numpy ``[n, W]`` (``[n, reduce_cr]`` with the fused read-out).  ``S`` as the kernel reads it
    (a bf16 operand: its values widened); ``cnt`` None: no shell normalisation; ``s_total`` None: no rest term.
    ``rows``: evaluate these rows only (row ``q`` of the result is row ``rows[q]`` of the graph)."""
    rowptr, col, code = _idx(rowptr), _idx(col), _idx(code)
    S, lut = _t64(S), _t64(lut)
    n_all = rowptr.numel() - 1
    rows = torch.arange(n_all) if rows is None else _idx(rows)
    n, W = rows.numel(), S.shape[1]
    D, Cw = lut.shape[-2], lut.shape[-1]
    rest = D - 1
    wt = lut[rows] if lut.dim() == 3 else lut.unsqueeze(0).expand(n, D, Cw)
    if cnt is not None:
        wt = wt / _idx(cnt)[rows].clamp_min(1).double().unsqueeze(-1)
    lo, deg = rowptr[rows], rowptr[rows + 1] - rowptr[rows]
    out_of_pair = torch.repeat_interleave(torch.arange(n), deg)
    pair = torch.repeat_interleave(lo - (torch.cumsum(deg, 0) - deg), deg) + torch.arange(int(deg.sum()))
    pc, pd = col[pair], code[pair].clamp_max(rest)
    tot = None if s_total is None else _t64(s_total).reshape(-1)
    truth = torch.empty((n, W), dtype=torch.float64)
    mag = torch.empty((n, W), dtype=torch.float64)
    step = max(1, min(W, (1 << 22) // max(1, pair.numel())))          # columns per pass: bounds the [pairs, columns] temporaries
    for c0 in range(0, W, step):
        cs = torch.arange(c0, min(W, c0 + step))
        ch = cs % Cw
        w = wt[out_of_pair, pd][:, ch]                               # [pairs, columns]
        s = S[pc][:, cs]
        zero = torch.zeros((n, cs.numel()), dtype=torch.float64)
        t = zero.clone().index_add_(0, out_of_pair, w * s)
        a = zero.clone().index_add_(0, out_of_pair, w.abs() * s.abs())
        if tot is not None:
            wr = wt[:, rest][:, ch]
            t = t + wr * (tot[cs].unsqueeze(0) - zero.clone().index_add_(0, out_of_pair, s))
            a = a + wr.abs() * (zero.clone().index_add_(0, out_of_pair, s.abs()) + tot[cs].abs().unsqueeze(0))
        truth[:, c0:c0 + cs.numel()], mag[:, c0:c0 + cs.numel()] = t, a
    k = torch.where(deg > hub_threshold, 2 * deg, deg + 5).double().numpy()
    truth, mag = truth.numpy(), mag.numpy()
    if reduce_cr:
        truth = truth.reshape(n, W // reduce_cr, reduce_cr).sum(1)
        mag = mag.reshape(n, W // reduce_cr, reduce_cr).sum(1)
        k = k + 10
    return truth, gamma(k)[:, None] * mag


def worst_ratio(y, truth, bound):
    """Largest ``|y - t| / bound`` over the elements with a positive bound (inf when any element — one with a zero bound, which must
    be exactly zero, included — fails or is not finite)."""
    y = _t64(y).numpy().reshape(truth.shape)
    err = np.abs(y - truth)
    if not bool(np.all(err <= bound)):              # (a NaN compares false)
        return float("inf")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def assert_within(y, truth, bound, what=""):
    """Every element within its bound; returns the worst ratio."""
    yv = _t64(y).numpy().reshape(truth.shape)
    err = np.abs(yv - truth)
    bad = ~(err <= bound)
    if bad.any():
        i, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the per-row bound; first at row {i}, column {c}: "
                             f"got {yv[i, c]!r}, truth {truth[i, c]!r}, |err| {err[i, c]:.3e} > bound {bound[i, c]:.3e}")
    return worst_ratio(y, truth, bound)


def exact_scaled(rowptr, col, code, S, lut, s_total=None, reduce_cr=0, cnt=None, scale=4):
    """The same sum for integer ``S`` and weights ``lut / max(cnt, 1)`` that are multiples of ``1 / scale`` (a power of two), in int64:
    ``(scale t, scale A)`` with ``A`` the magnitude above.  While ``scale A < 2^24`` every product and every partial sum of the float32
    evaluation is a multiple of ``1 / scale`` below ``2^24 / scale``, hence exact in any order: the output must equal ``t``."""
    rowptr, col, code = _idx(rowptr), _idx(col), _idx(code)
    S = _t64(S)
    n, W = rowptr.numel() - 1, S.shape[1]
    lut = _t64(lut).reshape(1, -1)
    rest = lut.shape[1] - 1
    w = lut.expand(n, rest + 1) * scale
    if cnt is not None:
        w = w / _idx(cnt).clamp_min(1).double()
    assert bool((S == S.round()).all()) and bool((w == w.round()).all())
    S, w = S.long(), w.long()
    deg = rowptr[1:] - rowptr[:-1]
    row_of_pair = torch.repeat_interleave(torch.arange(n), deg)
    wp, s = w[row_of_pair, code.clamp_max(rest)].unsqueeze(1), S[col]
    zero = torch.zeros((n, W), dtype=torch.int64)
    t = zero.clone().index_add_(0, row_of_pair, wp * s)
    a = zero.clone().index_add_(0, row_of_pair, wp.abs() * s.abs())
    if s_total is not None:
        tot = _t64(s_total).reshape(-1)
        assert bool((tot == tot.round()).all())
        tot, wr = tot.long(), w[:, rest:rest + 1]
        t = t + wr * (tot.unsqueeze(0) - zero.clone().index_add_(0, row_of_pair, s))
        a = a + wr.abs() * (zero.clone().index_add_(0, row_of_pair, s.abs()) + tot.abs().unsqueeze(0))
    if reduce_cr:
        t, a = t.view(n, W // reduce_cr, reduce_cr).sum(1), a.view(n, W // reduce_cr, reduce_cr).sum(1)
    return t, a


def exact_quarters(rowptr, col, code, S, lut, s_total=None, reduce_cr=0):
    """:func:`exact_scaled` for weights that are multiples of 1/4 and no counts: ``(4 t, 4 A)``."""
    return exact_scaled(rowptr, col, code, S, lut, s_total, reduce_cr, None, 4)


def short_csr(n, rng, D=4, hubs=((7, 600), (1234, 2000), (-1, 513)), self_share=0.8):
    """The degree mix of tests/test_gpu_short_tiles.py for any code count: rows of 0 .. 9 pairs and a few of 30, ``hubs`` =
    (row, pairs); most rows of 1 .. 4 pairs list themselves first (code 0), some do not; the other codes are 1 .. D - 2
    (D = 2: code 0 throughout)."""
    deg = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], size=n, p=[.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])
    for r, d in hubs:
        deg[r] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n, nnz).astype(np.int32)
    code = (rng.integers(1, D - 1, nnz) if D > 2 else np.zeros(nnz)).astype(np.uint8)
    for i in np.nonzero((deg > 0) & (deg <= 4) & (rng.random(n) < self_share))[0]:
        col[rowptr[i]], code[rowptr[i]] = i, 0
    return rowptr, col, code


def csr_of_degrees(deg, n_cols, rng, D=4):
    """A CSR with exactly these row lengths, random neighbours and codes 0 .. D - 2."""
    deg = np.asarray(deg, dtype=np.int64)
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    return rowptr, rng.integers(0, n_cols, nnz).astype(np.int32), rng.integers(0, max(D - 1, 1), nnz).astype(np.uint8)


def lanes_per_row(W, vec=4):
    """The lane group of a row of W floats read ``vec`` at a time: the smallest power of two covering it, at most a wavefront."""
    lpr = 1
    while lpr * vec < W and lpr < 64:
        lpr *= 2
    return lpr


def tile_partition(deg, lpr, lmax):
    """The short-row tiles of a degree-sorted copy with these row lengths, restated: run L = the rows of exactly L pairs, a lane
    group takes R_L rows of it (R_0 = 8, R_L = max(1, 8 // L)), a wave 64 / lpr groups, one tile per wave.
    ``(n_tiles, row_q0, first tile of every run)``."""
    deg = np.asarray(deg)
    first, t = [], 0
    for L in range(lmax + 1):
        first.append(t)
        per = (64 // lpr) * (8 if L == 0 else max(1, 8 // L))
        t += -(-int((deg == L).sum()) // per)
    return t, int((deg <= lmax).sum()), first
